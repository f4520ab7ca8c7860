// DDIM / DDPM sampling as ONE native call: the loop of /root/reference/src/sample_trials.py:149-170
// (noise -> [UNet, scheduler.step] x N -> decode(z / scale_factor)) and of sample_trials_ddpm.py:99-104 /
// util.py:261-285 (pixel-space model, 1000-step ancestral sampler).  Host code only.
//
// The reference samples ONE window per call (sample_trials.py:149-163).  At batch 1 a UNet forward is ~130 dependent launches whose
// own latency (not the host's launch rate: the rocprofv3 trace shows them back to back) sets the time per step, so the work went
// into the kernels of that chain (conv_skinny.hip, few-slab GroupNorm) and into taking launches out of the step: the
// embedding rows of all timesteps are computed once per run (below).  The forward CAN be replayed from a hipGraph captured once per
// (B, L) (activation arena, timestep buffer and latent buffer have fixed addresses) -- opt-in, because ROCm's graph launch measured
// slower than the eager launches at B = 1 and equal at B = 256.
#include <map>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>

#include "net.h"

namespace {
struct GraphKey { const eegldm_unet* u; int B, L; bool operator<(const GraphKey& o) const { return std::tie(u, B, L) < std::tie(o.u, o.B, o.L); } };
struct SamplerState {
  hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr;
  float *x = nullptr, *out = nullptr, *nz = nullptr; int64_t* tt = nullptr;
  float* hist = nullptr;         // multistep solver: the previous step's data prediction, one value per latent (allocated on first use)
  // long recordings: the canvas and its history (at most as many values as the window rows hold), the decoded windows ahead of the cross-fade
  float *canvas = nullptr, *chist = nullptr, *dec = nullptr; size_t dec_cap = 0;
  hipStream_t stream = nullptr; hipEvent_t ev_in = nullptr, ev_out = nullptr;
  bool capture_failed = false;
  // embedding rows of all timesteps of a run (eager path): table [emb_cap][etot], scratch of the embedding MLP, timesteps on the device
  float *emb_table = nullptr, *emb_work = nullptr; int64_t* steps_dev = nullptr; int emb_cap = 0;
  float* emb_row = nullptr;      // graph path: the ONE row the captured forward reads; the step's table row is copied here before every replay
  // how `exec` was captured: 0 = recomputing the embedding from s.tt (and s.lab), 1 = reading emb_row, 2 = reading emb_rows -- a replay in
  // another mode would use a stale timestep
  int exec_mode = -1;
  // class labels: one per forward row ([labels | null_class x B] with guidance), on the device and the host copy they came from; the table
  // then has K rows per step (tab_t / tab_y: the (timestep, class) of each row) and emb_rows [rows][etot] receives each step's gathered rows
  int64_t* lab = nullptr; std::vector<int64_t> lab_host, tab_t, tab_y; int64_t* tab_y_dev = nullptr; float* emb_rows = nullptr;
  // context UNets: the context of every forward row (one row per forward row, zeros without a context).  The handle points HERE for the
  // duration of a call, never at the caller's buffer: a captured graph outlives the call and keeps reading this address
  float* cx = nullptr;
};
std::map<GraphKey, SamplerState>& states() { static std::map<GraphKey, SamplerState> m; return m; }
// guards the map AND serialises eegldm_sample: a call swaps ctx->stream for its duration, so two concurrent calls on contexts that
// share a UNet -- or any other call on the same context from a second thread -- are not supported (one context = one thread,
// include/eegldm.h); the lock at least keeps the graph cache consistent when independent contexts sample from different threads
std::recursive_mutex& states_mutex() { static std::recursive_mutex m; return m; }

__global__ void fill_i64_kernel(int64_t* p, int n, int64_t v) { const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = v; }
}  // namespace

void sampler_release(const eegldm_unet* u) {
  std::lock_guard<std::recursive_mutex> lock(states_mutex());
  auto& m = states();
  for (auto it = m.begin(); it != m.end();) {
    if (it->first.u != u) { ++it; continue; }
    SamplerState& s = it->second;
    if (s.exec) (void)hipGraphExecDestroy(s.exec);
    if (s.graph) (void)hipGraphDestroy(s.graph);
    if (s.x) (void)hipFree(s.x);
    if (s.out) (void)hipFree(s.out);
    if (s.nz) (void)hipFree(s.nz);
    if (s.hist) (void)hipFree(s.hist);
    if (s.canvas) (void)hipFree(s.canvas);
    if (s.chist) (void)hipFree(s.chist);
    if (s.dec) (void)hipFree(s.dec);
    if (s.tt) (void)hipFree(s.tt);
    if (s.emb_table) (void)hipFree(s.emb_table);
    if (s.emb_work) (void)hipFree(s.emb_work);
    if (s.steps_dev) (void)hipFree(s.steps_dev);
    if (s.emb_row) (void)hipFree(s.emb_row);
    if (s.lab) (void)hipFree(s.lab);
    if (s.tab_y_dev) (void)hipFree(s.tab_y_dev);
    if (s.emb_rows) (void)hipFree(s.emb_rows);
    if (s.cx) (void)hipFree(s.cx);
    if (s.ev_in) (void)hipEventDestroy(s.ev_in);
    if (s.ev_out) (void)hipEventDestroy(s.ev_out);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    it = m.erase(it);
  }
}

// labels (class-conditional UNets; NULL otherwise): one class per sample.  guidance_scale != 1 runs every forward on 2B rows -- the B
// samples with their labels, then the same latents with null_class -- and mixes the two outputs inside the scheduler step (cfg_step_kernel)
// ms (eegldm_sample_multistep; NULL otherwise): the per-step coefficients of the linear multistep update, which then replaces the DDIM /
// DDPM step -- one eegldm_multistep_step launch behind every forward; a_prev / beta_t / ancestral are not read
struct MultistepCoef { const float *cx, *c0, *c1; };
// ed (eegldm_sample_edit; NULL otherwise): x starts from `known` noised to a_t[0] with `noise` instead of from `noise`; with a mask, every
// step is one eegldm_edit_step launch -- the same step plus the blend towards `known` noised to the level the step lands on (a_prev, or
// a_next[i] in the multistep form); mask NULL: the same launch without the blend.
struct EditBlock { const float *known, *mask, *a_next; };
// lg (eegldm_sample_long; NULL otherwise; needs ms): the B = R * W forward rows are overlapping slices of R canvases (window length L,
// margin m, ramp r: include/eegldm.h).  `noise` is canvas-shaped, x starts as its slices, and every step is one eegldm_canvas_step launch,
// which updates the canvas AND rewrites the slices the next forward reads.  latents_out / windows_out are not used: the canvas goes to
// canvas_out, the cross-faded decode (pixel-space model: the canvas itself) to recording_out.
// lg and ed together (eegldm_sample_long_edit): known / mask are canvas-shaped, the canvas starts as `known` noised to a_t[0] with `noise`,
// and every step is one eegldm_canvas_edit_step launch (the canvas step and the blend; mask NULL: the canvas step alone).
struct LongBlock { int R, W, m, r; float *canvas_out, *recording_out; };
// rs (eegldm_sample_edit_resample / eegldm_sample_long_edit_resample; NULL otherwise; needs ed with a mask -- resample_preamble checks
// that, both jump arrays and the entries behind a jump before the block is built): every host array holds one
// entry per FORWARD, and in front of the forwards with jump_n[i] != 0 one eegldm_edit_jump launch takes x -- the canvas, then a gather --
// back up to the level a_t[i] with noise drawn inside the kernel: Philox key `seed`, jump k of the call at offset k * ceil(elements / 4).
// The hist buffers are not cleared: c1[i] == 0 behind a jump keeps the step from reading them.
struct ResampleBlock { const float *jump_x, *jump_n; uint64_t seed; };
// context / context_rows (eegldm_sample_edit_ctx / eegldm_sample_long_edit_ctx on a UNet from eegldm_unet_create_ctx; NULL otherwise): device
// (rows, context_channels, L) with B % rows == 0 -- sample b reads row b % rows -- or, with lg, canvas-shaped (R, context_channels, Lc), gathered
// once into window rows.  The loop copies it into the state's own buffer (one row per forward row, both halves of a guided batch) and
// points the handle there; a context UNet without a context runs on zeros.
// One call of the loop.  The exports fill the leading members in the order of their own argument lists and name the rest.
struct SampleCall {
  eegldm_unet* u; eegldm_aekl* ae; const float* noise; const int64_t* timesteps; const float* a_t; int n_steps, pred_type, clip_sample;
  float inv_scale_factor; float *latents_out, *windows_out; int B, L, use_graph; int* graph_used; const int64_t* labels; float guidance_scale;
  int64_t null_class;
  const float *a_prev = nullptr, *beta_t = nullptr; int ancestral = 0; uint64_t noise_seed = 0;      // the DDIM / DDPM step
  const MultistepCoef* ms = nullptr; const EditBlock* ed = nullptr; const LongBlock* lg = nullptr; const ResampleBlock* rs = nullptr;
  const float* context = nullptr; int context_rows = 0;
};
static int sample_impl(const SampleCall& q) {
  eegldm_unet* const u = q.u; eegldm_aekl* const ae = q.ae;
  const int B = q.B, L = q.L;
  const MultistepCoef* const ms = q.ms; const EditBlock* const ed = q.ed; const LongBlock* const lg = q.lg; const ResampleBlock* const rs = q.rs;
  EEG_CHECK(u && q.noise && q.timesteps && q.a_t && (q.a_prev || ms), "null argument");
  EEG_CHECK(!q.ancestral || q.beta_t, "the ancestral (DDPM) step needs beta_t");
  EEG_CHECK(q.n_steps >= 1 && B >= 1 && L >= 1, "bad sizes");
  EEG_CHECK(lg || q.latents_out || q.windows_out, "nothing to return: pass latents_out and/or windows_out");
  EEG_CHECK(!lg || (ms && lg->R >= 1 && lg->W >= 1 && (long)lg->R * lg->W == B), "the canvas form needs the multistep coefficients and B == R * W");
  EEG_CHECK(!lg || lg->canvas_out || lg->recording_out, "nothing to return: pass canvas_out and/or recording_out");
  EEG_CHECK(!ed || (ed->known && !q.ancestral), "editing needs the known signal and a deterministic step");
  EEG_CHECK(!ed || !ms || ed->a_next, "the multistep form needs a_next");
  eegldm_ctx* ctx = unet_ctx(u);
  const int C = unet_x_channels(u), Cc = unet_context_channels(u);
  EEG_CHECK(unet_out_channels(u) == C, "sampling needs x channels == out_channels");
  EEG_CHECK(!q.context || Cc > 0, "a context for a UNet built without context channels");
  EEG_CHECK(!q.context || (lg ? q.context_rows == lg->R : (q.context_rows >= 1 && B % q.context_rows == 0)),
            "%d context rows: the canvas form needs one per recording, the others a divisor of B = %d", q.context_rows, B);
  EEG_CHECK(!ae || aekl_ctx(ae) == ctx, "the autoencoder and the UNet must share one context");
  const int K = unet_num_classes(u);
  const bool cond = q.labels != nullptr;
  const bool guided = cond && q.guidance_scale != 1.0f;      // w == 1 is the plain conditional sampler: the null-class half is not run
  const int Bf = guided ? 2 * B : B;                        // rows of every forward
  bool shared = true;                                       // every forward row reads the same embedding row (row stride 0)
  if (cond) {
    for (int b = 0; b < B; b++) {
      EEG_CHECK(q.labels[b] >= 0 && q.labels[b] < K, "label %lld of sample %d outside [0, %d)", (long long)q.labels[b], b, K);
      if (q.labels[b] != q.labels[0]) shared = false;
    }
    if (guided) { EEG_CHECK(q.null_class >= 0 && q.null_class < K, "null_class %lld outside [0, %d)", (long long)q.null_class, K); shared = false; }
  }
  const long n = (long)B * C * L, nf = (long)Bf * C * L;
  std::lock_guard<std::recursive_mutex> lock(states_mutex());
  SamplerState& s = states()[GraphKey{u, Bf, L}];
  if (!s.x) {
    // (nz too holds nf values: a guided call with B samples and a plain one with 2B share this state)
    HIP_TRY(hipMalloc(&s.x, sizeof(float) * nf)); HIP_TRY(hipMalloc(&s.out, sizeof(float) * nf)); HIP_TRY(hipMalloc(&s.nz, sizeof(float) * nf));
    HIP_TRY(hipMalloc(&s.tt, sizeof(int64_t) * Bf));
    HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&s.ev_out, hipEventDisableTiming));
  }
  if (cond && !s.lab) HIP_TRY(hipMalloc(&s.lab, sizeof(int64_t) * Bf));
  const long ncx = (long)B * Cc * L;                                 // context values of one half of the forward rows
  if (Cc > 0 && !s.cx) HIP_TRY(hipMalloc(&s.cx, sizeof(float) * (size_t)Bf * Cc * L));
  if (ms && !lg && !s.hist) HIP_TRY(hipMalloc(&s.hist, sizeof(float) * nf));      // (nf: the state is shared like nz)
  const int Sl = lg ? L - (2 * lg->m + lg->r) : 0;                 // (checked by the first eegldm_canvas_gather / eegldm_canvas_step below)
  const long Lc = lg ? (long)(lg->W - 1) * Sl + L : 0, ncv = lg ? (long)lg->R * C * Lc : 0;
  if (lg) {
    EEG_CHECK(lg->m >= 0 && lg->r >= 0 && (long)L >= 3L * lg->m + 2L * lg->r && Sl >= 1, "window length %d, margin %d, ramp %d: needs m, r >= 0 and L >= 3 m + 2 r", L, lg->m, lg->r);
    if (!s.canvas) { HIP_TRY(hipMalloc(&s.canvas, sizeof(float) * nf)); HIP_TRY(hipMalloc(&s.chist, sizeof(float) * nf)); }      // (ncv <= n <= nf)
  }
  // the whole loop runs on the sampler's own stream (a capture cannot start on the NULL stream the caller may have given the context):
  // it waits for the caller's stream first and the caller's stream waits for it at the end
  hipStream_t caller = ctx->stream;
  struct Restore { eegldm_ctx* c; hipStream_t s; ~Restore() { c->stream = s; } } restore{ctx, caller};
  // Eager launches (the default) stay on the caller's stream: a second stream is a second hardware queue, and alternating queues
  // measured +8 % on the one-window chain (47.5 vs 51.8 ms, the same as GPU_MAX_HW_QUEUES=1 gives with the own stream).
  EEG_ENV_VAR(bool, force_own, getenv("EEGLDM_SAMPLE_OWN_STREAM") != nullptr);
  const bool own = q.use_graph || force_own;
  const hipStream_t run = own ? s.stream : caller;
  if (own) {
    HIP_TRY(hipEventRecord(s.ev_in, caller));
    HIP_TRY(hipStreamWaitEvent(s.stream, s.ev_in, 0));
  }
  ctx->stream = run;
  if (lg) {
    if (ed) EEG_TRY(eegldm_edit_start(ctx, ed->known, 1.0f, q.noise, q.a_t[0], nullptr, s.canvas, ncv));
    else HIP_TRY(hipMemcpyAsync(s.canvas, q.noise, sizeof(float) * ncv, hipMemcpyDeviceToDevice, run));
    EEG_TRY(eegldm_canvas_gather(ctx, s.canvas, lg->R, C, lg->W, L, Sl, s.x, guided ? s.x + n : nullptr));
  } else if (ed) EEG_TRY(eegldm_edit_start(ctx, ed->known, 1.0f, q.noise, q.a_t[0], nullptr, s.x, n));
  else HIP_TRY(hipMemcpyAsync(s.x, q.noise, sizeof(float) * n, hipMemcpyDeviceToDevice, run));
  if (guided && !lg) HIP_TRY(hipMemcpyAsync(s.x + n, ed ? s.x : q.noise, sizeof(float) * n, hipMemcpyDeviceToDevice, run));     // the null-class half: same latents
  struct ClearContext { eegldm_unet* u; ~ClearContext() { if (u) (void)eegldm_unet_set_context(u, nullptr, 0); } } clear_context{Cc > 0 ? u : nullptr};
  if (Cc > 0) {
    if (!q.context) HIP_TRY(hipMemsetAsync(s.cx, 0, sizeof(float) * (size_t)Bf * Cc * L, run));
    else if (lg) EEG_TRY(eegldm_canvas_gather(ctx, q.context, lg->R, Cc, lg->W, L, Sl, s.cx, guided ? s.cx + ncx : nullptr));
    else {
      const long nrow = (long)q.context_rows * Cc * L;
      for (long k = 0; k < (long)Bf / q.context_rows; k++)
        HIP_TRY(hipMemcpyAsync(s.cx + k * nrow, q.context, sizeof(float) * nrow, hipMemcpyDeviceToDevice, run));
    }
    EEG_TRY(eegldm_unet_set_context(u, s.cx, Bf));
  }
  if (cond) {
    HIP_TRY(hipStreamSynchronize(run));             // (the host arrays below are rewritten: an earlier call's copies from them must be done)
    s.lab_host.assign(q.labels, q.labels + B);
    if (guided) s.lab_host.resize(Bf, q.null_class);
    HIP_TRY(hipMemcpyAsync(s.lab, s.lab_host.data(), sizeof(int64_t) * Bf, hipMemcpyHostToDevice, run));
  }
  const int64_t* fwd_lab = cond ? s.lab : nullptr;

  auto set_t = [&](int64_t t) { hipLaunchKernelGGL(fill_i64_kernel, dim3((Bf + 255) / 256), dim3(256), 0, run, s.tt, Bf, t); };
  bool graph_ok = false;
  const int etot = unet_emb_width(u);
  struct ClearEmb { eegldm_unet* u; ~ClearEmb() { unet_set_shared_emb(u, nullptr, 0); } } clear_emb{u};
  EEG_ENV_VAR(bool, no_table, getenv("EEGLDM_SAMPLE_NO_EMB_TABLE") != nullptr);
  const bool table = !no_table;
  const int mode = !table ? 0 : (shared ? 1 : 2);
  if (mode == 2 && !s.emb_rows) HIP_TRY(hipMalloc(&s.emb_rows, sizeof(float) * (size_t)Bf * etot));
  if (q.use_graph && !ctx->prof_on && !s.capture_failed) {
    // Round 5: the captured forward reads its embedding projections from ONE fixed row (s.emb_row) that the loop below refills from the
    // table of all timesteps before every replay -- until round 4 the graph path recomputed the embedding MLP and the 21 projections
    // inside every replay (six launches, ~100 us at B = 1: 5 of the 10.6 ms by which the replayed DDIM-50 trailed the eager one).
    // Several classes in one batch: the rows of all forward rows are gathered into s.emb_rows instead (row stride etot).
    if (mode == 1) {
      if (!s.emb_row) HIP_TRY(hipMalloc(&s.emb_row, sizeof(float) * (size_t)etot));
      unet_set_shared_emb(u, s.emb_row, 0);
    } else if (mode == 2) {
      unet_set_shared_emb(u, s.emb_rows, etot);
    }
    if (s.exec && s.exec_mode != mode) {      // captured in another embedding mode: capture again
      (void)hipGraphExecDestroy(s.exec); s.exec = nullptr;
      if (s.graph) { (void)hipGraphDestroy(s.graph); s.graph = nullptr; }
    }
    if (!s.exec) {
      // eager warm-up: grows the arena / workspaces (hipMalloc is not capturable), then capture the identical launch sequence
      set_t(q.timesteps[0]);
      if (mode == 2) HIP_TRY(hipMemsetAsync(s.emb_rows, 0, sizeof(float) * (size_t)Bf * etot, run));
      EEG_TRY(unet_forward_labels(u, s.x, s.tt, fwd_lab, s.out, Bf, L, 0));
      HIP_TRY(hipStreamSynchronize(run));
      int rc = 0;
      if (hipStreamBeginCapture(run, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        rc = unet_forward_labels(u, s.x, s.tt, fwd_lab, s.out, Bf, L, 0);
        hipError_t e = hipStreamEndCapture(run, &s.graph);
        if (rc == 0 && e == hipSuccess && s.graph && hipGraphInstantiate(&s.exec, s.graph, nullptr, nullptr, 0) == hipSuccess) { graph_ok = true; s.exec_mode = mode; }
      }
      if (!graph_ok) {
        (void)hipGetLastError();
        if (s.graph) { (void)hipGraphDestroy(s.graph); s.graph = nullptr; }
        s.exec = nullptr; s.capture_failed = true;
        if (rc) return rc;
      }
    } else graph_ok = true;
  }
  if (q.graph_used) *q.graph_used = graph_ok ? 1 : 0;

  // Eager path: the timesteps are known up front and shared by all samples, so the timestep-embedding MLP and the ResBlocks' embedding
  // projections run ONCE for all n_steps (one batch of n_steps rows) instead of six launches (~100 us at B = 1) inside every step;
  // each forward then reads its step's row with row stride 0.  EEGLDM_SAMPLE_NO_EMB_TABLE=1 restores the per-step computation.
  // A class-conditional UNet: K rows per step (one per class), row i * K + c; the forward reads the row of its one class with row stride 0,
  // or -- several classes or guidance -- each step gathers its rows into s.emb_rows (row stride etot).
  if (!graph_ok) unet_set_shared_emb(u, mode == 2 ? s.emb_rows : nullptr, mode == 2 ? etot : 0);      // (a failed capture falls back to the eager path below)
  const int Kt = cond ? K : 1;
  const int rows = q.n_steps * Kt;
  if (table) {
    if (s.emb_cap < rows) {
      HIP_TRY(hipStreamSynchronize(run));
      if (s.emb_table) (void)hipFree(s.emb_table);
      if (s.emb_work) (void)hipFree(s.emb_work);
      if (s.steps_dev) (void)hipFree(s.steps_dev);
      if (s.tab_y_dev) (void)hipFree(s.tab_y_dev);
      s.emb_table = nullptr; s.emb_work = nullptr; s.steps_dev = nullptr; s.tab_y_dev = nullptr; s.emb_cap = 0;
      HIP_TRY(hipMalloc(&s.emb_table, sizeof(float) * (size_t)rows * etot));
      HIP_TRY(hipMalloc(&s.emb_work, sizeof(float) * (size_t)rows * unet_embed_work_floats(u)));
      HIP_TRY(hipMalloc(&s.steps_dev, sizeof(int64_t) * rows));
      HIP_TRY(hipMalloc(&s.tab_y_dev, sizeof(int64_t) * rows));
      s.emb_cap = rows;
    }
    if (cond) {
      s.tab_t.resize(rows); s.tab_y.resize(rows);
      for (int i = 0; i < q.n_steps; i++) for (int c = 0; c < K; c++) { s.tab_t[(size_t)i * K + c] = q.timesteps[i]; s.tab_y[(size_t)i * K + c] = c; }
      HIP_TRY(hipMemcpyAsync(s.steps_dev, s.tab_t.data(), sizeof(int64_t) * rows, hipMemcpyHostToDevice, run));
      HIP_TRY(hipMemcpyAsync(s.tab_y_dev, s.tab_y.data(), sizeof(int64_t) * rows, hipMemcpyHostToDevice, run));
    } else {
      HIP_TRY(hipMemcpyAsync(s.steps_dev, q.timesteps, sizeof(int64_t) * q.n_steps, hipMemcpyHostToDevice, run));
    }
    EEG_TRY(unet_embed_table(u, s.steps_dev, cond ? s.tab_y_dev : nullptr, rows, s.emb_table, s.emb_work));
    set_t(q.timesteps[0]);                       // s.tt is not read on this path; keep it defined
  }

  const size_t row0 = cond ? (size_t)q.labels[0] : 0;
  uint64_t jump_index = 0;
  for (int i = 0; i < q.n_steps; i++) {
    if (rs && rs->jump_n[i] != 0.0f) {
      if (lg) {
        EEG_TRY(eegldm_edit_jump(ctx, s.canvas, rs->jump_x[i], rs->jump_n[i], nullptr, rs->seed, jump_index * (uint64_t)((ncv + 3) / 4), ed->known,
                                 q.noise, ed->mask, q.a_t[i], s.canvas, nullptr, ncv));
        EEG_TRY(eegldm_canvas_gather(ctx, s.canvas, lg->R, C, lg->W, L, Sl, s.x, guided ? s.x + n : nullptr));
      } else {
        EEG_TRY(eegldm_edit_jump(ctx, s.x, rs->jump_x[i], rs->jump_n[i], nullptr, rs->seed, jump_index * (uint64_t)((n + 3) / 4), ed->known, q.noise,
                                 ed->mask, q.a_t[i], s.x, guided ? s.x + n : nullptr, n));
      }
      jump_index++;
    }
    const float* step_rows = table ? s.emb_table + (size_t)i * Kt * etot : nullptr;
    if (mode == 2) EEG_TRY(ew_emb_gather(ctx, step_rows, s.lab, Kt, etot, s.emb_rows, Bf));
    else if (table && graph_ok) HIP_TRY(hipMemcpyAsync(s.emb_row, step_rows + row0 * etot, sizeof(float) * (size_t)etot, hipMemcpyDeviceToDevice, run));
    else if (table) unet_set_shared_emb(u, step_rows + row0 * etot, 0);
    else set_t(q.timesteps[i]);
    if (graph_ok) HIP_TRY(hipGraphLaunch(s.exec, run));
    else EEG_TRY(unet_forward_labels(u, s.x, s.tt, fwd_lab, s.out, Bf, L, 0));
    if (ed && lg) {
      EEG_TRY(eegldm_canvas_edit_step(ctx, s.out, q.guidance_scale, guided ? 1 : 0, s.canvas, s.chist, q.a_t[i], ed->a_next[i], q.pred_type, q.clip_sample,
                                      ms->cx[i], ms->c0[i], ms->c1[i], lg->R, C, lg->W, L, lg->m, lg->r, ed->known, q.noise, ed->mask, s.canvas, s.x,
                                      guided ? s.x + n : nullptr, nullptr));
      continue;
    }
    if (ed) {      // (without a mask too: an all-zero mask and no mask are then the same bytes in every form)
      const float coef[3] = {ms ? ms->cx[i] : 0.0f, ms ? ms->c0[i] : 0.0f, ms ? ms->c1[i] : 0.0f};
      EEG_TRY(eegldm_edit_step(ctx, s.out, q.guidance_scale, guided ? 1 : 0, s.x, ms ? s.hist : nullptr, q.a_t[i], ms ? ed->a_next[i] : q.a_prev[i],
                               q.pred_type, q.clip_sample, ms ? coef : nullptr, ed->known, q.noise, ed->mask, s.x, guided ? s.x + n : nullptr, nullptr, n));
      continue;
    }
    if (lg) {
      EEG_TRY(eegldm_canvas_step(ctx, s.out, q.guidance_scale, guided ? 1 : 0, s.canvas, s.chist, q.a_t[i], q.pred_type, q.clip_sample, ms->cx[i], ms->c0[i],
                                 ms->c1[i], lg->R, C, lg->W, L, lg->m, lg->r, s.canvas, s.x, guided ? s.x + n : nullptr, nullptr));
      continue;
    }
    if (ms) {
      EEG_TRY(eegldm_multistep_step(ctx, s.out, q.guidance_scale, guided ? 1 : 0, s.x, s.hist, q.a_t[i], q.pred_type, q.clip_sample, ms->cx[i], ms->c0[i],
                                    ms->c1[i], s.x, guided ? s.x + n : nullptr, nullptr, n));
      continue;
    }
    const bool last = q.a_prev[i] >= 1.0f;
    if (q.ancestral && !last) EEG_TRY(eegldm_randn(ctx, s.nz, n, q.noise_seed, (uint64_t)i * (uint64_t)((n + 3) / 4)));
    if (guided) {
      EEG_TRY(eegldm_guided_step(ctx, s.out, q.guidance_scale, s.x, last ? nullptr : s.nz, q.a_t[i], q.a_prev[i], q.ancestral ? q.beta_t[i] : 0.0f,
                                 q.ancestral, q.pred_type, q.clip_sample, s.x, s.x + n, n));
    } else if (q.ancestral) {
      EEG_TRY(eegldm_ddpm_step(ctx, s.out, s.x, last ? nullptr : s.nz, q.a_t[i], q.a_prev[i], q.beta_t[i], q.pred_type, q.clip_sample, s.x, nullptr, n));
    } else {
      EEG_TRY(eegldm_ddim_step(ctx, s.out, s.x, q.a_t[i], q.a_prev[i], q.pred_type, q.clip_sample, s.x, nullptr, n));
    }
  }
  if (lg) {
    if (lg->canvas_out) HIP_TRY(hipMemcpyAsync(lg->canvas_out, s.canvas, sizeof(float) * ncv, hipMemcpyDeviceToDevice, run));
    if (lg->recording_out && !ae) HIP_TRY(hipMemcpyAsync(lg->recording_out, s.canvas, sizeof(float) * ncv, hipMemcpyDeviceToDevice, run));    // pixel space
    if (lg->recording_out && ae) {
      // the slices of the final canvas, decoded window by window (one GroupNorm statistic per 30-s window, as in training), cross-faded
      const int down = aekl_down(ae), Co = aekl_out_channels(ae);
      EEG_TRY(eegldm_canvas_gather(ctx, s.canvas, lg->R, C, lg->W, L, Sl, s.x, nullptr));
      if (q.inv_scale_factor != 1.0f) EEG_TRY(eegldm_axpy(ctx, s.x, s.x, q.inv_scale_factor - 1.0f, n));
      const size_t nd = (size_t)B * Co * L * down;              // (a guided call and a plain one share this state at different B)
      if (s.dec_cap < nd) {
        HIP_TRY(hipStreamSynchronize(run));
        if (s.dec) (void)hipFree(s.dec);
        s.dec = nullptr; s.dec_cap = 0;
        HIP_TRY(hipMalloc(&s.dec, sizeof(float) * nd));
        s.dec_cap = nd;
      }
      EEG_TRY(eegldm_aekl_decode(ae, s.x, s.dec, B, L));
      EEG_TRY(eegldm_canvas_compose(ctx, s.dec, lg->R, Co, lg->W, L * down, Sl * down, lg->m * down, lg->r * down, lg->recording_out));
    }
  }
  if (q.latents_out) HIP_TRY(hipMemcpyAsync(q.latents_out, s.x, sizeof(float) * n, hipMemcpyDeviceToDevice, run));
  if (q.windows_out) {
    if (ae) {
      if (q.inv_scale_factor != 1.0f) EEG_TRY(eegldm_axpy(ctx, s.x, s.x, q.inv_scale_factor - 1.0f, n));     // z / scale_factor (sample_trials.py:166)
      EEG_TRY(eegldm_aekl_decode(ae, s.x, q.windows_out, B, L));
    } else {
      HIP_TRY(hipMemcpyAsync(q.windows_out, s.x, sizeof(float) * n, hipMemcpyDeviceToDevice, run));    // pixel-space model: x IS the window
    }
  }
  if (own) {
    HIP_TRY(hipEventRecord(s.ev_out, run));
    HIP_TRY(hipStreamWaitEvent(caller, s.ev_out, 0));
  }
  return 0;
}

extern "C" int eegldm_sample(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                             const float* a_prev_host, const float* beta_t_host, int n_steps, int ancestral, int pred_type, int clip_sample,
                             float inv_scale_factor, uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                             int* graph_used_host) {
  EEG_CHECK(u, "null argument");
  EEG_CHECK(unet_num_classes(u) == 0, "this UNet is class-conditional: use eegldm_sample_cond");
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, latents_out, windows_out, B, L, use_graph,
               graph_used_host, nullptr, 1.0f, 0};
  q.a_prev = a_prev_host; q.beta_t = beta_t_host; q.ancestral = ancestral; q.noise_seed = noise_seed;
  return sample_impl(q);
}

extern "C" int eegldm_sample_cond(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                                  const float* a_prev_host, const float* beta_t_host, int n_steps, int ancestral, int pred_type, int clip_sample,
                                  float inv_scale_factor, uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                                  int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  EEG_CHECK(u && labels_host, "null argument");
  EEG_CHECK(unet_num_classes(u) > 0, "this UNet was built without classes: use eegldm_sample");
  EEG_CHECK(guidance_scale == guidance_scale, "guidance_scale is NaN");
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, latents_out, windows_out, B, L, use_graph,
               graph_used_host, labels_host, guidance_scale, null_class};
  q.a_prev = a_prev_host; q.beta_t = beta_t_host; q.ancestral = ancestral; q.noise_seed = noise_seed;
  return sample_impl(q);
}

// What the multistep, edit and long exports check ahead of sample_impl.  multistep: the form needs its three coefficient arrays (false: the
// DDIM form of eegldm_sample_edit, which has none).  R, W: the canvas forms' rows, else 1, 1.  step0: how the message names the step without
// a history.  labels_host NULL: an unconditional UNet; non-NULL: a class-conditional one, guidance as in eegldm_sample_cond.
static int sample_preamble(eegldm_unet* u, bool multistep, const float* cx_host, const float* c0_host, const float* c1_host, int n_steps, int R,
                           int W, const char* step0, const int64_t* labels_host, float guidance_scale) {
  EEG_CHECK(u && (!multistep || (cx_host && c0_host && c1_host)), "null argument");
  EEG_CHECK(n_steps >= 1 && R >= 1 && W >= 1, "bad sizes");
  EEG_CHECK((long)R * W <= 0x3fffffffL, "R * W = %ld rows: too many", (long)R * W);
  if (multistep) EEG_CHECK(c1_host[0] == 0.0f, "%s has no history: c1[0] must be 0 (got %g)", step0, (double)c1_host[0]);
  if (labels_host) {
    EEG_CHECK(unet_num_classes(u) > 0, "labels for a UNet built without classes");
    EEG_CHECK(guidance_scale == guidance_scale, "guidance_scale is NaN");
  } else {
    EEG_CHECK(unet_num_classes(u) == 0, "this UNet is class-conditional: pass labels_host");
  }
  return 0;
}

// The same call with a linear multistep solver (DPM-Solver++ 2M, include/eegldm.h) in place of the DDIM / DDPM step.
extern "C" int eegldm_sample_multistep(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                                       const float* cx_host, const float* c0_host, const float* c1_host, int n_steps, int pred_type,
                                       int clip_sample, float inv_scale_factor, float* latents_out, float* windows_out, int B, int L,
                                       int use_graph, int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  EEG_TRY(sample_preamble(u, true, cx_host, c0_host, c1_host, n_steps, 1, 1, "step 0", labels_host, guidance_scale));
  const MultistepCoef ms{cx_host, c0_host, c1_host};
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, latents_out, windows_out, B, L, use_graph,
               graph_used_host, labels_host, labels_host ? guidance_scale : 1.0f, null_class};
  q.ms = &ms;
  return sample_impl(q);
}

// The same loops from an input (include/eegldm.h): cx_host NULL = DDIM, else the multistep form.
extern "C" int eegldm_sample_edit(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                  const int64_t* timesteps_host, const float* a_t_host, const float* a_prev_host, const float* cx_host,
                                  const float* c0_host, const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                  float inv_scale_factor, float* latents_out, float* windows_out, int B, int L, int use_graph, int* graph_used_host,
                                  const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  EEG_TRY(sample_preamble(u, cx_host != nullptr, cx_host, c0_host, c1_host, n_steps, 1, 1, "the first executed step", labels_host, guidance_scale));
  EEG_CHECK(known || !mask, "a mask needs the known signal");
  EEG_CHECK(cx_host || a_prev_host, "the DDIM form needs a_prev_host");
  EEG_CHECK(!cx_host || !known || a_next_host, "the multistep form needs a_next_host");
  const MultistepCoef ms{cx_host, c0_host, c1_host};
  const EditBlock ed{known, mask, a_next_host};
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, latents_out, windows_out, B, L, use_graph,
               graph_used_host, labels_host, labels_host ? guidance_scale : 1.0f, null_class};
  if (cx_host) q.ms = &ms; else q.a_prev = a_prev_host;
  if (known) q.ed = &ed;
  return sample_impl(q);
}

// Long recordings (include/eegldm.h): R canvases of W overlapping windows each, sampled as one batch of R * W rows.
extern "C" int eegldm_sample_long(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                                  const float* cx_host, const float* c0_host, const float* c1_host, int n_steps, int pred_type, int clip_sample,
                                  float inv_scale_factor, float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                                  int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  return eegldm_sample_long_edit(u, ae, noise, nullptr, nullptr, timesteps_host, a_t_host, cx_host, c0_host, c1_host, nullptr, n_steps, pred_type,
                                 clip_sample, inv_scale_factor, canvas_out, recording_out, R, W, L, m, r, use_graph, graph_used_host, labels_host,
                                 guidance_scale, null_class);
}

// The same loop from a real recording (include/eegldm.h): the canvas form with the edit block.  known == NULL: the plain form.
extern "C" int eegldm_sample_long_edit(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                       const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                                       const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                       float inv_scale_factor, float* canvas_out, float* recording_out, int R, int W, int L, int m, int r,
                                       int use_graph, int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  EEG_CHECK(known || !mask, "a mask needs the known signal");
  EEG_CHECK(!known || a_next_host, "the run from an input needs a_next_host");
  EEG_TRY(sample_preamble(u, true, cx_host, c0_host, c1_host, n_steps, R, W, known ? "the first executed step" : "step 0", labels_host,
                          guidance_scale));
  const MultistepCoef ms{cx_host, c0_host, c1_host};
  const EditBlock ed{known, mask, a_next_host};
  const LongBlock lg{R, W, m, r, canvas_out, recording_out};
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, nullptr, nullptr, R * W, L, use_graph,
               graph_used_host, labels_host, labels_host ? guidance_scale : 1.0f, null_class};
  q.ms = &ms; q.lg = &lg;
  if (known) q.ed = &ed;
  return sample_impl(q);
}

// What the resampling exports check ahead of the loop (include/eegldm.h): both jump arrays, no jump in front of the first forward, no
// history read behind a jump, and the known signal with its mask.
static int resample_preamble(const float* jump_x_host, const float* jump_n_host, const float* c1_host, int n_steps, const float* known,
                             const float* mask) {
  EEG_CHECK(jump_x_host && jump_n_host, "jump_x_host and jump_n_host must both be NULL or both be set");
  EEG_CHECK(known && mask, "resampling needs the known signal and the mask");
  EEG_CHECK(n_steps >= 1, "bad sizes");
  EEG_CHECK(jump_n_host[0] == 0.0f, "no jump can stand in front of the first forward (jump_n[0] = %g)", (double)jump_n_host[0]);
  for (int i = 0; i < n_steps; i++) {
    EEG_CHECK(jump_x_host[i] == jump_x_host[i] && jump_n_host[i] == jump_n_host[i], "jump coefficient %d is NaN", i);
    EEG_CHECK(jump_n_host[i] == 0.0f || !c1_host || c1_host[i] == 0.0f, "the step behind the jump at entry %d has no history: c1 must be 0 (got %g)", i,
              (double)c1_host[i]);
  }
  return 0;
}

// Resampled repair (include/eegldm.h): eegldm_sample_edit with one entry per forward and a jump in front of some of them.
extern "C" int eegldm_sample_edit_resample(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                           const int64_t* timesteps_host, const float* a_t_host, const float* a_prev_host, const float* cx_host,
                                           const float* c0_host, const float* c1_host, const float* a_next_host, int n_steps, int pred_type,
                                           int clip_sample, float inv_scale_factor, const float* jump_x_host, const float* jump_n_host,
                                           uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                                           int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  if (!jump_x_host && !jump_n_host)
    return eegldm_sample_edit(u, ae, noise, known, mask, timesteps_host, a_t_host, a_prev_host, cx_host, c0_host, c1_host, a_next_host, n_steps,
                              pred_type, clip_sample, inv_scale_factor, latents_out, windows_out, B, L, use_graph, graph_used_host, labels_host,
                              guidance_scale, null_class);
  EEG_TRY(sample_preamble(u, cx_host != nullptr, cx_host, c0_host, c1_host, n_steps, 1, 1, "the first executed step", labels_host, guidance_scale));
  EEG_TRY(resample_preamble(jump_x_host, jump_n_host, cx_host ? c1_host : nullptr, n_steps, known, mask));
  EEG_CHECK(cx_host || a_prev_host, "the DDIM form needs a_prev_host");
  EEG_CHECK(!cx_host || a_next_host, "the multistep form needs a_next_host");
  const MultistepCoef ms{cx_host, c0_host, c1_host};
  const EditBlock ed{known, mask, a_next_host};
  const ResampleBlock rs{jump_x_host, jump_n_host, noise_seed};
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, latents_out, windows_out, B, L, use_graph,
               graph_used_host, labels_host, labels_host ? guidance_scale : 1.0f, null_class};
  if (cx_host) q.ms = &ms; else q.a_prev = a_prev_host;
  q.ed = &ed; q.rs = &rs;
  return sample_impl(q);
}

// The same on the canvas: eegldm_sample_long_edit with one entry per forward.
extern "C" int eegldm_sample_long_edit_resample(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                                const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                                                const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                                float inv_scale_factor, const float* jump_x_host, const float* jump_n_host, uint64_t noise_seed,
                                                float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                                                int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  if (!jump_x_host && !jump_n_host)
    return eegldm_sample_long_edit(u, ae, noise, known, mask, timesteps_host, a_t_host, cx_host, c0_host, c1_host, a_next_host, n_steps, pred_type,
                                   clip_sample, inv_scale_factor, canvas_out, recording_out, R, W, L, m, r, use_graph, graph_used_host, labels_host,
                                   guidance_scale, null_class);
  EEG_CHECK(a_next_host, "the run from an input needs a_next_host");
  EEG_TRY(sample_preamble(u, true, cx_host, c0_host, c1_host, n_steps, R, W, "the first executed step", labels_host, guidance_scale));
  EEG_TRY(resample_preamble(jump_x_host, jump_n_host, c1_host, n_steps, known, mask));
  const MultistepCoef ms{cx_host, c0_host, c1_host};
  const EditBlock ed{known, mask, a_next_host};
  const LongBlock lg{R, W, m, r, canvas_out, recording_out};
  const ResampleBlock rs{jump_x_host, jump_n_host, noise_seed};
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, nullptr, nullptr, R * W, L, use_graph,
               graph_used_host, labels_host, labels_host ? guidance_scale : 1.0f, null_class};
  q.ms = &ms; q.lg = &lg; q.ed = &ed; q.rs = &rs;
  return sample_impl(q);
}

// Learned repair (include/eegldm.h): the two exports above on a context UNet, with the context every forward reads.  context == NULL is the
// predecessor itself (a context UNet then runs on zeros); jump_x_host == jump_n_host == NULL is the plain edit loop with a context.
extern "C" int eegldm_sample_edit_ctx(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                      const int64_t* timesteps_host, const float* a_t_host, const float* a_prev_host, const float* cx_host,
                                      const float* c0_host, const float* c1_host, const float* a_next_host, int n_steps, int pred_type,
                                      int clip_sample, float inv_scale_factor, const float* jump_x_host, const float* jump_n_host,
                                      uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                                      int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class,
                                      const float* context, int context_rows) {
  if (!context)
    return eegldm_sample_edit_resample(u, ae, noise, known, mask, timesteps_host, a_t_host, a_prev_host, cx_host, c0_host, c1_host, a_next_host,
                                       n_steps, pred_type, clip_sample, inv_scale_factor, jump_x_host, jump_n_host, noise_seed, latents_out,
                                       windows_out, B, L, use_graph, graph_used_host, labels_host, guidance_scale, null_class);
  const bool jumps = jump_x_host || jump_n_host;
  EEG_TRY(sample_preamble(u, cx_host != nullptr, cx_host, c0_host, c1_host, n_steps, 1, 1, "the first executed step", labels_host, guidance_scale));
  if (jumps) EEG_TRY(resample_preamble(jump_x_host, jump_n_host, cx_host ? c1_host : nullptr, n_steps, known, mask));
  EEG_CHECK(known || !mask, "a mask needs the known signal");
  EEG_CHECK(cx_host || a_prev_host, "the DDIM form needs a_prev_host");
  EEG_CHECK(!cx_host || !known || a_next_host, "the multistep form needs a_next_host");
  const MultistepCoef ms{cx_host, c0_host, c1_host};
  const EditBlock ed{known, mask, a_next_host};
  const ResampleBlock rs{jump_x_host, jump_n_host, noise_seed};
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, latents_out, windows_out, B, L, use_graph,
               graph_used_host, labels_host, labels_host ? guidance_scale : 1.0f, null_class};
  if (cx_host) q.ms = &ms; else q.a_prev = a_prev_host;
  if (known) q.ed = &ed;
  if (jumps) q.rs = &rs;
  q.context = context; q.context_rows = context_rows;
  return sample_impl(q);
}

// The same on the canvas: context is canvas-shaped (R, context_channels, Lc), gathered once per call into window rows.
extern "C" int eegldm_sample_long_edit_ctx(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                           const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                                           const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                           float inv_scale_factor, const float* jump_x_host, const float* jump_n_host, uint64_t noise_seed,
                                           float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                                           int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class,
                                           const float* context, int context_rows) {
  if (!context)
    return eegldm_sample_long_edit_resample(u, ae, noise, known, mask, timesteps_host, a_t_host, cx_host, c0_host, c1_host, a_next_host, n_steps,
                                            pred_type, clip_sample, inv_scale_factor, jump_x_host, jump_n_host, noise_seed, canvas_out, recording_out,
                                            R, W, L, m, r, use_graph, graph_used_host, labels_host, guidance_scale, null_class);
  const bool jumps = jump_x_host || jump_n_host;
  EEG_CHECK(known || !mask, "a mask needs the known signal");
  EEG_CHECK(!known || a_next_host, "the run from an input needs a_next_host");
  EEG_TRY(sample_preamble(u, true, cx_host, c0_host, c1_host, n_steps, R, W, known ? "the first executed step" : "step 0", labels_host,
                          guidance_scale));
  if (jumps) EEG_TRY(resample_preamble(jump_x_host, jump_n_host, c1_host, n_steps, known, mask));
  const MultistepCoef ms{cx_host, c0_host, c1_host};
  const EditBlock ed{known, mask, a_next_host};
  const LongBlock lg{R, W, m, r, canvas_out, recording_out};
  const ResampleBlock rs{jump_x_host, jump_n_host, noise_seed};
  SampleCall q{u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, nullptr, nullptr, R * W, L, use_graph,
               graph_used_host, labels_host, labels_host ? guidance_scale : 1.0f, null_class};
  q.ms = &ms; q.lg = &lg;
  if (known) q.ed = &ed;
  if (jumps) q.rs = &rs;
  q.context = context; q.context_rows = context_rows;
  return sample_impl(q);
}
