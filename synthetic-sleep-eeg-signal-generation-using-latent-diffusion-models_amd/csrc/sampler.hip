// DDIM / DDPM sampling as ONE native call: the loop of the reference's src/sample_trials.py:149-170
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


// Every precondition of a call of the loop, each stated once; include/eegldm.h (eegldm_sample_desc) describes the groups.  Host reads only:
// it runs ahead of the state lock and of every launch and allocation, so a refused call leaves nothing behind.
static int sample_check(const eegldm_sample_desc& d) {
  eegldm_unet* const u = d.unet;
  const bool ms = d.cx != nullptr, ed = d.known != nullptr, lg = d.R > 0;
  // null handles and arrays
  EEG_CHECK(u, "null argument: unet");
  EEG_CHECK(d.noise && d.timesteps && d.a_t, "null argument: noise, timesteps and a_t are required");
  // sizes
  EEG_CHECK(d.n_steps >= 1 && d.L >= 1 && (lg ? d.W >= 1 : d.B >= 1), "bad sizes");
  EEG_CHECK(!lg || (long)d.R * d.W <= 0x3fffffffL, "R * W = %ld rows: too many", (long)d.R * d.W);
  const int B = lg ? d.R * d.W : d.B;
  // exactly one step form: DDIM (a_prev), DDPM (a_prev, ancestral, beta_t) or multistep (cx, c0, c1)
  EEG_CHECK(ms ? (d.c0 && d.c1) : d.a_prev != nullptr, "null argument: the step needs a_prev (DDIM / DDPM) or cx, c0 and c1 (multistep)");
  EEG_CHECK(!d.ancestral || !ms, "the ancestral (DDPM) step and the multistep coefficients exclude each other");
  EEG_CHECK(!d.ancestral || d.beta_t, "null argument: the ancestral (DDPM) step needs beta_t");
  EEG_CHECK(!d.ancestral || !ed, "editing (known) needs a deterministic step");
  EEG_CHECK(!ms || d.c1[0] == 0.0f, "the first executed step has no history: c1[0] must be 0 (got %g)", ms ? (double)d.c1[0] : 0.0);
  // classes
  const int K = unet_num_classes(u);
  if (d.labels) {
    EEG_CHECK(K > 0, "labels for a UNet built without classes");
    EEG_CHECK(d.guidance_scale == d.guidance_scale, "guidance_scale is NaN");
    for (int b = 0; b < B; b++) EEG_CHECK(d.labels[b] >= 0 && d.labels[b] < K, "label %lld of sample %d outside [0, %d)", (long long)d.labels[b], b, K);
    EEG_CHECK(d.guidance_scale == 1.0f || (d.null_class >= 0 && d.null_class < K), "null_class %lld outside [0, %d)", (long long)d.null_class, K);
  } else {
    EEG_CHECK(K == 0, "this UNet is class-conditional: pass labels");
  }
  // edit
  EEG_CHECK(ed || !d.mask, "a mask needs the known signal");
  EEG_CHECK(!ed || !ms || d.a_next, "null argument: known with the multistep step needs a_next");
  // canvas
  EEG_CHECK(!lg || ms, "the canvas form needs the multistep coefficients");
  EEG_CHECK(!lg || (d.m >= 0 && d.r >= 0 && (long)d.L >= 3L * d.m + 2L * d.r && d.L - (2 * d.m + d.r) >= 1),
            "window length %d, margin %d, ramp %d: needs m, r >= 0 and L >= 3 m + 2 r", d.L, d.m, d.r);
  // something to return
  EEG_CHECK(lg ? (d.canvas_out || d.recording_out) : (d.latents_out || d.windows_out),
            "nothing to return: pass %s", lg ? "canvas_out and/or recording_out" : "latents_out and/or windows_out");
  // jumps
  if (d.jump_x || d.jump_n) {
    EEG_CHECK(d.jump_x && d.jump_n, "null argument: jump_x and jump_n must both be NULL or both be set");
    EEG_CHECK(ed && d.mask, "resampling needs the known signal and the mask");
    EEG_CHECK(d.jump_n[0] == 0.0f, "no jump can stand in front of the first forward (jump_n[0] = %g)", (double)d.jump_n[0]);
    for (int i = 0; i < d.n_steps; i++) {
      EEG_CHECK(d.jump_x[i] == d.jump_x[i] && d.jump_n[i] == d.jump_n[i], "jump coefficient %d is NaN", i);
      EEG_CHECK(d.jump_n[i] == 0.0f || !ms || d.c1[i] == 0.0f, "the step behind the jump at entry %d has no history: c1 must be 0 (got %g)", i,
                ms ? (double)d.c1[i] : 0.0);
    }
  }
  // model and context
  EEG_CHECK(unet_out_channels(u) == unet_x_channels(u), "sampling needs x channels == out_channels");
  EEG_CHECK(!d.ae || aekl_ctx(d.ae) == unet_ctx(u), "the autoencoder and the UNet must share one context");
  EEG_CHECK(!d.context || unet_context_channels(u) > 0, "a context for a UNet built without context channels");
  EEG_CHECK(!d.context || (lg ? d.context_rows == d.R : (d.context_rows >= 1 && B % d.context_rows == 0)),
            "%d context rows: the canvas form needs one per recording, the others a divisor of B = %d", d.context_rows, B);
  return 0;
}

// The loop itself (include/eegldm.h, eegldm_sample_desc: what each group of members selects).
static int sample_impl(const eegldm_sample_desc& d) {
  EEG_TRY(sample_check(d));
  eegldm_unet* const u = d.unet; eegldm_aekl* const ae = d.ae;
  const bool ms = d.cx != nullptr, ed = d.known != nullptr, lg = d.R > 0, rs = d.jump_n != nullptr;
  const int B = lg ? d.R * d.W : d.B, L = d.L;
  eegldm_ctx* ctx = unet_ctx(u);
  const int C = unet_x_channels(u), Cc = unet_context_channels(u);
  const int K = unet_num_classes(u);
  const bool cond = d.labels != nullptr;
  const float w = cond ? d.guidance_scale : 1.0f;             // (read only with labels: a zeroed descriptor without them is not w = 0)
  const bool guided = cond && w != 1.0f;                    // w == 1 is the plain conditional sampler: the null-class half is not run
  const int Bf = guided ? 2 * B : B;                        // rows of every forward
  bool shared = !guided;                                    // every forward row reads the same embedding row (row stride 0)
  for (int b = 1; cond && b < B; b++) if (d.labels[b] != d.labels[0]) shared = false;
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
  const int Sl = lg ? L - (2 * d.m + d.r) : 0;
  const long Lc = lg ? (long)(d.W - 1) * Sl + L : 0, ncv = lg ? (long)d.R * C * Lc : 0;
  if (lg && !s.canvas) { HIP_TRY(hipMalloc(&s.canvas, sizeof(float) * nf)); HIP_TRY(hipMalloc(&s.chist, sizeof(float) * nf)); }      // (ncv <= n <= nf)
  // the whole loop runs on the sampler's own stream (a capture cannot start on the NULL stream the caller may have given the context):
  // it waits for the caller's stream first and the caller's stream waits for it at the end
  hipStream_t caller = ctx->stream;
  struct Restore { eegldm_ctx* c; hipStream_t s; ~Restore() { c->stream = s; } } restore{ctx, caller};
  // Eager launches (the default) stay on the caller's stream: a second stream is a second hardware queue, and alternating queues
  // measured +8 % on the one-window chain (47.5 vs 51.8 ms, the same as GPU_MAX_HW_QUEUES=1 gives with the own stream).
  EEG_ENV_VAR(bool, force_own, getenv("EEGLDM_SAMPLE_OWN_STREAM") != nullptr);
  const bool own = d.use_graph || force_own;
  const hipStream_t run = own ? s.stream : caller;
  if (own) {
    HIP_TRY(hipEventRecord(s.ev_in, caller));
    HIP_TRY(hipStreamWaitEvent(s.stream, s.ev_in, 0));
  }
  ctx->stream = run;
  if (lg) {
    if (ed) EEG_TRY(eegldm_edit_start(ctx, d.known, 1.0f, d.noise, d.a_t[0], nullptr, s.canvas, ncv));
    else HIP_TRY(hipMemcpyAsync(s.canvas, d.noise, sizeof(float) * ncv, hipMemcpyDeviceToDevice, run));
    EEG_TRY(eegldm_canvas_gather(ctx, s.canvas, d.R, C, d.W, L, Sl, s.x, guided ? s.x + n : nullptr));
  } else if (ed) EEG_TRY(eegldm_edit_start(ctx, d.known, 1.0f, d.noise, d.a_t[0], nullptr, s.x, n));
  else HIP_TRY(hipMemcpyAsync(s.x, d.noise, sizeof(float) * n, hipMemcpyDeviceToDevice, run));
  if (guided && !lg) HIP_TRY(hipMemcpyAsync(s.x + n, ed ? s.x : d.noise, sizeof(float) * n, hipMemcpyDeviceToDevice, run));     // the null-class half: same latents
  struct ClearContext { eegldm_unet* u; ~ClearContext() { if (u) (void)eegldm_unet_set_context(u, nullptr, 0); } } clear_context{Cc > 0 ? u : nullptr};
  if (Cc > 0) {
    if (!d.context) HIP_TRY(hipMemsetAsync(s.cx, 0, sizeof(float) * (size_t)Bf * Cc * L, run));
    else if (lg) EEG_TRY(eegldm_canvas_gather(ctx, d.context, d.R, Cc, d.W, L, Sl, s.cx, guided ? s.cx + ncx : nullptr));
    else {
      const long nrow = (long)d.context_rows * Cc * L;
      for (long k = 0; k < (long)Bf / d.context_rows; k++)
        HIP_TRY(hipMemcpyAsync(s.cx + k * nrow, d.context, sizeof(float) * nrow, hipMemcpyDeviceToDevice, run));
    }
    EEG_TRY(eegldm_unet_set_context(u, s.cx, Bf));
  }
  if (cond) {
    HIP_TRY(hipStreamSynchronize(run));             // (the host arrays below are rewritten: an earlier call's copies from them must be done)
    s.lab_host.assign(d.labels, d.labels + B);
    if (guided) s.lab_host.resize(Bf, d.null_class);
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
  if (d.use_graph && !ctx->prof_on && !s.capture_failed) {
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
      set_t(d.timesteps[0]);
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
  if (d.graph_used) *d.graph_used = graph_ok ? 1 : 0;

  // Eager path: the timesteps are known up front and shared by all samples, so the timestep-embedding MLP and the ResBlocks' embedding
  // projections run ONCE for all n_steps (one batch of n_steps rows) instead of six launches (~100 us at B = 1) inside every step;
  // each forward then reads its step's row with row stride 0.  EEGLDM_SAMPLE_NO_EMB_TABLE=1 restores the per-step computation.
  // A class-conditional UNet: K rows per step (one per class), row i * K + c; the forward reads the row of its one class with row stride 0,
  // or -- several classes or guidance -- each step gathers its rows into s.emb_rows (row stride etot).
  if (!graph_ok) unet_set_shared_emb(u, mode == 2 ? s.emb_rows : nullptr, mode == 2 ? etot : 0);      // (a failed capture falls back to the eager path below)
  const int Kt = cond ? K : 1;
  const int rows = d.n_steps * Kt;
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
      for (int i = 0; i < d.n_steps; i++) for (int c = 0; c < K; c++) { s.tab_t[(size_t)i * K + c] = d.timesteps[i]; s.tab_y[(size_t)i * K + c] = c; }
      HIP_TRY(hipMemcpyAsync(s.steps_dev, s.tab_t.data(), sizeof(int64_t) * rows, hipMemcpyHostToDevice, run));
      HIP_TRY(hipMemcpyAsync(s.tab_y_dev, s.tab_y.data(), sizeof(int64_t) * rows, hipMemcpyHostToDevice, run));
    } else {
      HIP_TRY(hipMemcpyAsync(s.steps_dev, d.timesteps, sizeof(int64_t) * d.n_steps, hipMemcpyHostToDevice, run));
    }
    EEG_TRY(unet_embed_table(u, s.steps_dev, cond ? s.tab_y_dev : nullptr, rows, s.emb_table, s.emb_work));
    set_t(d.timesteps[0]);                       // s.tt is not read on this path; keep it defined
  }

  const size_t row0 = cond ? (size_t)d.labels[0] : 0;
  uint64_t jump_index = 0;
  for (int i = 0; i < d.n_steps; i++) {
    if (rs && d.jump_n[i] != 0.0f) {
      if (lg) {
        EEG_TRY(eegldm_edit_jump(ctx, s.canvas, d.jump_x[i], d.jump_n[i], nullptr, d.noise_seed, jump_index * (uint64_t)((ncv + 3) / 4), d.known,
                                 d.noise, d.mask, d.a_t[i], s.canvas, nullptr, ncv));
        EEG_TRY(eegldm_canvas_gather(ctx, s.canvas, d.R, C, d.W, L, Sl, s.x, guided ? s.x + n : nullptr));
      } else {
        EEG_TRY(eegldm_edit_jump(ctx, s.x, d.jump_x[i], d.jump_n[i], nullptr, d.noise_seed, jump_index * (uint64_t)((n + 3) / 4), d.known, d.noise,
                                 d.mask, d.a_t[i], s.x, guided ? s.x + n : nullptr, n));
      }
      jump_index++;
    }
    const float* step_rows = table ? s.emb_table + (size_t)i * Kt * etot : nullptr;
    if (mode == 2) EEG_TRY(ew_emb_gather(ctx, step_rows, s.lab, Kt, etot, s.emb_rows, Bf));
    else if (table && graph_ok) HIP_TRY(hipMemcpyAsync(s.emb_row, step_rows + row0 * etot, sizeof(float) * (size_t)etot, hipMemcpyDeviceToDevice, run));
    else if (table) unet_set_shared_emb(u, step_rows + row0 * etot, 0);
    else set_t(d.timesteps[i]);
    if (graph_ok) HIP_TRY(hipGraphLaunch(s.exec, run));
    else EEG_TRY(unet_forward_labels(u, s.x, s.tt, fwd_lab, s.out, Bf, L, 0));
    if (ed && lg) {
      EEG_TRY(eegldm_canvas_edit_step(ctx, s.out, w, guided ? 1 : 0, s.canvas, s.chist, d.a_t[i], d.a_next[i], d.pred_type, d.clip_sample, d.cx[i],
                                      d.c0[i], d.c1[i], d.R, C, d.W, L, d.m, d.r, d.known, d.noise, d.mask, s.canvas, s.x, guided ? s.x + n : nullptr,
                                      nullptr));
      continue;
    }
    if (ed) {      // (without a mask too: an all-zero mask and no mask are then the same bytes in every form)
      const float coef[3] = {ms ? d.cx[i] : 0.0f, ms ? d.c0[i] : 0.0f, ms ? d.c1[i] : 0.0f};
      EEG_TRY(eegldm_edit_step(ctx, s.out, w, guided ? 1 : 0, s.x, ms ? s.hist : nullptr, d.a_t[i], ms ? d.a_next[i] : d.a_prev[i], d.pred_type,
                               d.clip_sample, ms ? coef : nullptr, d.known, d.noise, d.mask, s.x, guided ? s.x + n : nullptr, nullptr, n));
      continue;
    }
    if (lg) {
      EEG_TRY(eegldm_canvas_step(ctx, s.out, w, guided ? 1 : 0, s.canvas, s.chist, d.a_t[i], d.pred_type, d.clip_sample, d.cx[i], d.c0[i], d.c1[i], d.R, C,
                                 d.W, L, d.m, d.r, s.canvas, s.x, guided ? s.x + n : nullptr, nullptr));
      continue;
    }
    if (ms) {
      EEG_TRY(eegldm_multistep_step(ctx, s.out, w, guided ? 1 : 0, s.x, s.hist, d.a_t[i], d.pred_type, d.clip_sample, d.cx[i], d.c0[i], d.c1[i], s.x,
                                    guided ? s.x + n : nullptr, nullptr, n));
      continue;
    }
    const bool last = d.a_prev[i] >= 1.0f;
    if (d.ancestral && !last) EEG_TRY(eegldm_randn(ctx, s.nz, n, d.noise_seed, (uint64_t)i * (uint64_t)((n + 3) / 4)));
    if (guided) {
      EEG_TRY(eegldm_guided_step(ctx, s.out, w, s.x, last ? nullptr : s.nz, d.a_t[i], d.a_prev[i], d.ancestral ? d.beta_t[i] : 0.0f, d.ancestral,
                                 d.pred_type, d.clip_sample, s.x, s.x + n, n));
    } else if (d.ancestral) {
      EEG_TRY(eegldm_ddpm_step(ctx, s.out, s.x, last ? nullptr : s.nz, d.a_t[i], d.a_prev[i], d.beta_t[i], d.pred_type, d.clip_sample, s.x, nullptr, n));
    } else {
      EEG_TRY(eegldm_ddim_step(ctx, s.out, s.x, d.a_t[i], d.a_prev[i], d.pred_type, d.clip_sample, s.x, nullptr, n));
    }
  }
  if (lg) {
    if (d.canvas_out) HIP_TRY(hipMemcpyAsync(d.canvas_out, s.canvas, sizeof(float) * ncv, hipMemcpyDeviceToDevice, run));
    if (d.recording_out && !ae) HIP_TRY(hipMemcpyAsync(d.recording_out, s.canvas, sizeof(float) * ncv, hipMemcpyDeviceToDevice, run));    // pixel space
    if (d.recording_out && ae) {
      // the slices of the final canvas, decoded window by window (one GroupNorm statistic per 30-s window, as in training), cross-faded
      const int down = aekl_down(ae), Co = aekl_out_channels(ae);
      EEG_TRY(eegldm_canvas_gather(ctx, s.canvas, d.R, C, d.W, L, Sl, s.x, nullptr));
      if (d.inv_scale_factor != 1.0f) EEG_TRY(eegldm_axpy(ctx, s.x, s.x, d.inv_scale_factor - 1.0f, n));
      const size_t nd = (size_t)B * Co * L * down;              // (a guided call and a plain one share this state at different B)
      if (s.dec_cap < nd) {
        HIP_TRY(hipStreamSynchronize(run));
        if (s.dec) (void)hipFree(s.dec);
        s.dec = nullptr; s.dec_cap = 0;
        HIP_TRY(hipMalloc(&s.dec, sizeof(float) * nd));
        s.dec_cap = nd;
      }
      EEG_TRY(eegldm_aekl_decode(ae, s.x, s.dec, B, L));
      EEG_TRY(eegldm_canvas_compose(ctx, s.dec, d.R, Co, d.W, L * down, Sl * down, d.m * down, d.r * down, d.recording_out));
    }
  }
  if (!lg && d.latents_out) HIP_TRY(hipMemcpyAsync(d.latents_out, s.x, sizeof(float) * n, hipMemcpyDeviceToDevice, run));
  if (!lg && d.windows_out) {
    if (ae) {
      if (d.inv_scale_factor != 1.0f) EEG_TRY(eegldm_axpy(ctx, s.x, s.x, d.inv_scale_factor - 1.0f, n));     // z / scale_factor (sample_trials.py:166)
      EEG_TRY(eegldm_aekl_decode(ae, s.x, d.windows_out, B, L));
    } else {
      HIP_TRY(hipMemcpyAsync(d.windows_out, s.x, sizeof(float) * n, hipMemcpyDeviceToDevice, run));    // pixel-space model: x IS the window
    }
  }
  if (own) {
    HIP_TRY(hipEventRecord(s.ev_out, run));
    HIP_TRY(hipStreamWaitEvent(caller, s.ev_out, 0));
  }
  return 0;
}

extern "C" int eegldm_sample_run(const eegldm_sample_desc* desc) {
  EEG_CHECK(desc, "null argument: desc");
  EEG_CHECK(desc->size == sizeof(eegldm_sample_desc), "eegldm_sample_desc.size is %u, this library's is %u", (unsigned)desc->size,
            (unsigned)sizeof(eegldm_sample_desc));
  return sample_impl(*desc);
}

// ---- the positional exports: each fills a descriptor from its argument list (include/eegldm.h) and runs it.  What a NULL optional argument
// means falls out of the descriptor's own NULL semantics; the rules are sample_check's.  The edit and the canvas families stand
// with their widest argument list first.

// The members every export sets.  guidance_scale passes through only with labels.
static eegldm_sample_desc desc_of(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps, const float* a_t, int n_steps,
                                  int pred_type, int clip_sample, float inv_scale_factor, int L, int use_graph, int* graph_used,
                                  const int64_t* labels, float guidance_scale, int64_t null_class) {
  eegldm_sample_desc d = {};
  d.size = sizeof d;
  d.unet = u; d.ae = ae; d.noise = noise; d.L = L;
  d.n_steps = n_steps; d.timesteps = timesteps; d.a_t = a_t;
  d.pred_type = pred_type; d.clip_sample = clip_sample; d.inv_scale_factor = inv_scale_factor;
  d.labels = labels; d.guidance_scale = labels ? guidance_scale : 1.0f; d.null_class = null_class;
  d.use_graph = use_graph; d.graph_used = graph_used;
  return d;
}

extern "C" int eegldm_sample(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                             const float* a_prev_host, const float* beta_t_host, int n_steps, int ancestral, int pred_type, int clip_sample,
                             float inv_scale_factor, uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                             int* graph_used_host) {
  EEG_CHECK(u, "null argument: unet");
  EEG_CHECK(unet_num_classes(u) == 0, "this UNet is class-conditional: use eegldm_sample_cond");
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, nullptr, 1.0f, 0);
  d.B = B; d.latents_out = latents_out; d.windows_out = windows_out;
  d.a_prev = a_prev_host; d.beta_t = beta_t_host; d.ancestral = ancestral; d.noise_seed = noise_seed;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_cond(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                                  const float* a_prev_host, const float* beta_t_host, int n_steps, int ancestral, int pred_type, int clip_sample,
                                  float inv_scale_factor, uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                                  int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  EEG_CHECK(u && labels_host, "null argument: unet and labels_host are required");
  EEG_CHECK(unet_num_classes(u) > 0, "this UNet was built without classes: use eegldm_sample");
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.B = B; d.latents_out = latents_out; d.windows_out = windows_out;
  d.a_prev = a_prev_host; d.beta_t = beta_t_host; d.ancestral = ancestral; d.noise_seed = noise_seed;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_multistep(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                                       const float* cx_host, const float* c0_host, const float* c1_host, int n_steps, int pred_type,
                                       int clip_sample, float inv_scale_factor, float* latents_out, float* windows_out, int B, int L,
                                       int use_graph, int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.B = B; d.latents_out = latents_out; d.windows_out = windows_out;
  d.cx = cx_host; d.c0 = c0_host; d.c1 = c1_host;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_edit_ctx(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                      const int64_t* timesteps_host, const float* a_t_host, const float* a_prev_host, const float* cx_host,
                                      const float* c0_host, const float* c1_host, const float* a_next_host, int n_steps, int pred_type,
                                      int clip_sample, float inv_scale_factor, const float* jump_x_host, const float* jump_n_host,
                                      uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                                      int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class,
                                      const float* context, int context_rows) {
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.B = B; d.latents_out = latents_out; d.windows_out = windows_out;
  d.a_prev = a_prev_host; d.cx = cx_host; d.c0 = c0_host; d.c1 = c1_host; d.a_next = a_next_host;
  d.known = known; d.mask = mask;
  d.jump_x = jump_x_host; d.jump_n = jump_n_host; d.noise_seed = noise_seed;
  d.context = context; d.context_rows = context_rows;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_edit_resample(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                           const int64_t* timesteps_host, const float* a_t_host, const float* a_prev_host, const float* cx_host,
                                           const float* c0_host, const float* c1_host, const float* a_next_host, int n_steps, int pred_type,
                                           int clip_sample, float inv_scale_factor, const float* jump_x_host, const float* jump_n_host,
                                           uint64_t noise_seed, float* latents_out, float* windows_out, int B, int L, int use_graph,
                                           int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.B = B; d.latents_out = latents_out; d.windows_out = windows_out;
  d.a_prev = a_prev_host; d.cx = cx_host; d.c0 = c0_host; d.c1 = c1_host; d.a_next = a_next_host;
  d.known = known; d.mask = mask;
  d.jump_x = jump_x_host; d.jump_n = jump_n_host; d.noise_seed = noise_seed;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_edit(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                  const int64_t* timesteps_host, const float* a_t_host, const float* a_prev_host, const float* cx_host,
                                  const float* c0_host, const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                  float inv_scale_factor, float* latents_out, float* windows_out, int B, int L, int use_graph, int* graph_used_host,
                                  const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.B = B; d.latents_out = latents_out; d.windows_out = windows_out;
  d.a_prev = a_prev_host; d.cx = cx_host; d.c0 = c0_host; d.c1 = c1_host; d.a_next = a_next_host;
  d.known = known; d.mask = mask;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_long_edit_ctx(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                           const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                                           const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                           float inv_scale_factor, const float* jump_x_host, const float* jump_n_host, uint64_t noise_seed,
                                           float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                                           int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class,
                                           const float* context, int context_rows) {
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.R = R; d.W = W; d.m = m; d.r = r; d.canvas_out = canvas_out; d.recording_out = recording_out;
  d.cx = cx_host; d.c0 = c0_host; d.c1 = c1_host; d.a_next = a_next_host;
  d.known = known; d.mask = mask;
  d.jump_x = jump_x_host; d.jump_n = jump_n_host; d.noise_seed = noise_seed;
  d.context = context; d.context_rows = context_rows;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_long_edit_resample(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                                const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                                                const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                                float inv_scale_factor, const float* jump_x_host, const float* jump_n_host, uint64_t noise_seed,
                                                float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                                                int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.R = R; d.W = W; d.m = m; d.r = r; d.canvas_out = canvas_out; d.recording_out = recording_out;
  d.cx = cx_host; d.c0 = c0_host; d.c1 = c1_host; d.a_next = a_next_host;
  d.known = known; d.mask = mask;
  d.jump_x = jump_x_host; d.jump_n = jump_n_host; d.noise_seed = noise_seed;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_long_edit(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const float* known, const float* mask,
                                       const int64_t* timesteps_host, const float* a_t_host, const float* cx_host, const float* c0_host,
                                       const float* c1_host, const float* a_next_host, int n_steps, int pred_type, int clip_sample,
                                       float inv_scale_factor, float* canvas_out, float* recording_out, int R, int W, int L, int m, int r,
                                       int use_graph, int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.R = R; d.W = W; d.m = m; d.r = r; d.canvas_out = canvas_out; d.recording_out = recording_out;
  d.cx = cx_host; d.c0 = c0_host; d.c1 = c1_host; d.a_next = a_next_host;
  d.known = known; d.mask = mask;
  return eegldm_sample_run(&d);
}

extern "C" int eegldm_sample_long(eegldm_unet* u, eegldm_aekl* ae, const float* noise, const int64_t* timesteps_host, const float* a_t_host,
                                  const float* cx_host, const float* c0_host, const float* c1_host, int n_steps, int pred_type, int clip_sample,
                                  float inv_scale_factor, float* canvas_out, float* recording_out, int R, int W, int L, int m, int r, int use_graph,
                                  int* graph_used_host, const int64_t* labels_host, float guidance_scale, int64_t null_class) {
  eegldm_sample_desc d = desc_of(u, ae, noise, timesteps_host, a_t_host, n_steps, pred_type, clip_sample, inv_scale_factor, L, use_graph,
                                 graph_used_host, labels_host, guidance_scale, null_class);
  d.R = R; d.W = W; d.m = m; d.r = r; d.canvas_out = canvas_out; d.recording_out = recording_out;
  d.cx = cx_host; d.c0 = c0_host; d.c1 = c1_host;
  return eegldm_sample_run(&d);
}
