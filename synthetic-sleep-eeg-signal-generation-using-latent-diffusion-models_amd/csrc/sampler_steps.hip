// The sampler's device code: the scheduler steps (add_noise, DDIM, DDIM with eta, ancestral DDPM, classifier-free guidance), the linear
// multistep / edit step, the start and window kernels of an edit, and the canvas kernels of long recordings, with their C ABI wrappers.
// HBM-bound, one pass over the data each.  sampler.hip sequences them behind the UNet forwards.
#include "elementwise.h"
#include "internal.h"

namespace {
// ------------------------------------------------------------------ the arithmetic every step shares
// x0 -- and e, the noise the model implies -- from the model output o and the sample s by the prediction type (sa = sqrt(a_t),
// sb = sqrt(1 - a_t)), x0 optionally clamped; e is taken from the unclamped x0.  Plain expressions: the compiler contracts them as it sees
// fit, the same way in every kernel that inlines them.
__device__ __forceinline__ float step_x0_e(float o, float s, float sa, float sb, int pred, int clip, float& e) {
  float x0;
  if (pred == EEGLDM_PRED_EPSILON) { x0 = (s - sb * o) / sa; e = o; }
  else if (pred == EEGLDM_PRED_V) { x0 = sa * s - sb * o; e = sa * o + sb * s; }
  else { x0 = o; e = (s - sa * x0) / sb; }
  if (clip) x0 = clamp_keep_nan(x0, -1.0f, 1.0f);
  return x0;
}
// x0 alone: e is dead code
__device__ __forceinline__ float step_x0(float o, float s, float sa, float sb, int pred, int clip) {
  float e;
  return step_x0_e(o, s, sa, sb, pred, clip, e);
}
// classifier-free guidance on the raw model output: oc the conditional, ou the null-class output
__device__ __forceinline__ float guided_out(float oc, float ou, float w) { return ou + w * (oc - ou); }

// ------------------------------------------------------------------ schedulers (training.py:429-436, sample_trials.py:163)
__global__ void add_noise_kernel(const float* __restrict__ x, const float* __restrict__ nz, const int64_t* __restrict__ t,
                                 const float* __restrict__ acp, float* __restrict__ out, long n, long per, int velocity) {
  GRID_STRIDE(i, n) {
    const float a = acp[t[i / per]];
    const float sa = sqrtf(a), sb = sqrtf(1.0f - a);
    out[i] = velocity ? (sa * nz[i] - sb * x[i]) : add_noise_value(x[i], nz[i], sa, sb);
  }
}
__global__ void ddim_step_kernel(const float* __restrict__ mo, const float* __restrict__ x, float a_t, float a_prev, int pred,
                                 int clip, float* __restrict__ prev, float* __restrict__ x0o, long n) {
  const float sa = sqrtf(a_t), sb = sqrtf(1.0f - a_t), sap = sqrtf(a_prev), sbp = sqrtf(1.0f - a_prev);
  GRID_STRIDE(i, n) {
    const float o = mo[i], s = x[i];
    float e;
    const float x0 = step_x0_e(o, s, sa, sb, pred, clip, e);
    prev[i] = sap * x0 + sbp * e;
    if (x0o) x0o[i] = x0;
  }
}

// DDIMScheduler.step with eta > 0 (Song et al. eq. 12 / 16): sigma = eta sqrt((1 - a_prev) / (1 - a_t) (1 - a_t / a_prev)),
// prev = sqrt(a_prev) x0 + sqrt(1 - a_prev - sigma^2) e + sigma noise; eta = 0 is ddim_step_kernel
__global__ void ddim_step_eta_kernel(const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ nz, float a_t, float a_prev,
                                     float sigma, float dir, int pred, int clip, float* __restrict__ prev, float* __restrict__ x0o, long n) {
  const float sa = sqrtf(a_t), sb = sqrtf(1.0f - a_t), sap = sqrtf(a_prev);
  GRID_STRIDE(i, n) {
    const float o = mo[i], s = x[i];
    float e;
    const float x0 = step_x0_e(o, s, sa, sb, pred, clip, e);
    prev[i] = fmaf(sigma, nz[i], fmaf(sap, x0, dir * e));
    if (x0o) x0o[i] = x0;
  }
}

// DDPM ancestral step (DDPMScheduler.step, variance_type fixed_small: the 1000-step logging sampler of util.py:241-243,261-285 and
// sample_trials_ddpm.py:99-102; same arithmetic as DDPM.p_sample, /root/reference/src/models/ldm.py:311-357):
//   x0 from the prediction type, optional clamp, mean = c0 * x0 + ct * x_t, plus sigma * noise when t > 0 (sigma = 0 at t = 0)
__global__ void ddpm_step_kernel(const float* __restrict__ mo, const float* __restrict__ x, const float* __restrict__ nz, float sa, float sb,
                                 float c0, float ct, float sigma, int pred, int clip, float* __restrict__ prev, float* __restrict__ x0o, long n) {
  GRID_STRIDE(i, n) {
    const float o = mo[i], s = x[i];
    const float x0 = step_x0(o, s, sa, sb, pred, clip);
    float m = c0 * x0 + ct * s;
    if (sigma != 0.0f) m += sigma * nz[i];
    prev[i] = m;
    if (x0o) x0o[i] = x0;
  }
}

// Classifier-free guidance fused into the scheduler step: mo holds the conditional outputs [0, n) and the null-class outputs [n, 2n);
// o = o_u + w (o_c - o_u) in fp32 on the raw model output (whatever the prediction type), then the DDIM (eta 0) or the ancestral DDPM
// step of the kernels above.  prev2 (optional) receives a second copy of prev: the null-class half of the sampler's 2B-row latent buffer.
__global__ void cfg_step_kernel(const float* __restrict__ mo, float w, const float* __restrict__ x, const float* __restrict__ nz, int ancestral,
                                float sa, float sb, float c0, float ct, float sigma, int pred, int clip, float* __restrict__ prev,
                                float* __restrict__ prev2, long n) {
  GRID_STRIDE(i, n) {
    const float ou = mo[n + i];
    const float o = guided_out(mo[i], ou, w), s = x[i];
    float e;
    const float x0 = step_x0_e(o, s, sa, sb, pred, clip, e);
    float m;
    if (ancestral) { m = c0 * x0 + ct * s; if (sigma != 0.0f) m += sigma * nz[i]; }
    else m = c0 * x0 + ct * e;                      // DDIM: c0 = sqrt(a_prev), ct = sqrt(1 - a_prev)
    prev[i] = m;
    if (prev2) prev2[i] = m;
  }
}

// ------------------------------------------------------------------ linear multistep sampler step (DPM-Solver++ 2M; include/eegldm.h)
// prev = cx * sample + c0 * x0 + c1 * hist, hist <- x0, with x0 = step_x0 of the (guided) model output.  The three coefficients come from
// the host (schedulers.py multistep_coefficients), so the device side is solver-agnostic.  The update is ONE function, contraction off and
// the fused multiply-adds spelled out (as adam_elem / ema_elem), so the float4 body, the scalar edges and every caller round alike.
__device__ __forceinline__ float multistep_update(float s, float x0, float h, float cx, float c0, float c1) {
#pragma clang fp contract(off)
  const float m = c1 != 0.0f ? fmaf(c0, x0, c1 * h) : c0 * x0;      // c1 == 0 (first-order step): the history is not read
  return fmaf(cx, s, m);
}
// ------------------------------------------------------------------ editing: sampling from an input, with a keep-mask (include/eegldm.h)
// k = the known clean signal z0 noised to the level a (ka = sqrt(a), kb = sqrt(1 - a)) with the caller's noise; kb == 0 (a == 1) is z0
// itself.  ONE function for the start kernel and for the blend inside the step, contraction off, so that both round alike.
__device__ __forceinline__ float edit_renoise(float z0, float nz, float ka, float kb) {
#pragma clang fp contract(off)
  return kb != 0.0f ? fmaf(ka, z0, kb * nz) : ka * z0;
}
// m k + (1 - m) p.  m == 0 is p and m == 1 is k, bit for bit, whatever the other operand holds.
__device__ __forceinline__ float edit_blend(float m, float k, float p) {
#pragma clang fp contract(off)
  if (m == 0.0f) return p;
  if (m == 1.0f) return k;
  return fmaf(m, k, (1.0f - m) * p);
}
// One element of the flat step: the DDIM (eta 0) form (!MULTISTEP: p0 = sqrt(a_prev), p1 = sqrt(1 - a_prev); the expression of
// ddim_step_kernel / cfg_step_kernel with the compiler's own contraction, hence their bytes) or the multistep form (p0, p1, p2 = cx, c0, c1;
// h = the history value, 0 when it is not read).  -> prev; x0 = the model's own data prediction.
template <bool MULTISTEP>
__device__ __forceinline__ float flat_step_elem(float o, float s, float h, float sa, float sb, int pred, int clip, float p0, float p1, float p2,
                                                float& x0) {
  if (MULTISTEP) {
    x0 = step_x0(o, s, sa, sb, pred, clip);
    return multistep_update(s, x0, h, p0, p1, p2);
  }
  float e;
  x0 = step_x0_e(o, s, sa, sb, pred, clip, e);
  return p0 * x0 + p1 * e;
}
// One sampling step, one launch, whatever the solver: the DDIM or the multistep form, each plain or guided (mo: n values, or 2n when guided
// -- conditional outputs, then null-class outputs), then, with BLEND, prev = blend(mask, renoise(known, noise), prev).  !BLEND
// (eegldm_multistep_step always; eegldm_edit_step without a mask): known / noise / mask are not read.  The form is chosen at compile time --
// the step is launch-bound at batch 1, where the run-time flags measured outside the parent's spread (profiles/sampler_steps_refactor.txt);
// the vector body and the edge loop are written once.  The history and pred_x0 receive the model's own x0.  prev may alias x (every element
// is read before it is written, by the same thread); hist is NULL only when it is not read; prev2 / x0o are optional.
template <bool MULTISTEP, bool BLEND>
__global__ __launch_bounds__(NT) void edit_step_kernel(const float* __restrict__ mo, float w, int guided, const float* x, float* hist, float sa,
                                                       float sb, int pred, int clip, float p0, float p1, float p2,
                                                       const float* __restrict__ known, const float* __restrict__ noise,
                                                       const float* __restrict__ mask, float ka, float kb, float* prev, float* prev2,
                                                       float* x0o, long n, long head) {
  const VecSplit s = vec_split(n, head);
  const f32x4* oc4 = (const f32x4*)(mo + head); const f32x4* ou4 = (const f32x4*)(mo + n + head); const f32x4* x4 = (const f32x4*)(x + head);
  const f32x4* k4 = (const f32x4*)(known + head); const f32x4* n4 = (const f32x4*)(noise + head); const f32x4* m4 = (const f32x4*)(mask + head);
  f32x4* h4 = (f32x4*)(hist + head); f32x4* q1 = (f32x4*)(prev + head); f32x4* q2 = (f32x4*)(prev2 + head); f32x4* z4 = (f32x4*)(x0o + head);
  const bool two = MULTISTEP && p2 != 0.0f;
  GRID_STRIDE(i, s.n4) {
    f32x4 ov = oc4[i];
    if (guided) {
      const f32x4 uv = ou4[i];
#pragma unroll
      for (int k = 0; k < 4; k++) ov[k] = guided_out(ov[k], uv[k], w);
    }
    const f32x4 xv = x4[i];
    f32x4 hv = {0.0f, 0.0f, 0.0f, 0.0f}, pv, zv;
    if (two) hv = h4[i];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float z;
      pv[k] = flat_step_elem<MULTISTEP>(ov[k], xv[k], hv[k], sa, sb, pred, clip, p0, p1, p2, z);
      zv[k] = z;
    }
    if (BLEND) {
      const f32x4 kv = k4[i], nv = n4[i], mv = m4[i];
#pragma unroll
      for (int k = 0; k < 4; k++) pv[k] = edit_blend(mv[k], edit_renoise(kv[k], nv[k], ka, kb), pv[k]);
    }
    q1[i] = pv;
    if (prev2) q2[i] = pv;
    if (hist) h4[i] = zv;
    if (x0o) z4[i] = zv;
  }
  GRID_STRIDE(j, s.nedge) {
    const long i = EDGE_INDEX(s, j);
    float o = mo[i];
    if (guided) o = guided_out(o, mo[n + i], w);
    const float xs = x[i];
    float x0;
    float m = flat_step_elem<MULTISTEP>(o, xs, two ? hist[i] : 0.0f, sa, sb, pred, clip, p0, p1, p2, x0);
    if (BLEND) m = edit_blend(mask[i], edit_renoise(known[i], noise[i], ka, kb), m);
    prev[i] = m;
    if (prev2) prev2[i] = m;
    if (hist) hist[i] = x0;
    if (x0o) x0o[i] = x0;
  }
}
// The start of an edit run: z0 = sf * z_mu (sf == 1: z_mu itself) and x = renoise(z0, noise) at the first executed step's noise level;
// either output may be left out.
__global__ __launch_bounds__(NT) void edit_start_kernel(const float* __restrict__ zmu, float sf, const float* __restrict__ noise, float ka, float kb,
                                                        float* __restrict__ z0o, float* __restrict__ xo, long n, long head) {
  const VecSplit s = vec_split(n, head);
  const f32x4* z4 = (const f32x4*)(zmu + head); const f32x4* n4 = (const f32x4*)(noise + head);
  f32x4* o4 = (f32x4*)(z0o + head); f32x4* x4 = (f32x4*)(xo + head);
  GRID_STRIDE(i, s.n4) {
    f32x4 zv = z4[i];
#pragma unroll
    for (int k = 0; k < 4; k++) zv[k] = sf * zv[k];
    if (z0o) o4[i] = zv;
    if (xo) {
      const f32x4 nv = n4[i];
      f32x4 xv;
#pragma unroll
      for (int k = 0; k < 4; k++) xv[k] = edit_renoise(zv[k], nv[k], ka, kb);
      x4[i] = xv;
    }
  }
  GRID_STRIDE(j, s.nedge) {
    const long i = EDGE_INDEX(s, j);
    const float z = sf * zmu[i];
    if (z0o) z0o[i] = z;
    if (xo) xo[i] = edit_renoise(z, noise[i], ka, kb);
  }
}
// ------------------------------------------------------------------ resampled repair: the jump back up the noise schedule (include/eegldm.h)
// p = jx x + jn eps -- contraction off and the fma spelled out, as multistep_update -- then, with BLEND, the blend of the step towards the
// known signal noised to the level the jump lands on, so the kept positions hold k(a_level) bit for bit after a jump as after a step.
__device__ __forceinline__ float jump_update(float x, float eps, float jx, float jn) {
#pragma clang fp contract(off)
  return fmaf(jx, x, jn * eps);
}
// word e & 3 of the quad of counter e >> 2: the value eegldm_randn writes to out[e]
__device__ __forceinline__ float jump_draw1(unsigned long long seed, unsigned long long offset, long e) {
  float z[4]; philox_normal4(seed, offset + (unsigned long long)(e >> 2), z);
  const int k = (int)(e & 3);
  return k == 0 ? z[0] : (k == 1 ? z[1] : (k == 2 ? z[2] : z[3]));
}
// DRAW: eps[e] is drawn in registers -- a function of (seed, offset, e) alone, whatever the pointers' alignment, the body / edge split and
// the grid; else eps = fresh.  A float4 of the body starts at element head + 4 i: with head & 3 == 0 it is one quad, otherwise the thread
// evaluates the two quads its four elements straddle and takes words sh .. sh + 3 of the eight (sh is uniform: the selects are static).
// out may be x itself (every element is read before it is written, by the same thread); out2 is optional.
template <bool DRAW, bool BLEND>
__global__ __launch_bounds__(NT) void edit_jump_kernel(const float* x, float jx, float jn, const float* __restrict__ fresh, unsigned long long seed,
                                                       unsigned long long offset, const float* __restrict__ known, const float* __restrict__ noise,
                                                       const float* __restrict__ mask, float ka, float kb, float* out, float* out2, long n,
                                                       long head) {
  const VecSplit s = vec_split(n, head);
  const f32x4* x4 = (const f32x4*)(x + head); const f32x4* f4 = (const f32x4*)(fresh + head);
  const f32x4* k4 = (const f32x4*)(known + head); const f32x4* n4 = (const f32x4*)(noise + head); const f32x4* m4 = (const f32x4*)(mask + head);
  f32x4* q1 = (f32x4*)(out + head); f32x4* q2 = (f32x4*)(out2 + head);
  const int sh = (int)(head & 3);
  const unsigned long long quad0 = offset + (unsigned long long)(head >> 2);
  GRID_STRIDE(i, s.n4) {
    const f32x4 xv = x4[i];
    f32x4 ev, pv;
    if (DRAW) {
      float za[4], zb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      philox_normal4(seed, quad0 + (unsigned long long)i, za);
      if (sh != 0) philox_normal4(seed, quad0 + (unsigned long long)i + 1ull, zb);
      if (sh == 0) { ev[0] = za[0]; ev[1] = za[1]; ev[2] = za[2]; ev[3] = za[3]; }
      else if (sh == 1) { ev[0] = za[1]; ev[1] = za[2]; ev[2] = za[3]; ev[3] = zb[0]; }
      else if (sh == 2) { ev[0] = za[2]; ev[1] = za[3]; ev[2] = zb[0]; ev[3] = zb[1]; }
      else { ev[0] = za[3]; ev[1] = zb[0]; ev[2] = zb[1]; ev[3] = zb[2]; }
    } else ev = f4[i];
#pragma unroll
    for (int k = 0; k < 4; k++) pv[k] = jump_update(xv[k], ev[k], jx, jn);
    if (BLEND) {
      const f32x4 kv = k4[i], nv = n4[i], mv = m4[i];
#pragma unroll
      for (int k = 0; k < 4; k++) pv[k] = edit_blend(mv[k], edit_renoise(kv[k], nv[k], ka, kb), pv[k]);
    }
    q1[i] = pv;
    if (out2) q2[i] = pv;
  }
  GRID_STRIDE(j, s.nedge) {
    const long i = EDGE_INDEX(s, j);
    float p = jump_update(x[i], DRAW ? jump_draw1(seed, offset, i) : fresh[i], jx, jn);
    if (BLEND) p = edit_blend(mask[i], edit_renoise(known[i], noise[i], ka, kb), p);
    out[i] = p;
    if (out2) out2[i] = p;
  }
}
// Window side of an edit: (1) the keep-mask at the sampler's resolution, mask_lat[b][c][l] = min over the `down` window samples latent
// position l covers (every one of the C channels receives the same row); (2) the composite out = blend(mask_win, input, decoded) over
// Co channels.  Either half may be left out (mask_lat / out NULL).  One-off work of a sampling call: scalar accesses, any alignment.
__global__ __launch_bounds__(NT) void edit_window_kernel(const float* __restrict__ mask_win, long n_lat, long n_win, int Lw, int down, int C,
                                                         float* __restrict__ mask_lat, const float* __restrict__ input, const float* decoded,
                                                         int Co, float* out) {
  const int Ll = Lw / down;
  GRID_STRIDE(i, n_lat) {
    const long b = i / ((long)C * Ll); const int l = (int)(i % Ll);
    const float* row = mask_win + b * Lw + (long)l * down;
    float m = row[0];
    for (int d = 1; d < down; d++) m = fminf(m, row[d]);
    mask_lat[i] = m;
  }
  GRID_STRIDE(i, n_win) {
    const long b = i / ((long)Co * Lw); const int t = (int)(i % Lw);
    out[i] = edit_blend(mask_win[b * Lw + t], input[i], decoded[i]);
  }
}
// ------------------------------------------------------------------ long recordings: overlapped windows on one canvas (include/eegldm.h)
// Window k of a recording covers canvas positions [k S, k S + L), S = L - (2 m + r).  Position p belongs to the LAST window k1 whose
// zero-weight margin it has left (k1 S + m <= p; k1 = 0 below S + m); jp = p - k1 S.  Inside the ramp (k1 >= 1, jp < m + r) window k1 has
// weight u = (jp - m + 0.5) / r and window k1 - 1 has 1 - u; everywhere else window k1 has weight 1 and no other window is read.
struct CanvasGeo { int C, W, L, S, m, r, Lc; };
struct CanvasAt { int k1, jp; bool ramp; };
__device__ __forceinline__ CanvasAt canvas_at(const CanvasGeo& g, int p) {
  CanvasAt a;
  a.k1 = p < g.S + g.m ? 0 : min(g.W - 1, (p - g.m) / g.S);
  a.jp = p - a.k1 * g.S;
  a.ramp = a.k1 >= 1 && a.jp < g.m + g.r;
  return a;
}
__device__ __forceinline__ float canvas_u(const CanvasGeo& g, int jp) { return ((float)(jp - g.m) + 0.5f) / (float)g.r; }
// the windows that cover p, weight-0 ones included
__device__ __forceinline__ int canvas_kmin(const CanvasGeo& g, int p) { return p < g.L ? 0 : (p - g.L) / g.S + 1; }
__device__ __forceinline__ int canvas_kmax(const CanvasGeo& g, int p) { return min(g.W - 1, p / g.S); }
// (1 - u) a + u b with the exactness of edit_blend at both ends
__device__ __forceinline__ float canvas_fuse(float u, float a, float b) {
#pragma clang fp contract(off)
  if (u == 0.0f) return a;
  if (u == 1.0f) return b;
  return fmaf(u, b, (1.0f - u) * a);
}
// N = 4: one 16-byte access when the address allows it, else four 4-byte ones; N = 1: one element
template <int N> __device__ __forceinline__ void canvas_ld(const float* p, float (&v)[4]) {
  if (N == 4 && ((uintptr_t)p & 15) == 0) {
    const f32x4 t = *(const f32x4*)p;
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = t[k];
  } else {
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = p[k];
  }
}
template <int N> __device__ __forceinline__ void canvas_st(float* p, const float (&v)[4]) {
  if (N == 4 && ((uintptr_t)p & 15) == 0) {
    f32x4 t;
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = v[k];
    *(f32x4*)p = t;
  } else {
#pragma unroll
    for (int k = 0; k < N; k++) p[k] = v[k];
  }
}
// four consecutive flat indices from i form ONE span when they lie in one row of length `len` (*row, *p: the row and position of i)
__device__ __forceinline__ bool canvas_one_row(long i, int len, long* row, int* p) {
  *row = i / len; *p = (int)(i - *row * len);
  return *p + 3 < len;
}
struct CanvasStepArgs {
  const float* mo; float w; int guided; const float* canvas; float* hist; float sa, sb; int pred, clip; float cx, c0, c1;
  float *out, *win, *win2, *x0o; long n_win;
};
// the blend of eegldm_canvas_edit_step: three canvas-shaped inputs and the noise level the step lands on (ka = sqrt(a_next), kb = sqrt(1 - a_next))
struct CanvasEditArgs { const float *known, *noise, *mask; float ka, kb; };
// N canvas elements from position p of row `row` (= rec * C + c): all in one row, one owner window, one ramp state, one set of covering windows.
// EDIT (canvas_edit_step_kernel only; e is not read otherwise): prev <- edit_blend(mask, edit_renoise(known, noise), prev) ahead of the stores
// of prev; hist / pred_x0 keep the model's own fused x0.
template <int N, bool EDIT>
__device__ __forceinline__ void canvas_step_span(const CanvasGeo& g, const CanvasStepArgs& a, const CanvasEditArgs& e, long row, int p,
                                                 const CanvasAt& at) {
  const long ci = row * g.Lc + p;
  const long rec = row / g.C; const int c = (int)(row - rec * g.C);
  float xc[4], o[4], z[4], h[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pv[4];
  canvas_ld<N>(a.canvas + ci, xc);
  const long wb = ((rec * g.W + at.k1) * g.C + c) * g.L + at.jp;       // the owner window's element, in model_out and in win
  canvas_ld<N>(a.mo + wb, o);
  if (a.guided) {
    float ou[4];
    canvas_ld<N>(a.mo + a.n_win + wb, ou);
#pragma unroll
    for (int k = 0; k < N; k++) o[k] = guided_out(o[k], ou[k], a.w);
  }
#pragma unroll
  for (int k = 0; k < N; k++) z[k] = step_x0(o[k], xc[k], a.sa, a.sb, a.pred, a.clip);
  if (at.ramp) {
    const long wa = wb - (long)g.C * g.L + g.S;                         // the same canvas position in window k1 - 1
    float oa[4];
    canvas_ld<N>(a.mo + wa, oa);
    if (a.guided) {
      float ou[4];
      canvas_ld<N>(a.mo + a.n_win + wa, ou);
#pragma unroll
      for (int k = 0; k < N; k++) oa[k] = guided_out(oa[k], ou[k], a.w);
    }
#pragma unroll
    for (int k = 0; k < N; k++) z[k] = canvas_fuse(canvas_u(g, at.jp + k), step_x0(oa[k], xc[k], a.sa, a.sb, a.pred, a.clip), z[k]);
  }
  if (a.c1 != 0.0f) canvas_ld<N>(a.hist + ci, h);
#pragma unroll
  for (int k = 0; k < N; k++) pv[k] = multistep_update(xc[k], z[k], h[k], a.cx, a.c0, a.c1);
  if (EDIT) {
    float kn[4], nz[4], mk[4];
    canvas_ld<N>(e.known + ci, kn);
    canvas_ld<N>(e.noise + ci, nz);
    canvas_ld<N>(e.mask + ci, mk);
#pragma unroll
    for (int k = 0; k < N; k++) pv[k] = edit_blend(mk[k], edit_renoise(kn[k], nz[k], e.ka, e.kb), pv[k]);
  }
  canvas_st<N>(a.out + ci, pv);
  if (a.hist) canvas_st<N>(a.hist + ci, z);
  if (a.x0o) canvas_st<N>(a.x0o + ci, z);
  if (a.win) {
    const int k1 = canvas_kmax(g, p);
    for (int k = canvas_kmin(g, p); k <= k1; k++) {
      const long off = ((rec * g.W + k) * g.C + c) * g.L + (p - k * g.S);
      canvas_st<N>(a.win + off, pv);
      if (a.win2) canvas_st<N>(a.win2 + off, pv);
    }
  }
}
// One sampling step on the canvas, one launch: n = R C Lc canvas elements, four per thread from `head` on (the canvas's own 16-byte
// grid; every other buffer takes 16-byte accesses where its address allows).  A group of four that crosses a row end, a window's margin
// or ramp edge, or the edge of a covering window goes element by element in the same thread; every output element has one writer.
template <bool EDIT>
__device__ __forceinline__ void canvas_step_body(const CanvasGeo& g, const CanvasStepArgs& a, const CanvasEditArgs& e, long n, long head) {
  const VecSplit s = vec_split(n, head);
  GRID_STRIDE(q, s.n4) {
    const long i = head + (q << 2);
    long row; int p;
    bool one = canvas_one_row(i, g.Lc, &row, &p);
    CanvasAt at = canvas_at(g, p);
    if (one) {
      const CanvasAt e3 = canvas_at(g, p + 3);
      one = e3.k1 == at.k1 && e3.ramp == at.ramp && canvas_kmin(g, p) == canvas_kmin(g, p + 3) && canvas_kmax(g, p) == canvas_kmax(g, p + 3);
    }
    if (one) { canvas_step_span<4, EDIT>(g, a, e, row, p, at); continue; }
    for (int k = 0; k < 4; k++) {
      (void)canvas_one_row(i + k, g.Lc, &row, &p);
      canvas_step_span<1, EDIT>(g, a, e, row, p, canvas_at(g, p));
    }
  }
  GRID_STRIDE(j, s.nedge) {
    long row; int p;
    (void)canvas_one_row(EDGE_INDEX(s, j), g.Lc, &row, &p);
    canvas_step_span<1, EDIT>(g, a, e, row, p, canvas_at(g, p));
  }
}
__global__ __launch_bounds__(NT) void canvas_step_kernel(CanvasGeo g, CanvasStepArgs a, long n, long head) {
  canvas_step_body<false>(g, a, CanvasEditArgs{}, n, head);
}
// The same step plus the blend towards the known signal noised to the level the step lands on (eegldm_canvas_edit_step with a mask): the
// grouping is unchanged -- known / noise / mask are canvas-shaped, so a span of the canvas is a span of theirs.
__global__ __launch_bounds__(NT) void canvas_edit_step_kernel(CanvasGeo g, CanvasStepArgs a, CanvasEditArgs e, long n, long head) {
  canvas_step_body<true>(g, a, e, n, head);
}
// win[rec * W + k][c][l] = canvas[rec][c][k S + l] (and the same into win2): n = R W C L window elements on win's 16-byte grid
template <int N>
__device__ __forceinline__ void canvas_gather_span(const CanvasGeo& g, const float* canvas, float* win, float* win2, long wrow, int l) {
  const long rk = wrow / g.C; const int c = (int)(wrow - rk * g.C);
  const long rec = rk / g.W; const int k = (int)(rk - rec * g.W);
  float v[4];
  canvas_ld<N>(canvas + (rec * g.C + c) * g.Lc + (long)k * g.S + l, v);
  canvas_st<N>(win + wrow * g.L + l, v);
  if (win2) canvas_st<N>(win2 + wrow * g.L + l, v);
}
__global__ __launch_bounds__(NT) void canvas_gather_kernel(CanvasGeo g, const float* __restrict__ canvas, float* __restrict__ win,
                                                           float* __restrict__ win2, long n, long head) {
  const VecSplit s = vec_split(n, head);
  GRID_STRIDE(q, s.n4) {
    const long i = head + (q << 2);
    long wrow; int l;
    if (canvas_one_row(i, g.L, &wrow, &l)) { canvas_gather_span<4>(g, canvas, win, win2, wrow, l); continue; }
    for (int k = 0; k < 4; k++) {
      (void)canvas_one_row(i + k, g.L, &wrow, &l);
      canvas_gather_span<1>(g, canvas, win, win2, wrow, l);
    }
  }
  GRID_STRIDE(j, s.nedge) {
    long wrow; int l;
    (void)canvas_one_row(EDGE_INDEX(s, j), g.L, &wrow, &l);
    canvas_gather_span<1>(g, canvas, win, win2, wrow, l);
  }
}
// out[rec][c][p] = the owner window's decoded sample, cross-faded with its predecessor's inside the ramp (g at window resolution)
template <int N>
__device__ __forceinline__ void canvas_compose_span(const CanvasGeo& g, const float* dec, float* out, long row, int p, const CanvasAt& at) {
  const long rec = row / g.C; const int c = (int)(row - rec * g.C);
  const long wb = ((rec * g.W + at.k1) * g.C + c) * g.L + at.jp;
  float v[4];
  canvas_ld<N>(dec + wb, v);
  if (at.ramp) {
    float va[4];
    canvas_ld<N>(dec + wb - (long)g.C * g.L + g.S, va);
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = canvas_fuse(canvas_u(g, at.jp + k), va[k], v[k]);
  }
  canvas_st<N>(out + row * g.Lc + p, v);
}
__global__ __launch_bounds__(NT) void canvas_compose_kernel(CanvasGeo g, const float* __restrict__ dec, float* __restrict__ out, long n, long head) {
  const VecSplit s = vec_split(n, head);
  GRID_STRIDE(q, s.n4) {
    const long i = head + (q << 2);
    long row; int p;
    bool one = canvas_one_row(i, g.Lc, &row, &p);
    CanvasAt at = canvas_at(g, p);
    if (one) { const CanvasAt e = canvas_at(g, p + 3); one = e.k1 == at.k1 && e.ramp == at.ramp; }
    if (one) { canvas_compose_span<4>(g, dec, out, row, p, at); continue; }
    for (int k = 0; k < 4; k++) {
      (void)canvas_one_row(i + k, g.Lc, &row, &p);
      canvas_compose_span<1>(g, dec, out, row, p, canvas_at(g, p));
    }
  }
  GRID_STRIDE(j, s.nedge) {
    long row; int p;
    (void)canvas_one_row(EDGE_INDEX(s, j), g.Lc, &row, &p);
    canvas_compose_span<1>(g, dec, out, row, p, canvas_at(g, p));
  }
}
}  // namespace

// ================================================================== C ABI
extern "C" int eegldm_add_noise(eegldm_ctx* ctx, const float* x, const float* nz, const int64_t* t, const float* acp, float* out, int B, long per) {
  hipLaunchKernelGGL(add_noise_kernel, dim3(grid1d((long)B * per, ctx)), dim3(NT), 0, ctx->stream, x, nz, t, acp, out, (long)B * per, per, 0);
  LAUNCH_CHECK(); return 0;
}
extern "C" int eegldm_get_velocity(eegldm_ctx* ctx, const float* x, const float* nz, const int64_t* t, const float* acp, float* out, int B, long per) {
  hipLaunchKernelGGL(add_noise_kernel, dim3(grid1d((long)B * per, ctx)), dim3(NT), 0, ctx->stream, x, nz, t, acp, out, (long)B * per, per, 1);
  LAUNCH_CHECK(); return 0;
}
extern "C" int eegldm_ddim_step(eegldm_ctx* ctx, const float* mo, const float* x, float a_t, float a_prev, int pred, int clip,
                                float* prev, float* x0, long n) {
  EEG_CHECK(pred >= 0 && pred <= 2, "prediction type %d", pred);
  hipLaunchKernelGGL(ddim_step_kernel, dim3(grid1d(n, ctx)), dim3(NT), 0, ctx->stream, mo, x, a_t, a_prev, pred, clip, prev, x0, n);
  LAUNCH_CHECK(); return 0;
}
extern "C" int eegldm_ddim_step_eta(eegldm_ctx* ctx, const float* mo, const float* x, const float* noise, float a_t, float a_prev, float eta,
                                    int pred, int clip, float* prev, float* x0, long n) {
  EEG_CHECK(ctx && mo && x && prev, "null argument");
  EEG_CHECK(pred >= 0 && pred <= 2, "prediction type %d", pred);
  EEG_CHECK(eta >= 0.0f && a_t > 0.0f && a_t < 1.0f && a_prev > 0.0f && a_prev <= 1.0f, "bad eta / schedule values");
  if (eta == 0.0f) return eegldm_ddim_step(ctx, mo, x, a_t, a_prev, pred, clip, prev, x0, n);
  EEG_CHECK(noise, "eta > 0 needs a noise tensor");
  // sigma_t(eta) and the direction coefficient in double on the host, like the schedulers' tables
  const double var = (1.0 - (double)a_prev) / (1.0 - (double)a_t) * (1.0 - (double)a_t / (double)a_prev);
  const double sigma = (double)eta * sqrt(var > 0.0 ? var : 0.0);
  const double d2 = 1.0 - (double)a_prev - sigma * sigma;
  hipLaunchKernelGGL(ddim_step_eta_kernel, dim3(grid1d(n, ctx)), dim3(NT), 0, ctx->stream, mo, x, noise, a_t, a_prev, (float)sigma,
                     (float)sqrt(d2 > 0.0 ? d2 : 0.0), pred, clip, prev, x0, n);
  LAUNCH_CHECK(); return 0;
}
extern "C" int eegldm_ddpm_step(eegldm_ctx* ctx, const float* mo, const float* x, const float* noise, float a_t, float a_prev, float beta_t,
                                int pred, int clip, float* prev, float* x0, long n) {
  return eegldm_ddpm_step_var(ctx, mo, x, noise, a_t, a_prev, beta_t, 0, pred, clip, prev, x0, n);
}
// variance_large != 0: DDPMScheduler(variance_type="fixed_large"): sigma^2 = beta_t instead of the posterior variance
extern "C" int eegldm_ddpm_step_var(eegldm_ctx* ctx, const float* mo, const float* x, const float* noise, float a_t, float a_prev, float beta_t,
                                    int variance_large, int pred, int clip, float* prev, float* x0, long n) {
  EEG_CHECK(ctx && mo && x && prev, "null argument");
  EEG_CHECK(pred >= 0 && pred <= 2, "prediction type %d", pred);
  EEG_CHECK(a_t > 0.0f && a_t < 1.0f && a_prev > 0.0f && a_prev <= 1.0f && beta_t > 0.0f && beta_t < 1.0f, "bad schedule values");
  // posterior q(x_{t-1} | x_t, x_0): coefficients in double on the host, as the schedulers build their tables
  const double bt = 1.0 - (double)a_t, bp = 1.0 - (double)a_prev;
  const double c0 = sqrt((double)a_prev) * (double)beta_t / bt, ct = sqrt(1.0 - (double)beta_t) * bp / bt;
  double var = variance_large ? (double)beta_t : bp / bt * (double)beta_t;
  const bool last = a_prev >= 1.0f;                  // t == 0: no noise
  if (var < 1e-20) var = 1e-20;
  const float sigma = last ? 0.0f : (float)sqrt(var);
  EEG_CHECK(last || noise, "noise is required for t > 0");
  hipLaunchKernelGGL(ddpm_step_kernel, dim3(grid1d(n, ctx)), dim3(NT), 0, ctx->stream, mo, x, noise, (float)sqrt((double)a_t), (float)sqrt(bt),
                     (float)c0, (float)ct, sigma, pred, clip, prev, x0, n);
  LAUNCH_CHECK(); return 0;
}
extern "C" int eegldm_guided_step(eegldm_ctx* ctx, const float* mo, float w, const float* x, const float* noise, float a_t, float a_prev,
                                  float beta_t, int ancestral, int pred, int clip, float* prev, float* prev2, long n) {
  EEG_CHECK(ctx && mo && x && prev, "null argument");
  EEG_CHECK(pred >= 0 && pred <= 2, "prediction type %d", pred);
  EEG_CHECK(a_t > 0.0f && a_t < 1.0f && a_prev > 0.0f && a_prev <= 1.0f, "bad schedule values");
  // the coefficients exactly as eegldm_ddim_step / eegldm_ddpm_step derive them
  float c0, ct, sigma = 0.0f;
  if (ancestral) {
    EEG_CHECK(beta_t > 0.0f && beta_t < 1.0f, "bad beta_t");
    const double bt = 1.0 - (double)a_t, bp = 1.0 - (double)a_prev;
    c0 = (float)(sqrt((double)a_prev) * (double)beta_t / bt); ct = (float)(sqrt(1.0 - (double)beta_t) * bp / bt);
    double var = bp / bt * (double)beta_t;
    if (var < 1e-20) var = 1e-20;
    if (a_prev < 1.0f) { sigma = (float)sqrt(var); EEG_CHECK(noise, "noise is required for t > 0"); }
  } else {
    c0 = sqrtf(a_prev); ct = sqrtf(1.0f - a_prev);
  }
  const float sa = ancestral ? (float)sqrt((double)a_t) : sqrtf(a_t), sb = ancestral ? (float)sqrt(1.0 - (double)a_t) : sqrtf(1.0f - a_t);
  hipLaunchKernelGGL(cfg_step_kernel, dim3(grid1d(n, ctx)), dim3(NT), 0, ctx->stream, mo, w, x, noise, ancestral, sa, sb, c0, ct, sigma,
                     pred, clip, prev, prev2, n);
  LAUNCH_CHECK(); return 0;
}
// ranges [p, p + np) and [q, q + nq) share an element (a NULL buffer overlaps nothing)
static bool ov(const float* p, long np, const float* q, long nq) { return p && q && p < q + nq && q < p + np; }
// ---- the flat step (include/eegldm.h): one launch of edit_step_kernel<multistep form, blend> behind eegldm_multistep_step and eegldm_edit_step
// coef NULL: the DDIM form, a_next is its a_prev; else {cx, c0, c1} of the multistep form and a_next only sets the blend's noise level.
// mask NULL: no blend.  The float4 body needs every buffer in use -- the null-class half of model_out included -- at one offset inside a
// 16-byte line; otherwise the whole range goes one element at a time.
static int flat_step_launch(eegldm_ctx* ctx, const float* mo, float w, int guided, const float* x, float* hist, float a_t, float a_next,
                            int pred, int clip, const float* coef, const float* known, const float* noise, const float* mask, float* prev,
                            float* prev2, float* x0, long n) {
  EEG_CHECK(ctx && mo && x && prev, "null argument");
  EEG_CHECK(n >= 0, "negative n (%ld)", n);
  EEG_CHECK(pred >= 0 && pred <= 2, "prediction type %d", pred);
  EEG_CHECK(a_t > 0.0f && a_t < 1.0f, "a_t %g outside (0, 1)", (double)a_t);
  EEG_CHECK(a_next > 0.0f && a_next <= 1.0f, "a_next %g outside (0, 1]", (double)a_next);
  EEG_CHECK(!guided || w == w, "guidance_scale is NaN");
  EEG_CHECK(!mask || (known && noise), "a mask needs the known signal and the noise");
  const bool ms = coef != nullptr;
  float p0, p1, p2 = 0.0f;
  if (ms) {
    p0 = coef[0]; p1 = coef[1]; p2 = coef[2];
    EEG_CHECK(p0 == p0 && p1 == p1 && p2 == p2, "a coefficient is NaN");
    EEG_CHECK(hist || p2 == 0.0f, "c1 != 0 needs the history buffer");
  } else {
    p0 = sqrtf(a_next); p1 = sqrtf(1.0f - a_next);      // as eegldm_ddim_step / eegldm_guided_step derive them
  }
  const long nm = guided ? 2 * n : n;
  // (prev == sample is the one aliasing the kernel is written for)
  EEG_CHECK(!ov(mo, nm, prev, n) && !ov(mo, nm, prev2, n) && !ov(mo, nm, x0, n) && !ov(mo, nm, hist, n), "model_out aliases an output buffer");
  EEG_CHECK(!ov(hist, n, x, n) && !ov(hist, n, prev, n) && !ov(hist, n, prev2, n) && !ov(hist, n, x0, n), "the history buffer aliases another buffer");
  EEG_CHECK(!ov(prev2, n, prev, n) && !ov(prev2, n, x, n) && !ov(x0, n, prev, n) && !ov(x0, n, x, n) && !ov(x0, n, prev2, n),
            "prev2 / pred_x0 alias another buffer");
  EEG_CHECK(prev == x || !ov(prev, n, x, n), "prev may be sample itself, not a shifted view of it");
  if (mask)
    for (const float* q : {known, noise, mask})
      EEG_CHECK(!ov(q, n, prev, n) && !ov(q, n, prev2, n) && !ov(q, n, x0, n) && !ov(q, n, hist, n), "known / noise / mask alias an output buffer");
  for (const void* q : {(const void*)mo, (const void*)x, (const void*)hist, (const void*)prev, (const void*)prev2, (const void*)x0,
                        (const void*)known, (const void*)noise, (const void*)mask})
    EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
  if (n == 0) return 0;
  long head = vec_head(n, {mo, x, prev});
  for (const void* q : {(const void*)(guided ? mo + n : nullptr), (const void*)hist, (const void*)prev2, (const void*)x0,
                        (const void*)(mask ? known : nullptr), (const void*)(mask ? noise : nullptr), (const void*)mask})
    if (q && head < n && ((uintptr_t)q & 15) != ((uintptr_t)mo & 15)) head = n;
  auto kernel = ms ? (mask ? edit_step_kernel<true, true> : edit_step_kernel<true, false>)
                   : (mask ? edit_step_kernel<false, true> : edit_step_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(grid_vec(n, head, ctx)), dim3(NT), 0, ctx->stream, mo, w, guided ? 1 : 0, x, hist, sqrtf(a_t), sqrtf(1.0f - a_t),
                     pred, clip, p0, p1, p2, known, noise, mask, sqrtf(a_next), sqrtf(1.0f - a_next), prev, prev2, x0, n, head);
  LAUNCH_CHECK(); return 0;
}
// the multistep form without a blend (a_next is not used then: any value in (0, 1])
extern "C" int eegldm_multistep_step(eegldm_ctx* ctx, const float* mo, float w, int guided, const float* x, float* hist, float a_t, int pred,
                                     int clip, float cx, float c0, float c1, float* prev, float* prev2, float* x0, long n) {
  const float coef[3] = {cx, c0, c1};
  return flat_step_launch(ctx, mo, w, guided, x, hist, a_t, 1.0f, pred, clip, coef, nullptr, nullptr, nullptr, prev, prev2, x0, n);
}
// ---- editing (include/eegldm.h): the step with the blend, the start of a run, the window-side mask pooling and composite
extern "C" int eegldm_edit_step(eegldm_ctx* ctx, const float* mo, float w, int guided, const float* x, float* hist, float a_t, float a_next,
                                int pred, int clip, const float* coef_host, const float* known, const float* noise, const float* mask,
                                float* prev, float* prev2, float* x0, long n) {
  return flat_step_launch(ctx, mo, w, guided, x, hist, a_t, a_next, pred, clip, coef_host, known, noise, mask, prev, prev2, x0, n);
}
extern "C" int eegldm_edit_start(eegldm_ctx* ctx, const float* z_mu, float scale_factor, const float* noise, float a_start, float* z0,
                                 float* x_start, long n) {
  EEG_CHECK(ctx && z_mu && (z0 || x_start), "null argument");
  EEG_CHECK(n >= 0, "negative n (%ld)", n);
  EEG_CHECK(scale_factor == scale_factor, "scale_factor is NaN");
  EEG_CHECK(!x_start || noise, "the noised start needs the noise");
  EEG_CHECK(!x_start || (a_start > 0.0f && a_start <= 1.0f), "a_start %g outside (0, 1]", (double)a_start);
  EEG_CHECK(!ov(z0, n, z_mu, n) && !ov(z0, n, noise, n) && !ov(x_start, n, z_mu, n) && !ov(x_start, n, noise, n) && !ov(z0, n, x_start, n),
            "an output aliases another buffer");
  for (const void* q : {(const void*)z_mu, (const void*)noise, (const void*)z0, (const void*)x_start})
    EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
  if (n == 0) return 0;
  long head = vec_head(n, {z_mu});
  for (const void* q : {(const void*)(x_start ? noise : nullptr), (const void*)z0, (const void*)x_start})
    if (q && head < n && ((uintptr_t)q & 15) != ((uintptr_t)z_mu & 15)) head = n;
  const float a = x_start ? a_start : 1.0f;
  hipLaunchKernelGGL(edit_start_kernel, dim3(grid_vec(n, head, ctx)), dim3(NT), 0, ctx->stream, z_mu, scale_factor, noise, sqrtf(a), sqrtf(1.0f - a),
                     z0, x_start, n, head);
  LAUNCH_CHECK(); return 0;
}
// the jump of a resampled repair: one launch of edit_jump_kernel<draw in registers, blend>; the checks follow flat_step_launch
extern "C" int eegldm_edit_jump(eegldm_ctx* ctx, const float* x, float jump_x, float jump_n, const float* fresh, uint64_t seed, uint64_t offset,
                                const float* known, const float* noise, const float* mask, float a_level, float* out, float* out2, long n) {
  EEG_CHECK(ctx && x && out, "null argument");
  EEG_CHECK(n >= 0, "negative n (%ld)", n);
  EEG_CHECK(jump_x == jump_x && jump_n == jump_n, "a coefficient is NaN");
  EEG_CHECK(a_level > 0.0f && a_level <= 1.0f, "a_level %g outside (0, 1]", (double)a_level);
  EEG_CHECK(!mask || (known && noise), "a mask needs the known signal and the noise");
  // (out == x is the one aliasing the kernel is written for)
  EEG_CHECK(out == x || !ov(out, n, x, n), "out may be x itself, not a shifted view of it");
  EEG_CHECK(!ov(out2, n, out, n) && !ov(out2, n, x, n), "out2 aliases another buffer");
  EEG_CHECK(!ov(fresh, n, out, n) && !ov(fresh, n, out2, n), "fresh aliases an output buffer");
  if (mask)
    for (const float* q : {known, noise, mask}) EEG_CHECK(!ov(q, n, out, n) && !ov(q, n, out2, n), "known / noise / mask alias an output buffer");
  for (const void* q : {(const void*)x, (const void*)fresh, (const void*)out, (const void*)out2, (const void*)(mask ? known : nullptr),
                        (const void*)(mask ? noise : nullptr), (const void*)mask})
    EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
  if (n == 0) return 0;
  long head = vec_head(n, {x, out});
  for (const void* q : {(const void*)fresh, (const void*)out2, (const void*)(mask ? known : nullptr), (const void*)(mask ? noise : nullptr),
                        (const void*)mask})
    if (q && head < n && ((uintptr_t)q & 15) != ((uintptr_t)x & 15)) head = n;
  auto kernel = fresh ? (mask ? edit_jump_kernel<false, true> : edit_jump_kernel<false, false>)
                      : (mask ? edit_jump_kernel<true, true> : edit_jump_kernel<true, false>);
  hipLaunchKernelGGL(kernel, dim3(grid_vec(n, head, ctx)), dim3(NT), 0, ctx->stream, x, jump_x, jump_n, fresh, (unsigned long long)seed,
                     (unsigned long long)offset, known, noise, mask, sqrtf(a_level), sqrtf(1.0f - a_level), out, out2, n, head);
  LAUNCH_CHECK(); return 0;
}
extern "C" int eegldm_edit_window(eegldm_ctx* ctx, const float* mask_win, int B, int Lw, int down, int C, float* mask_lat, const float* input,
                                  const float* decoded, int Co, float* out) {
  EEG_CHECK(ctx && mask_win && (mask_lat || out), "null argument");
  EEG_CHECK(B >= 0 && Lw >= 1 && down >= 1 && Lw % down == 0, "bad sizes (B %d, Lw %d, down %d)", B, Lw, down);
  EEG_CHECK(!mask_lat || C >= 1, "bad channel count %d", C);
  EEG_CHECK(!out || (input && decoded && Co >= 1), "the composite needs input, decoded and Co >= 1");
  const long n_lat = mask_lat ? (long)B * C * (Lw / down) : 0, n_win = out ? (long)B * Co * Lw : 0, nm = (long)B * Lw;
  EEG_CHECK(!ov(mask_lat, n_lat, mask_win, nm) && !ov(mask_lat, n_lat, input, n_win) && !ov(mask_lat, n_lat, decoded, n_win) &&
            !ov(mask_lat, n_lat, out, n_win) && !ov(out, n_win, mask_win, nm) && !ov(out, n_win, input, n_win), "an output aliases another buffer");
  EEG_CHECK(out == decoded || !ov(out, n_win, decoded, n_win), "out may be decoded itself, not a shifted view of it");
  for (const void* q : {(const void*)mask_win, (const void*)mask_lat, (const void*)input, (const void*)decoded, (const void*)out})
    EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
  if (n_lat + n_win == 0) return 0;
  hipLaunchKernelGGL(edit_window_kernel, dim3(grid1d(n_lat > n_win ? n_lat : n_win, ctx)), dim3(NT), 0, ctx->stream, mask_win, n_lat, n_win, Lw, down,
                     C, mask_lat, input, decoded, Co, out);
  LAUNCH_CHECK(); return 0;
}
// ---- long recordings (include/eegldm.h): the slices of a canvas, one sampling step on it, the cross-fade of the decoded windows
static int canvas_geo(int R, int C, int W, int L, int S, int m, int r, CanvasGeo* g) {
  EEG_CHECK(R >= 1 && C >= 1 && W >= 1 && L >= 1, "bad sizes (R %d, C %d, W %d, L %d)", R, C, W, L);
  EEG_CHECK(m >= 0 && r >= 0, "margin %d / ramp %d must be >= 0", m, r);
  EEG_CHECK((long)L >= 3L * m + 2L * r, "window length %d < 3 * margin + 2 * ramp = %ld: more than two windows would carry weight", L, 3L * m + 2L * r);
  EEG_CHECK(S == L - (2 * m + r) && S >= 1, "stride %d is not L - (2 margin + ramp) = %d >= 1", S, L - (2 * m + r));
  const long Lc = (long)(W - 1) * S + L;
  EEG_CHECK(Lc <= 0x7fffffffL - 4, "canvas length %ld: too long", Lc);
  g->C = C; g->W = W; g->L = L; g->S = S; g->m = m; g->r = r; g->Lc = (int)Lc;
  return 0;
}
static long canvas_head(const void* p, long n) {
  const long head = (long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
  return head < n ? head : n;
}
extern "C" int eegldm_canvas_gather(eegldm_ctx* ctx, const float* canvas, int R, int C, int W, int L, int S, float* win, float* win2) {
  EEG_CHECK(ctx && canvas && win, "null argument");
  EEG_CHECK(R >= 1 && C >= 1 && W >= 1 && L >= 1 && S >= 1 && S <= L, "bad sizes (R %d, C %d, W %d, L %d, S %d)", R, C, W, L, S);
  const long Lc = (long)(W - 1) * S + L, n = (long)R * W * C * L, nc = (long)R * C * Lc;
  EEG_CHECK(Lc <= 0x7fffffffL - 4, "canvas length %ld: too long", Lc);
  EEG_CHECK(!ov(canvas, nc, win, n) && !ov(canvas, nc, win2, n) && !ov(win, n, win2, n), "the canvas / window buffers overlap");
  for (const void* q : {(const void*)canvas, (const void*)win, (const void*)win2})
    EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
  CanvasGeo g; g.C = C; g.W = W; g.L = L; g.S = S; g.m = 0; g.r = 0; g.Lc = (int)Lc;
  const long head = canvas_head(win, n);
  hipLaunchKernelGGL(canvas_gather_kernel, dim3(grid_vec(n, head, ctx)), dim3(NT), 0, ctx->stream, g, canvas, win, win2, n, head);
  LAUNCH_CHECK(); return 0;
}
// e == NULL: eegldm_canvas_step; else eegldm_canvas_edit_step with a mask (the checks of the step, then those of the three edit inputs)
static int canvas_step_launch(eegldm_ctx* ctx, const float* mo, float w, int guided, const float* canvas, float* hist, float a_t, int pred,
                              int clip, float cx, float c0, float c1, int R, int C, int W, int L, int m, int r, float* canvas_out, float* win,
                              float* win2, float* x0, const CanvasEditArgs* e) {
  EEG_CHECK(ctx && mo && canvas && canvas_out, "null argument");
  CanvasGeo g;
  EEG_TRY(canvas_geo(R, C, W, L, L - (2 * m + r), m, r, &g));
  EEG_CHECK(pred >= 0 && pred <= 2, "prediction type %d", pred);
  EEG_CHECK(a_t > 0.0f && a_t < 1.0f, "a_t %g outside (0, 1)", (double)a_t);
  EEG_CHECK(!guided || w == w, "guidance_scale is NaN");
  EEG_CHECK(cx == cx && c0 == c0 && c1 == c1, "a coefficient is NaN");
  EEG_CHECK(hist || c1 == 0.0f, "c1 != 0 needs the history buffer");
  EEG_CHECK(win || !win2, "win2 needs win");
  const long n = (long)R * C * g.Lc, nw = (long)R * W * C * L, nm = guided ? 2 * nw : nw;
  EEG_CHECK(!ov(mo, nm, canvas_out, n) && !ov(mo, nm, x0, n) && !ov(mo, nm, hist, n) && !ov(mo, nm, win, nw) && !ov(mo, nm, win2, nw),
            "model_out aliases an output buffer");
  EEG_CHECK(!ov(hist, n, canvas, n) && !ov(hist, n, canvas_out, n) && !ov(hist, n, x0, n) && !ov(hist, n, win, nw) && !ov(hist, n, win2, nw),
            "the history buffer aliases another buffer");
  EEG_CHECK(!ov(x0, n, canvas, n) && !ov(x0, n, canvas_out, n) && !ov(x0, n, win, nw) && !ov(x0, n, win2, nw), "pred_x0 aliases another buffer");
  EEG_CHECK(!ov(win, nw, canvas, n) && !ov(win, nw, canvas_out, n) && !ov(win2, nw, canvas, n) && !ov(win2, nw, canvas_out, n) && !ov(win, nw, win2, nw),
            "win / win2 alias another buffer");
  EEG_CHECK(canvas_out == canvas || !ov(canvas_out, n, canvas, n), "canvas_out may be the canvas itself, not a shifted view of it");
  for (const void* q : {(const void*)mo, (const void*)canvas, (const void*)hist, (const void*)canvas_out, (const void*)win, (const void*)win2, (const void*)x0})
    EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
  CanvasStepArgs a{mo, w, guided ? 1 : 0, canvas, hist, sqrtf(a_t), sqrtf(1.0f - a_t), pred, clip, cx, c0, c1, canvas_out, win, win2, x0, nw};
  const long head = canvas_head(canvas, n);
  if (!e) {
    hipLaunchKernelGGL(canvas_step_kernel, dim3(grid_vec(n, head, ctx)), dim3(NT), 0, ctx->stream, g, a, n, head);
    LAUNCH_CHECK(); return 0;
  }
  for (const float* q : {e->known, e->noise, e->mask}) {
    EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
    EEG_CHECK(!ov(q, n, canvas_out, n) && !ov(q, n, x0, n) && !ov(q, n, hist, n) && !ov(q, n, win, nw) && !ov(q, n, win2, nw),
              "known / noise / mask alias an output buffer");
  }
  hipLaunchKernelGGL(canvas_edit_step_kernel, dim3(grid_vec(n, head, ctx)), dim3(NT), 0, ctx->stream, g, a, *e, n, head);
  LAUNCH_CHECK(); return 0;
}
extern "C" int eegldm_canvas_step(eegldm_ctx* ctx, const float* mo, float w, int guided, const float* canvas, float* hist, float a_t, int pred,
                                  int clip, float cx, float c0, float c1, int R, int C, int W, int L, int m, int r, float* canvas_out,
                                  float* win, float* win2, float* x0) {
  return canvas_step_launch(ctx, mo, w, guided, canvas, hist, a_t, pred, clip, cx, c0, c1, R, C, W, L, m, r, canvas_out, win, win2, x0, nullptr);
}
// mask == NULL: the launch of eegldm_canvas_step itself (known / noise are not read); else the same step with the blend inside it
extern "C" int eegldm_canvas_edit_step(eegldm_ctx* ctx, const float* mo, float w, int guided, const float* canvas, float* hist, float a_t,
                                       float a_next, int pred, int clip, float cx, float c0, float c1, int R, int C, int W, int L, int m, int r,
                                       const float* known, const float* noise, const float* mask, float* canvas_out, float* win, float* win2,
                                       float* x0) {
  EEG_CHECK(a_next > 0.0f && a_next <= 1.0f, "a_next %g outside (0, 1]", (double)a_next);
  EEG_CHECK(!mask || (known && noise), "a mask needs the known signal and the noise");
  const CanvasEditArgs e{known, noise, mask, sqrtf(a_next), sqrtf(1.0f - a_next)};
  return canvas_step_launch(ctx, mo, w, guided, canvas, hist, a_t, pred, clip, cx, c0, c1, R, C, W, L, m, r, canvas_out, win, win2, x0,
                            mask ? &e : nullptr);
}
extern "C" int eegldm_canvas_compose(eegldm_ctx* ctx, const float* decoded, int R, int Co, int W, int Lw, int Sw, int mw, int rw, float* out) {
  EEG_CHECK(ctx && decoded && out, "null argument");
  CanvasGeo g;
  EEG_TRY(canvas_geo(R, Co, W, Lw, Sw, mw, rw, &g));
  const long n = (long)R * Co * g.Lc, nw = (long)R * W * Co * Lw;
  EEG_CHECK(!ov(decoded, nw, out, n), "out overlaps the decoded windows");
  EEG_CHECK(((uintptr_t)decoded & 3) == 0 && ((uintptr_t)out & 3) == 0, "buffers must be 4-byte aligned");
  const long head = canvas_head(out, n);
  hipLaunchKernelGGL(canvas_compose_kernel, dim3(grid_vec(n, head, ctx)), dim3(NT), 0, ctx->stream, g, decoded, out, n, head);
  LAUNCH_CHECK(); return 0;
}
