// Preparing raw recordings (eegldm.recordings): a zero-phase rational-rate FIR resampler over whole-night rows and per-epoch statistics.
//   * resample_fir_kernel<R, XT>: v[i] = xe[i / U] where U divides i, else 0;  y[m] = sum_k h[k] v[m D + k - c], c = (M - 1) / 2.  Only the
//     taps k = k0 + t U, k0 = (c - m D) mod U, meet a sample: output m is the chain over t of h[k0 + t U] xe[j0 + t], j0 = (m D - c + k0) / U,
//     at most ceil(M / U) terms.  A 256-thread workgroup owns `seg` consecutive outputs of one row; thread t owns outputs t, t + 256, ...
//     (R of them: consecutive lanes hold consecutive outputs, so the stores coalesce and the sample reads of a wave walk through LDS with
//     stride D / U).  The terms are taken in chunks of TC: per chunk the workgroup stages the taps phase-major (row p holds h[p], h[p + U],
//     ...; the pitch is odd, so the up to U distinct rows a wave reads at one t fall on distinct banks, equal rows broadcast) and the
//     input span xe[j0(first) + T0 .. j0(last) + T0 + TC) (int16 converted as it is staged, one fmaf; 16-byte loads over the aligned
//     interior of the row, scalar loads for the head, the tail and the reflected edges).  The production shapes (up to 9387 taps at U = 25)
//     take one chunk; chunks exist so that every (M, U, D) the export accepts fits the same 64 KB.  An output is ONE fmaf chain in ascending k
//     from +0 over its own terms, whatever R, seg or the batch; under edge 0 the terms outside the row are skipped, not multiplied.
//   * epoch_stats_kernel: one workgroup per (row, epoch), the epoch in LDS; min / max by < / > from the first sample, the mean in float64, then
//     the root of the float64 mean squared deviation about that mean (two passes); fixed reduction order.
// No atomics, no memset, one writer per element.
#include <type_traits>

#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int RS_MAX_M = 16383, RS_MAX_U = 64, RS_MAX_D = 4096, RS_MAX_R = 8;
constexpr long RS_MAX_L = 1L << 30;
constexpr int RS_T_FLOATS = 10240;      // 40 KB of taps: U rows of an odd pitch
constexpr int RS_X_FLOATS = 6144;       // 24 KB of samples
constexpr int RS_MAX_TC = 3072;         // terms per chunk: leaves half of the sample area to the segment's own span
constexpr int ES_MAX_E = 12288;

template <typename XT> __device__ __forceinline__ float rs_sample(XT v, float g, float o);
template <> __device__ __forceinline__ float rs_sample<float>(float v, float, float) { return v; }
template <> __device__ __forceinline__ float rs_sample<short>(short v, float g, float o) { return fmaf((float)v, g, o); }

// first term of output m: tap k0 in [0, U) and sample j0 (may lie before the row) with m D - c + k0 == j0 U
__device__ __forceinline__ void rs_first(long m, int D, int U, int c, int& k0, long& j0) {
  const long q = m * D - c;
  int r = (int)((-q) % U);
  if (r < 0) r += U;
  k0 = r;
  j0 = (q + r) / U;                                   // exact
}
__device__ __forceinline__ long rs_first_sample(long m, int D, int U, int c) {
  int k0;
  long j0;
  rs_first(m, D, U, c, k0, j0);
  return j0;
}
// Workgroup number on the 2-D grid (x up to 2^20, y up to 65535: a 1-D grid of 256-thread workgroups ends at 2^24 - 1 of them)
constexpr long GRID_X = 1L << 20, GRID_MAX = GRID_X * 65535;
__device__ __forceinline__ long wg_index() { return (long)blockIdx.y * gridDim.x + blockIdx.x; }
inline dim3 wg_grid(long total) {
  const long gx = total < GRID_X ? total : GRID_X;
  return dim3((unsigned)gx, (unsigned)((total + gx - 1) / gx));
}

template <int R, typename XT>
__global__ __launch_bounds__(NT) void resample_fir_kernel(const XT* __restrict__ x, long ldx, const float* __restrict__ gain,
                                                          const float* __restrict__ offset, const float* __restrict__ taps, int M, int U, int D,
                                                          float* __restrict__ y, long ldy, long L, long Lout, int seg, long nseg, long total,
                                                          int TC, int pitch, int edge) {
  __shared__ __attribute__((aligned(16))) float sT[RS_T_FLOATS];
  __shared__ __attribute__((aligned(16))) float sX[RS_X_FLOATS];
  constexpr int G = 16 / (int)sizeof(XT);             // samples per 16-byte load
  const int t = threadIdx.x;
  const long wg = wg_index();
  if (wg >= total) return;                            // the last row of the 2-D grid may be partly empty (the whole workgroup leaves)
  const long b = wg / nseg;
  const long m0 = (wg % nseg) * seg;
  const int n_out = (int)min((long)seg, Lout - m0);   // > 0: the grid holds no empty segment
  const int c = (M - 1) >> 1;
  const int nterm = (M + U - 1) / U;
  const XT* xr = x + b * ldx;
  float g = 0.f, o = 0.f;
  if constexpr (std::is_same<XT, short>::value) { g = gain[b]; o = offset[b]; }
  const long jf = rs_first_sample(m0, D, U, c), jl = rs_first_sample(m0 + n_out - 1, D, U, c);
  const int xspan = (int)(jl - jf);                   // j0 never decreases with m; the host keeps xspan + TC <= RS_X_FLOATS

  // this thread's outputs: tap row, first sample relative to jf, and the terms [lo, hi) that are taken
  int tp[R], xo[R], lo[R], hi[R];
  float acc[R];
  int tA = 0, tB = 0x3fffffff;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int mine = t + r * NT;
    const int oo = mine < n_out ? mine : (t < n_out ? t : 0);      // a slot past the segment repeats a live one and is not stored
    int k0;
    long j0;
    rs_first(m0 + oo, D, U, c, k0, j0);
    const int nt = k0 < M ? (M - 1 - k0) / U + 1 : 0;
    long l = 0, h = nt;
    if (!edge) {                                      // zeros outside the row: those terms are skipped
      if (j0 < 0) l = -j0;
      if (j0 + h > L) h = L - j0;
      if (l > nt) l = nt;
      if (h < l) h = l;
    }
    if (t >= n_out) { l = 0; h = 0; }
    tp[r] = k0 * pitch; xo[r] = (int)(j0 - jf); lo[r] = (int)l; hi[r] = (int)h; acc[r] = 0.f;
    tA = max(tA, lo[r]); tB = min(tB, hi[r]);
  }
  if (tA >= tB) { tA = 0x3fffffff; tB = 0x3fffffff; }  // no term common to all R chains: each runs on its own

  for (int T0 = 0; T0 < nterm; T0 += TC) {
    if (T0) __syncthreads();
    // taps k in [T0 U, (T0 + TC) U): row k % U, column k / U - T0
    const int kend = min(M, (T0 + TC) * U);
    for (int k = T0 * U + t; k < kend; k += NT) {
      const int col = k / U;
      sT[(k - col * U) * pitch + col - T0] = taps[k];
    }
    // samples xe[xb .. xb + count)
    const long xb = jf + T0;
    const int count = min(xspan + TC, RS_X_FLOATS);
    const long ilo = max(xb, 0L), ihi = min(xb + count, L);
    long va = 0, vb = 0;                              // [va, vb): whole 16-byte groups inside the row
    if (ihi > ilo) {
      const int mis = (int)(((uintptr_t)(xr + ilo) & 15u) / sizeof(XT));
      va = min(ilo + (mis ? G - mis : 0), ihi);
      vb = va + (ihi - va) / G * G;
    }
    const int nvec = (int)((vb - va) / G);
    float* sv = sX + (va - xb);
    for (int v = t; v < nvec; v += NT) {
      if constexpr (std::is_same<XT, float>::value) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(xr + va + (long)v * G);
#pragma unroll
        for (int i = 0; i < 4; i++) sv[v * G + i] = w[i];
      } else {
        const uint4 w = *reinterpret_cast<const uint4*>(xr + va + (long)v * G);
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
          sv[v * G + 2 * i] = rs_sample<short>((short)(ww[i] & 0xffffu), g, o);
          sv[v * G + 2 * i + 1] = rs_sample<short>((short)(ww[i] >> 16), g, o);
        }
      }
    }
    for (int i = t; i < count; i += NT) {
      long j = xb + i;
      if (j >= va && j < vb) continue;
      if (edge) j = j < 0 ? -j : (j > L - 1 ? 2 * (L - 1) - j : j);       // a position no output reads may still fall outside: it stays zero
      sX[i] = (j >= 0 && j < L) ? rs_sample<XT>(xr[j], g, o) : 0.f;
    }
    __syncthreads();
    const int T1 = T0 + TC;
    const float* cT = sT - T0;
    const float* cX = sX - T0;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int e = min(min(hi[r], tA), T1);
      for (int tt = max(lo[r], T0); tt < e; tt++) acc[r] = fmaf(cT[tp[r] + tt], cX[xo[r] + tt], acc[r]);
    }
    {
      const int e = min(tB, T1);
      for (int tt = max(tA, T0); tt < e; tt++) {
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = fmaf(cT[tp[r] + tt], cX[xo[r] + tt], acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int e = min(hi[r], T1);
      for (int tt = max(max(tB, lo[r]), T0); tt < e; tt++) acc[r] = fmaf(cT[tp[r] + tt], cX[xo[r] + tt], acc[r]);
    }
  }
  float* yr = y + b * ldy + m0;
#pragma unroll
  for (int r = 0; r < R; r++)
    if (t + r * NT < n_out) yr[t + r * NT] = acc[r];
}

template <int R, typename XT>
void rs_launch(eegldm_ctx* ctx, const void* x, long ldx, const float* gain, const float* offset, const float* taps, int M, int U, int D, float* y,
               long ldy, long B, long L, long Lout, int seg, long nseg, int TC, int pitch, int edge) {
  hipLaunchKernelGGL((resample_fir_kernel<R, XT>), wg_grid(B * nseg), dim3(NT), 0, ctx->stream, (const XT*)x, ldx, gain, offset, taps, M,
                     U, D, y, ldy, L, Lout, seg, nseg, B * nseg, TC, pitch, edge);
}
template <typename XT>
void rs_launch_r(int R, eegldm_ctx* ctx, const void* x, long ldx, const float* gain, const float* offset, const float* taps, int M, int U, int D,
                 float* y, long ldy, long B, long L, long Lout, int seg, long nseg, int TC, int pitch, int edge) {
  if (R == 1) rs_launch<1, XT>(ctx, x, ldx, gain, offset, taps, M, U, D, y, ldy, B, L, Lout, seg, nseg, TC, pitch, edge);
  else if (R == 2) rs_launch<2, XT>(ctx, x, ldx, gain, offset, taps, M, U, D, y, ldy, B, L, Lout, seg, nseg, TC, pitch, edge);
  else if (R == 4) rs_launch<4, XT>(ctx, x, ldx, gain, offset, taps, M, U, D, y, ldy, B, L, Lout, seg, nseg, TC, pitch, edge);
  else rs_launch<8, XT>(ctx, x, ldx, gain, offset, taps, M, U, D, y, ldy, B, L, Lout, seg, nseg, TC, pitch, edge);
}

// ------------------------------------------------------------------------------------------------ epoch statistics
__device__ __forceinline__ float wave_min_lt(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const float w = __shfl_xor(v, o, 64); if (w < v) v = w; }
  return v;
}
__device__ __forceinline__ float wave_max_gt(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const float w = __shfl_xor(v, o, 64); if (w > v) v = w; }
  return v;
}

__global__ __launch_bounds__(NT) void epoch_stats_kernel(const float* __restrict__ x, long ldx, long nE, long total, int E,
                                                         float* __restrict__ out) {
  __shared__ float sE[ES_MAX_E];
  __shared__ double sSum[NT / 64], sSq[NT / 64];
  __shared__ float sMin[NT / 64], sMax[NT / 64];
  __shared__ int sNan[NT / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long wg = wg_index();
  if (wg >= total) return;
  const long b = wg / nE, e = wg % nE;
  const float* xe = x + b * ldx + e * E;
  for (int i = t; i < E; i += NT) sE[i] = xe[i];
  __syncthreads();
  double s = 0.0;
  float mn = sE[0], mx = sE[0];
  int bad = 0;
  for (int i = t; i < E; i += NT) {
    const float v = sE[i];
    s += (double)v;
    if (v < mn) mn = v;
    if (v > mx) mx = v;
    bad |= v != v ? 1 : 0;
  }
  s = wave_sum_d(s); mn = wave_min_lt(mn); mx = wave_max_gt(mx);
  bad = __any(bad) ? 1 : 0;
  if (lane == 0) { sSum[wave] = s; sMin[wave] = mn; sMax[wave] = mx; sNan[wave] = bad; }
  __syncthreads();
  const double mean = (((sSum[0] + sSum[1]) + sSum[2]) + sSum[3]) / (double)E;
  double q = 0.0;
  for (int i = t; i < E; i += NT) {
    const double d = (double)sE[i] - mean;
    q += d * d;
  }
  q = wave_sum_d(q);
  if (lane == 0) sSq[wave] = q;
  __syncthreads();
  if (t == 0) {
    float r0 = sMin[0], r1 = sMax[0];
    for (int w = 1; w < NT / 64; w++) { if (sMin[w] < r0) r0 = sMin[w]; if (sMax[w] > r1) r1 = sMax[w]; }
    const double var = (((sSq[0] + sSq[1]) + sSq[2]) + sSq[3]) / (double)E;
    float r2 = (float)mean, r3 = (float)sqrt(var);
    if (sNan[0] | sNan[1] | sNan[2] | sNan[3]) { r0 = r1 = r2 = r3 = __builtin_nanf(""); }
    float* po = out + (b * nE + e) * 4;
    po[0] = r0; po[1] = r1; po[2] = r2; po[3] = r3;
  }
}

// EEGLDM_RS_SEG: outputs per workgroup (at most 256 R and what the 24 KB sample area holds); EEGLDM_RS_R = 1 | 2 | 4 | 8: outputs per thread.
// Developer switches: no bit of the result depends on either.
int rs_env_seg() { EEG_ENV_VAR(int, n, getenv("EEGLDM_RS_SEG") ? atoi(getenv("EEGLDM_RS_SEG")) : 0); return n; }
int rs_env_r() { EEG_ENV_VAR(int, r, getenv("EEGLDM_RS_R") ? atoi(getenv("EEGLDM_RS_R")) : 0); return r; }
}  // namespace

extern "C" int eegldm_resample_fir(eegldm_ctx* ctx, const void* x, long ldx, int xtype, const float* gain, const float* offset, const float* taps,
                                   int M, int U, int D, float* y, long ldy, long B, long L, int edge) {
  EEG_CHECK(ctx && x && taps && y, "null argument");
  EEG_CHECK(xtype == 0 || xtype == 1, "xtype %d is neither 0 (fp32) nor 1 (int16)", xtype);
  EEG_CHECK(!(xtype == 1 && !(gain && offset)), "int16 rows need gain and offset");
  EEG_CHECK(M >= 1 && M <= RS_MAX_M, "M %d outside [1, %d]", M, RS_MAX_M);
  EEG_CHECK(M & 1, "M %d is even: a zero-phase filter needs a centre tap", M);
  EEG_CHECK(U >= 1 && U <= RS_MAX_U, "U %d outside [1, %d]", U, RS_MAX_U);
  EEG_CHECK(D >= 1 && D <= RS_MAX_D, "D %d outside [1, %d]", D, RS_MAX_D);
  EEG_CHECK(L >= 1 && L <= RS_MAX_L, "L %ld outside [1, 2^30]", L);
  EEG_CHECK(edge == 0 || edge == 1, "edge %d is neither 0 (zeros) nor 1 (reflect)", edge);
  const int c = (M - 1) / 2;
  EEG_CHECK(!(edge == 1 && (c + U - 1) / U > L - 1), "reflect needs ceil(c / U) <= L - 1, got M %d U %d L %ld", M, U, L);
  EEG_CHECK(B >= 0 && B <= 0x7fffffffL, "B %ld outside [0, 2^31)", B);
  const long Lout = (L * U + D - 1) / D;
  EEG_CHECK(ldx >= L && ldy >= Lout, "row strides %ld / %ld shorter than the rows %ld / %ld", ldx, ldy, L, Lout);
  EEG_CHECK((const void*)x != (const void*)y, "in-place resampling is not supported (x == y)");
  EEG_CHECK((((uintptr_t)taps | (uintptr_t)y | (uintptr_t)gain | (uintptr_t)offset) & 3u) == 0 && ((uintptr_t)x & (xtype ? 1u : 3u)) == 0,
            "fp32 pointers must be 4-byte aligned, int16 pointers 2-byte aligned");
  // terms per chunk and the odd pitch of the tap rows
  const int nterm = (M + U - 1) / U;
  int TC = RS_T_FLOATS / U - 1;
  if (TC > RS_MAX_TC) TC = RS_MAX_TC;
  if (TC > nterm) TC = nterm;
  const int pitch = TC | 1;
  // outputs per workgroup: 256 R, less where the segment's input span (seg - 1) D / U + 1 + TC would not fit the sample area
  const long fit = (long)(RS_X_FLOATS - TC - 2) * U / D + 1;
  // outputs per thread, from the measured times (profiles/prepare_timing.txt, 8-h rows): R = 8 takes 0.90 .. 0.99 of R = 4's time at 100, 125 and
  // 256 Hz.  8 where a full segment of 2048 outputs fits the sample area (at 512 Hz 1126 fit: R = 8 would run half its chains for nothing)
  // and the rows still give two such workgroups per CU; else 4.
  int R = rs_env_r();
  if (R != 1 && R != 2 && R != 4 && R != 8) R = (fit >= NT * 8 && B * Lout >= 2L * ctx->num_cu * NT * 8) ? 8 : 4;
  long seg = rs_env_seg() > 0 ? rs_env_seg() : NT * R;
  if (seg > NT * R) seg = NT * R;
  if (seg > fit) seg = fit;
  if (seg > Lout) seg = Lout;
  const long nseg = (Lout + seg - 1) / seg;
  EEG_CHECK(B == 0 || nseg <= GRID_MAX / B, "B %ld rows of %ld segments exceed the grid of %ld workgroups", B, nseg, GRID_MAX);
  if (B == 0) return 0;
  if (xtype == 0) rs_launch_r<float>(R, ctx, x, ldx, gain, offset, taps, M, U, D, y, ldy, B, L, Lout, (int)seg, nseg, TC, pitch, edge);
  else rs_launch_r<short>(R, ctx, x, ldx, gain, offset, taps, M, U, D, y, ldy, B, L, Lout, (int)seg, nseg, TC, pitch, edge);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_epoch_stats(eegldm_ctx* ctx, const float* x, long ldx, long B, long L, int E, float* out) {
  EEG_CHECK(ctx && x && out, "null argument");
  EEG_CHECK(E >= 1 && E <= ES_MAX_E, "E %d outside [1, %d]", E, ES_MAX_E);
  EEG_CHECK(L >= 0 && L <= RS_MAX_L, "L %ld outside [0, 2^30]", L);
  EEG_CHECK(B >= 0 && B <= 0x7fffffffL, "B %ld outside [0, 2^31)", B);
  EEG_CHECK(ldx >= L, "row stride %ld shorter than L %ld", ldx, L);
  EEG_CHECK((((uintptr_t)x | (uintptr_t)out) & 3u) == 0, "float pointers must be 4-byte aligned");
  const long nE = L / E;
  EEG_CHECK(B == 0 || nE <= GRID_MAX / B, "B %ld rows of %ld epochs exceed the grid of %ld workgroups", B, nE, GRID_MAX);
  if (B == 0 || nE == 0) return 0;
  hipLaunchKernelGGL(epoch_stats_kernel, wg_grid(B * nE), dim3(NT), 0, ctx->stream, x, ldx, nE, B * nE, E, out);
  LAUNCH_CHECK();
  return 0;
}
