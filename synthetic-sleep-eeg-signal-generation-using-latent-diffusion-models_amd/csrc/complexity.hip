// Signal-complexity primitives (eegldm.metrics: Hjorth parameters, permutation entropy, (multiscale) sample entropy): three passes over rows
// of at most 4096 fp32 samples that sit in LDS (16 KB).  The definitions are in include/eegldm.h.
//   * row_moments_kernel: one 256-thread workgroup per row.  Pass 1: float64 sums of x, d1, d2 and |d1|, min and max; pass 2: central sums
//     about the means of pass 1 and the sign changes of x - mean.  A thread's chain runs over the indices t, t + 256, ... in ascending order from
//     +0, a fixed xor butterfly folds a wave, the four waves are added in index order: the bits do not depend on B or on the other rows.
//   * ordinal_counts_kernel: one workgroup per row, a position per thread and stride, the order! bins and the skipped count in LDS with integer
//     LDS atomics (integers: any order of the adds gives the same counts), stored by plain stores at the end.
//   * template_matches_kernel: the O(L^2) pair count of sample entropy, LAG per thread.  With N = L / scale coarse-grained samples y and T = N - m
//     templates, the pairs (i, i + d) of lag d match at length m iff e_d[n] = |y[n] - y[n + d]| <= r holds for n = i .. i + m - 1, at length
//     m + 1 iff it also holds at n = i + m.  A lane owns lag d, walks n = 0 .. N - d - 1 and keeps the length of the current run of e_d: a run of
//     >= m that ends at n adds one to B unless n is the last step (whose window would start at template T - d, outside the range: y[N - 1]
//     enters A only), a run of >= m + 1 adds one to A.  That is one subtract-compare per pair whatever m; y[n] is a broadcast read and
//     y[n + d] a read of consecutive words by consecutive lanes, so no LDS bank is asked twice.  Lane s walks lag s and then lag T - s:
//     N + m steps for every lane, the triangle is balanced.  A wave owns 64 consecutive slots s; the slots of a row are dealt over G
//     workgroups x W waves, so that a handful of rows still fills the chip.  Counts are integers: a lane's fit 32 bits (a row has at most
//     4095 * 4094 / 2 < 2^23 pairs), a wave is folded by shuffles, a workgroup through LDS, and the G workgroups of a row write 32-bit
//     partials that a second small launch adds in index order (G == 1 stores the row's counts at once).  No atomics on memory, no memset.
#include "common.h"

namespace {
constexpr int NT = 256, NW = NT / 64;
constexpr int CX_MAX_L = 4096;
constexpr int CX_MAX_ORDER = 6, CX_MAX_BINS = 720;
constexpr int CX_MAX_M = 4, CX_MAX_SCALE = 64;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ moments
// sums of K doubles per thread over the workgroup, the same total in every thread: butterfly per wave, then the waves in index order
template <int K>
__device__ __forceinline__ void block_sum_d(double (&v)[K], double (*sh)[K]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) v[k] = wave_sum_d(v[k]);
  __syncthreads();                                     // the previous use of sh is over
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) sh[wave][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    double s = sh[0][k];
#pragma unroll
    for (int w = 1; w < NW; w++) s += sh[w][k];
    v[k] = s;
  }
}

__global__ __launch_bounds__(NT) void row_moments_kernel(const float* __restrict__ x, long ldx, int L, double* __restrict__ out) {
  __shared__ float sx[CX_MAX_L];
  __shared__ double sh[NW][4];
  __shared__ float smn[NW], smx[NW];
  __shared__ int sflag[NW], ssc[NW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* xr = x + (long)blockIdx.x * ldx;
  for (int i = t; i < L; i += NT) sx[i] = xr[i];
  __syncthreads();
  // pass 1: sums, extremes
  double s1[4] = {0.0, 0.0, 0.0, 0.0};                 // x, d1, d2, |d1|
  float mn = sx[0], mx = sx[0];
  int nan = 0;
  for (int i = t; i < L; i += NT) {
    const float f = sx[i];
    const double a = (double)f;
    s1[0] += a;
    mn = f < mn ? f : mn; mx = f > mx ? f : mx; nan |= f != f ? 1 : 0;
    if (i + 1 < L) {
      const double b = (double)sx[i + 1];
      const double d1 = b - a;
      s1[1] += d1; s1[3] += fabs(d1);
      if (i + 2 < L) s1[2] += ((double)sx[i + 2] - b) - d1;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float p = __shfl_xor(mn, o, 64), q = __shfl_xor(mx, o, 64);
    mn = p < mn ? p : mn; mx = q > mx ? q : mx; nan |= __shfl_xor(nan, o, 64);
  }
  if (lane == 0) { smn[wave] = mn; smx[wave] = mx; sflag[wave] = nan; }
  block_sum_d<4>(s1, sh);                              // (its barriers also publish smn / smx / sflag)
  const double mean = s1[0] / (double)L;
  const double mean1 = L > 1 ? s1[1] / (double)(L - 1) : 0.0;
  const double mean2 = L > 2 ? s1[2] / (double)(L - 2) : 0.0;
  // pass 2: central sums, sign changes of x - mean
  double s2[4] = {0.0, 0.0, 0.0, 0.0};
  int sc = 0;
  for (int i = t; i < L; i += NT) {
    const double a = (double)sx[i];
    const double c = a - mean;
    s2[0] += c * c;
    if (i >= 1) sc += (((double)sx[i - 1] - mean) < 0.0) != (c < 0.0) ? 1 : 0;
    if (i + 1 < L) {
      const double b = (double)sx[i + 1];
      const double d1 = b - a, c1 = d1 - mean1;
      s2[1] += c1 * c1;
      if (i + 2 < L) {
        const double c2 = (((double)sx[i + 2] - b) - d1) - mean2;
        s2[2] += c2 * c2;
      }
    }
  }
  sc = wave_sum_i(sc);
  if (lane == 0) ssc[wave] = sc;
  block_sum_d<4>(s2, sh);
  if (t == 0) {
    float a = smn[0], b = smx[0];
    int f = sflag[0], n = ssc[0];
    for (int w = 1; w < NW; w++) { a = smn[w] < a ? smn[w] : a; b = smx[w] > b ? smx[w] : b; f |= sflag[w]; n += ssc[w]; }
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double* o = out + (long)blockIdx.x * 8;
    o[0] = mean; o[1] = s2[0]; o[2] = s2[1]; o[3] = s2[2]; o[4] = s1[3]; o[5] = (double)n;
    o[6] = f ? qnan : (double)a; o[7] = f ? qnan : (double)b;
  }
}

// ------------------------------------------------------------------------------------------------ ordinal patterns
__global__ __launch_bounds__(NT) void ordinal_counts_kernel(const float* __restrict__ x, long ldx, int L, int order, int delay, int nbins,
                                                            int* __restrict__ counts, int* __restrict__ skipped) {
  __shared__ float sx[CX_MAX_L];
  __shared__ int hist[CX_MAX_BINS + 1];                // slot nbins: the skipped positions
  const int t = threadIdx.x;
  const float* xr = x + (long)blockIdx.x * ldx;
  for (int i = t; i < L; i += NT) sx[i] = xr[i];
  for (int i = t; i <= nbins; i += NT) hist[i] = 0;
  __syncthreads();
  const int P = L - (order - 1) * delay;               // >= 1 (checked by the caller): the last read is sx[P - 1 + (order - 1) delay] = sx[L - 1]
  for (int p = t; p < P; p += NT) {
    float v[CX_MAX_ORDER];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < CX_MAX_ORDER; k++) {
      v[k] = k < order ? sx[p + k * delay] : 0.f;
      ok = ok && finite_f(v[k]);
    }
    int idx = 0, fact = 1;                             // Lehmer code, from the last element: fact = (order - 1 - k)!
#pragma unroll
    for (int k = CX_MAX_ORDER - 2; k >= 0; k--) {
      if (k < order - 1) {
        int c = 0;
#pragma unroll
        for (int l = k + 1; l < CX_MAX_ORDER; l++) c += (l < order && v[l] < v[k]) ? 1 : 0;
        idx += c * fact;
        fact *= order - k;                             // (order - 1 - (k - 1))! = (order - 1 - k)! (order - k)
      }
    }
    atomicAdd(&hist[ok ? idx : nbins], 1);
  }
  __syncthreads();
  int* cr = counts + (long)blockIdx.x * nbins;
  for (int i = t; i < nbins; i += NT) cr[i] = hist[i];
  if (t == 0) skipped[blockIdx.x] = hist[nbins];
}

// ------------------------------------------------------------------------------------------------ template matches
// one lag: the steps n = 0 .. N - d - 1 of e_d, the last of which can only complete a window of length m + 1
__device__ __forceinline__ void walk_lag(const float* sy, int N, int d, int m, float r, int& cb, int& ca) {
  const int last = N - d - 1;                          // >= m >= 1: d <= T - 1 = N - m - 1
  int run = 0;
#pragma unroll 4
  for (int n = 0; n < last; n++) {
    const bool e = fabsf(sy[n] - sy[n + d]) <= r;      // one fp32 rounding of the difference; a NaN on either side or in r: no match
    run = e ? run + 1 : 0;
    cb += run >= m ? 1 : 0;
    ca += run > m ? 1 : 0;
  }
  ca += (fabsf(sy[last] - sy[last + d]) <= r && run >= m) ? 1 : 0;
}

// grid (B, G); W = blockDim.x / 64 waves; wave w of workgroup g owns the slot chunks c = g W + w, + G W, ...; slot s = 64 c + lane + 1 in [1, T / 2]
__global__ __launch_bounds__(NT) void template_matches_kernel(const float* __restrict__ x, long ldx, int L, int m, int scale,
                                                              const float* __restrict__ r, long long* __restrict__ counts,
                                                              unsigned* __restrict__ partials) {
  __shared__ float sy[CX_MAX_L];
  __shared__ int sred[NW][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, W = blockDim.x >> 6;
  const int N = L / scale, T = N - m, S = T >> 1;
  const float* xr = x + (long)blockIdx.x * ldx;
  const float fs = (float)scale;
  for (int j = t; j < N; j += blockDim.x) {
    const float* p = xr + (long)j * scale;             // the last read is x[N scale - 1], inside the row
    float acc = 0.f;
    for (int k = 0; k < scale; k++) acc = acc + p[k];
    sy[j] = acc / fs;
  }
  const float rb = r[blockIdx.x];
  __syncthreads();
  int cb = 0, ca = 0;
  const int G = gridDim.y, nch = (S + 63) >> 6;
  for (int c = blockIdx.y * W + wave; c < nch; c += G * W) {
    const int s = 64 * c + lane + 1;
    if (s <= S) {
      walk_lag(sy, N, s, m, rb, cb, ca);
      if (2 * s != T) walk_lag(sy, N, T - s, m, rb, cb, ca);
    }
  }
  cb = wave_sum_i(cb); ca = wave_sum_i(ca);
  if (lane == 0) { sred[wave][0] = cb; sred[wave][1] = ca; }
  __syncthreads();
  if (t == 0) {
    int b = 0, a = 0;
    for (int w = 0; w < W; w++) { b += sred[w][0]; a += sred[w][1]; }
    if (G == 1) {
      counts[2 * (long)blockIdx.x] = b; counts[2 * (long)blockIdx.x + 1] = a;
    } else {
      unsigned* pr = partials + ((long)blockIdx.x * G + blockIdx.y) * 2;
      pr[0] = (unsigned)b; pr[1] = (unsigned)a;
    }
  }
}

__global__ void template_fold_kernel(const unsigned* __restrict__ partials, long B, int G, long long* __restrict__ counts) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (row, which)
  if (i >= 2 * B) return;
  const unsigned* p = partials + (i >> 1) * G * 2 + (i & 1);
  long long s = 0;
  for (int g = 0; g < G; g++) s += p[2 * g];
  counts[i] = s;
}

// EEGLDM_TM_SPLIT = G, EEGLDM_TM_WAVES = 1 | 4: workgroups per row and waves per workgroup of eegldm_template_matches instead of its rule
// (developer switches: the counts do not depend on them)
int tm_env_split() { EEG_ENV_VAR(int, g, getenv("EEGLDM_TM_SPLIT") ? atoi(getenv("EEGLDM_TM_SPLIT")) : 0); return g; }
int tm_env_waves() { EEG_ENV_VAR(int, w, getenv("EEGLDM_TM_WAVES") ? atoi(getenv("EEGLDM_TM_WAVES")) : 0); return w; }
}  // namespace

extern "C" int eegldm_row_moments(eegldm_ctx* ctx, const float* x, long ldx, long B, int L, double* out) {
  EEG_CHECK(ctx && x && out, "null argument");
  EEG_CHECK(L >= 1 && L <= CX_MAX_L, "L %d outside [1, %d]", L, CX_MAX_L);
  EEG_CHECK(B >= 0 && B <= 0x7fffffffL, "B %ld outside [0, 2^31)", B);
  EEG_CHECK(ldx >= L, "row stride %ld shorter than L %d", ldx, L);
  EEG_CHECK(((uintptr_t)x & 3u) == 0 && ((uintptr_t)out & 7u) == 0, "x must be 4-byte aligned and out 8-byte aligned");
  if (B == 0) return 0;
  hipLaunchKernelGGL(row_moments_kernel, dim3((unsigned)B), dim3(NT), 0, ctx->stream, x, ldx, L, out);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_ordinal_counts(eegldm_ctx* ctx, const float* x, long ldx, long B, int L, int order, int delay, int* counts, int* skipped) {
  EEG_CHECK(ctx && x && counts && skipped, "null argument");
  EEG_CHECK(L >= 1 && L <= CX_MAX_L, "L %d outside [1, %d]", L, CX_MAX_L);
  EEG_CHECK(order >= 2 && order <= CX_MAX_ORDER, "order %d outside [2, %d]", order, CX_MAX_ORDER);
  EEG_CHECK(delay >= 1, "delay %d < 1", delay);
  EEG_CHECK((long)(order - 1) * delay < L, "(order - 1) * delay = %ld does not leave one position in a row of %d samples", (long)(order - 1) * delay, L);
  EEG_CHECK(B >= 0 && B <= 0x7fffffffL, "B %ld outside [0, 2^31)", B);
  EEG_CHECK(ldx >= L, "row stride %ld shorter than L %d", ldx, L);
  EEG_CHECK((((uintptr_t)x | (uintptr_t)counts | (uintptr_t)skipped) & 3u) == 0, "pointers must be 4-byte aligned");
  if (B == 0) return 0;
  int nbins = 1;
  for (int k = 2; k <= order; k++) nbins *= k;
  hipLaunchKernelGGL(ordinal_counts_kernel, dim3((unsigned)B), dim3(NT), 0, ctx->stream, x, ldx, L, order, delay, nbins, counts, skipped);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_template_matches(eegldm_ctx* ctx, const float* x, long ldx, long B, int L, int m, int scale, const float* r, long long* counts) {
  EEG_CHECK(ctx && x && r && counts, "null argument");
  EEG_CHECK(L >= 1 && L <= CX_MAX_L, "L %d outside [1, %d]", L, CX_MAX_L);
  EEG_CHECK(m >= 1 && m <= CX_MAX_M, "m %d outside [1, %d]", m, CX_MAX_M);
  EEG_CHECK(scale >= 1 && scale <= CX_MAX_SCALE, "scale %d outside [1, %d]", scale, CX_MAX_SCALE);
  EEG_CHECK(L / scale - m >= 2, "L / scale - m = %d: fewer than two templates", L / scale - m);
  EEG_CHECK(B >= 0 && B <= 0x7fffffffL, "B %ld outside [0, 2^31)", B);
  EEG_CHECK(ldx >= L, "row stride %ld shorter than L %d", ldx, L);
  EEG_CHECK((((uintptr_t)x | (uintptr_t)r) & 3u) == 0 && ((uintptr_t)counts & 7u) == 0, "x and r must be 4-byte aligned and counts 8-byte aligned");
  if (B == 0) return 0;
  // geometry: chunks of 64 slots (a slot = the lags s and T - s), one per wave and turn.  Four waves per workgroup and one workgroup per row
  // while the rows alone give two workgroups per CU; fewer rows are cut into G workgroups each, of one wave where that is needed to reach it.
  const int S = (L / scale - m) / 2, nch = (S + 63) / 64;
  const long want = (2L * ctx->num_cu + B - 1) / B;
  int W = NW, G = 1;
  if (want > (nch + NW - 1) / NW) W = 1;
  if (want > 1) G = (int)(want < nch ? want : nch);
  if (tm_env_waves() == 1 || tm_env_waves() == NW) W = tm_env_waves();
  if (tm_env_split() >= 1) G = tm_env_split();
  const int most = (nch + W - 1) / W;                  // more workgroups than chunk turns would idle
  if (G > most) G = most;
  unsigned* ws = nullptr;
  if (G > 1) {
    const size_t need = sizeof(unsigned) * 2 * (size_t)B * G;
    if (ctx->splitk_ws_bytes < need) {
      if (ctx->splitk_ws) { HIP_TRY(hipStreamSynchronize(ctx->stream)); if (ctx->side_on) HIP_TRY(hipStreamSynchronize(ctx->side)); HIP_TRY(hipFree(ctx->splitk_ws)); ctx->splitk_ws = nullptr; ctx->splitk_ws_bytes = 0; }
      HIP_TRY(hipMalloc(&ctx->splitk_ws, need)); ctx->splitk_ws_bytes = need;
    }
    ws = (unsigned*)ctx->splitk_ws;
  }
  hipLaunchKernelGGL(template_matches_kernel, dim3((unsigned)B, (unsigned)G), dim3(64 * W), 0, ctx->stream, x, ldx, L, m, scale, r, counts, ws);
  LAUNCH_CHECK();
  if (G > 1) {
    hipLaunchKernelGGL(template_fold_kernel, dim3((unsigned)((2 * B + NT - 1) / NT)), dim3(NT), 0, ctx->stream, (const unsigned*)ws, B, G, counts);
    LAUNCH_CHECK();
  }
  return 0;
}
