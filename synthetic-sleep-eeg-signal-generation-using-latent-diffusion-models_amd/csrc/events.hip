// Sleep micro-structure primitives (eegldm.metrics: spindle and slow-wave detectors): a zero-phase FIR filter over rows of windows and the
// extraction of thresholded runs with per-event features.  fp32 throughout.
//   * fir_same_kernel<R>: y[b][n] = sum_k taps[k] xe[b][n + k - c], c = (M - 1) / 2, xe the row extended by zeros or by whole-sample
//     reflection; mode 1 squares every sample on the way in and stores sqrt(max(sum, 0)) (RMS envelope; a non-finite sum stays non-finite).  Direct form on the vector ALU: a
//     256-thread workgroup owns one row and one segment of its outputs (grid.y segments), stages the extended segment (already squared in
//     mode 1) and the taps into LDS; a thread produces R consecutive outputs from a register window that slides by 8 samples per block of 8
//     taps: 8 R fmaf per two 16-byte sample reads and two broadcast tap reads.  The last M % 8 taps run one at a time, so no padded zero
//     tap ever multiplies a sample: an output is ONE fmaf chain over its own support in ascending k from +0, whatever R, the segment
//     length or the batch, and a non-finite sample reaches exactly the outputs whose support holds it.
//   * threshold_events_kernel: one wave per row, lane l owns samples [64 l, 64 l + 64).  Ballots over coalesced loads give every lane the
//     64-bit activity mask of its chunk (and the mask of upward zero crossings of aux); max / min scans over the lanes give the last active
//     index before a chunk and the first one after it, which decides the closing of stretches that cross lanes; a min scan from the right
//     gives the end of a run that leaves its chunk; prefix sums give the raw-run and crossing counts of any interval and the ordinal of the
//     kept events.  The lane that owns a run's start walks it for the features (runs outside [min_len, max_len] are rejected unwalked).
//     No atomics, no memset, one writer per element.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int FIR_MAX_M = 2049, FIR_MAX_L = 4096, FIR_MAX_R = 12;
constexpr int FIR_LEAD = 1;           // sample i of the staged segment sits at sX[FIR_LEAD + i]: (R - 1 + FIR_LEAD) % 4 == 0 aligns the 16-byte reads
constexpr int FIR_TAPS_FLOATS = 2056;
constexpr int FIR_X_FLOATS = FIR_LEAD + NT * FIR_MAX_R + FIR_MAX_M - 1 + 7;
constexpr int IDX_NONE = 0x3fffffff;

template <int R>
__global__ __launch_bounds__(NT) void fir_same_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ taps, int M,
                                                      float* __restrict__ y, long ldy, int L, int seg_len, int edge, int mode) {
  static_assert((R - 1 + FIR_LEAD) % 4 == 0 && R <= FIR_MAX_R, "window reads must be 16-byte aligned");
  __shared__ __attribute__((aligned(16))) float sT[FIR_TAPS_FLOATS];
  __shared__ __attribute__((aligned(16))) float sX[FIR_X_FLOATS];
  const int t = threadIdx.x;
  const int seg0 = blockIdx.y * seg_len;
  const int n_out = min(seg_len, L - seg0);           // > 0: the grid holds no empty segment
  const int c = (M - 1) >> 1;
  const int ext = n_out + M - 1;                      // <= NT * R + M - 1
  const float* xr = x + (long)blockIdx.x * ldx;
  for (int i = t; i < M; i += NT) sT[i] = taps[i];
  for (int i = t; i < ext; i += NT) {
    int j = seg0 - c + i;                             // in [-c, L - 1 + c]
    float v = 0.f;
    if (edge) {
      j = j < 0 ? -j : (j > L - 1 ? 2 * (L - 1) - j : j);      // c <= L - 1 (checked by the caller): back inside the row
      v = xr[j];
    } else if (j >= 0 && j < L) {
      v = xr[j];
    }
    sX[FIR_LEAD + i] = mode ? v * v : v;
  }
  __syncthreads();
  const int o0 = t * R;
  if (o0 >= n_out) return;
  // sp[r + k] = xe[n0 + r + k - c].  A thread whose last outputs lie past n_out reads LDS words nobody staged: those words can only feed the
  // accumulators acc[r] with o0 + r >= n_out, whose stores are masked below, and every index stays inside sX.
  const float* sp = sX + FIR_LEAD + o0;
  float acc[R], w[R + 7];
#pragma unroll
  for (int r = 0; r < R; r++) acc[r] = 0.f;
#pragma unroll
  for (int i = 0; i < R - 1; i++) w[i] = sp[i];
  int kb = 0;
  for (; kb + 8 <= M; kb += 8) {
    const f32x4 n0 = *reinterpret_cast<const f32x4*>(sp + kb + R - 1), n1 = *reinterpret_cast<const f32x4*>(sp + kb + R + 3);
    const f32x4 t0 = *reinterpret_cast<const f32x4*>(sT + kb), t1 = *reinterpret_cast<const f32x4*>(sT + kb + 4);
#pragma unroll
    for (int i = 0; i < 4; i++) { w[R - 1 + i] = n0[i]; w[R + 3 + i] = n1[i]; }
    const float tk[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
      for (int r = 0; r < R; r++) acc[r] = fmaf(tk[j], w[r + j], acc[r]);
#pragma unroll
    for (int i = 0; i < R - 1; i++) w[i] = w[i + 8];
  }
  for (; kb < M; kb++) {
    const float tk = sT[kb];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = fmaf(tk, sp[kb + r], acc[r]);
  }
  float* yr = y + (long)blockIdx.x * ldy + seg0 + o0;
#pragma unroll
  for (int r = 0; r < R; r++) {
    float v = acc[r];
    if (mode) v = sqrtf(v < 0.f && v >= -3.402823466e38f ? 0.f : v);      // max(sum, 0) for finite sums; a NaN stays, -inf (negative taps) becomes NaN
    if (o0 + r < n_out) yr[r] = v;
  }
}

template <int R>
void fir_launch(eegldm_ctx* ctx, const float* x, long ldx, const float* taps, int M, float* y, long ldy, long B, int L, int seg_len, int nseg,
                int edge, int mode) {
  hipLaunchKernelGGL(fir_same_kernel<R>, dim3((unsigned)B, (unsigned)nseg), dim3(NT), 0, ctx->stream, x, ldx, taps, M, y, ldy, L, seg_len, edge, mode);
}

// ------------------------------------------------------------------------------------------------ runs above a threshold
typedef unsigned long long u64;
constexpr int EV_MAX_L = 4096, EV_MAX_E = 64, EV_WAVES = NT / 64;

__device__ __forceinline__ u64 low_bits(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }     // n in [0, 64]

struct EvWave {               // per wave: the masks and prefix counts every lane may look up for any index of the row
  u64 rawstart[65], up[65];
  int rs_before[65], up_before[65];
};
// marks at indices < n, from a lane-wise mask and its exclusive prefix count (slot 64: the whole row)
__device__ __forceinline__ int count_before(const u64* mask, const int* before, int n) {
  const int l = n >> 6;
  return before[l] + __popcll(mask[l] & low_bits(n & 63));
}

__global__ __launch_bounds__(NT) void threshold_events_kernel(const float* __restrict__ s, long lds_, const float* __restrict__ aux, long ldaux,
                                                              const float* __restrict__ thr, long B, int L, int min_len, int max_len,
                                                              int merge_gap, int drop_edge, int E, int* __restrict__ counts,
                                                              int* __restrict__ ev_i, float* __restrict__ ev_f) {
  __shared__ EvWave sh[EV_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = (long)blockIdx.x * EV_WAVES + wave;
  const bool live = b < B;                              // a wave past the batch builds empty masks and writes nothing
  EvWave& W = sh[wave];
  const float* sr = s + (live ? b : 0) * lds_;
  const float* ar = aux ? aux + (live ? b : 0) * ldaux : nullptr;
  const float th = live ? thr[b] : 0.f;
  const int nch = (L + 63) >> 6;
  u64 a = 0, up = 0;
  for (int j = 0; j < nch; j++) {
    const int n = 64 * j + lane;
    const bool in = live && n < L;
    const bool act = in && sr[n] > th;                  // NaN on either side: inactive; a tie: inactive
    const u64 m = __ballot(act);
    if (lane == j) a = m;
    if (ar) {
      const bool u = in && n >= 1 && ar[n - 1] < 0.f && ar[n] >= 0.f;
      const u64 mu = __ballot(u);
      if (lane == j) up = mu;
    }
  }
  const int base = 64 * lane;
  const int nvalid = min(64, max(0, L - base));
  // last active index before this chunk, first active index after it
  int prev_a = a ? base + 63 - __builtin_clzll(a) : -1;
  int next_a = a ? base + __builtin_ctzll(a) : IDX_NONE;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int p = __shfl_up(prev_a, d, 64), q = __shfl_down(next_a, d, 64);
    if (lane >= d) prev_a = max(prev_a, p);
    if (lane + d < 64) next_a = min(next_a, q);
  }
  prev_a = __shfl_up(prev_a, 1, 64); if (lane == 0) prev_a = -1;
  next_a = __shfl_down(next_a, 1, 64); if (lane == 63) next_a = IDX_NONE;
  // closing: an inactive stretch strictly between two active samples, at most merge_gap long, becomes active
  u64 closed = a;
  for (u64 z = ~a & low_bits(nvalid); z;) {
    const int s0 = __builtin_ctzll(z);
    const u64 rest = ~(z >> s0);                        // the shifted-in top bits count as the stretch's end
    const int len = rest ? __builtin_ctzll(rest) : 64;
    const u64 bits = low_bits(len) << s0;
    const int p = s0 > 0 ? base + s0 - 1 : prev_a;
    const int q = s0 + len < nvalid ? base + s0 + len : (nvalid < 64 ? IDX_NONE : next_a);
    if (p >= 0 && q != IDX_NONE && q - p - 1 <= merge_gap) closed |= bits;
    z &= ~bits;
  }
  // run starts of the raw and of the closed set
  const u64 a_prev = __shfl_up(a, 1, 64), c_prev = __shfl_up(closed, 1, 64);
  const u64 rawstart = a & ~((a << 1) | (lane ? a_prev >> 63 : 0ull));
  const u64 cstart = closed & ~((closed << 1) | (lane ? c_prev >> 63 : 0ull));
  // first index at or after the next chunk that is outside the closed set (indices >= L are outside)
  int zero_after = ~closed ? base + __builtin_ctzll(~closed) : IDX_NONE;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int q = __shfl_down(zero_after, d, 64);
    if (lane + d < 64) zero_after = min(zero_after, q);
  }
  zero_after = __shfl_down(zero_after, 1, 64); if (lane == 63) zero_after = IDX_NONE;
  zero_after = min(zero_after, L);
  // exclusive prefix counts of raw starts and of upward crossings
  const int my_rs = __popcll(rawstart), my_up = __popcll(up);
  int rs_inc = my_rs, up_inc = my_up;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int p = __shfl_up(rs_inc, d, 64), q = __shfl_up(up_inc, d, 64);
    if (lane >= d) { rs_inc += p; up_inc += q; }
  }
  W.rawstart[lane] = rawstart; W.up[lane] = up; W.rs_before[lane] = rs_inc - my_rs; W.up_before[lane] = up_inc - my_up;
  if (lane == 63) { W.rawstart[64] = 0; W.up[64] = 0; W.rs_before[64] = rs_inc; W.up_before[64] = up_inc; }
  __syncthreads();

  // the runs that start in this chunk: end, gate
  auto run_stop = [&](int sb) {
    const u64 rem = ~closed >> sb;
    return rem ? base + sb + __builtin_ctzll(rem) : zero_after;
  };
  auto run_kept = [&](int start, int stop) {
    const int len = stop - start;
    return len >= min_len && len <= max_len && !(drop_edge && (start == 0 || stop == L));
  };
  int my_kept = 0;
  for (u64 st = cstart; st; st &= st - 1) {
    const int sb = __builtin_ctzll(st);
    my_kept += run_kept(base + sb, run_stop(sb)) ? 1 : 0;
  }
  int kept_inc = my_kept;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int p = __shfl_up(kept_inc, d, 64);
    if (lane >= d) kept_inc += p;
  }
  const int kept_total = __shfl(kept_inc, 63, 64);
  if (!live) return;
  if (lane == 0) { counts[2 * b] = kept_total; counts[2 * b + 1] = W.rs_before[64]; }
  int e = kept_inc - my_kept;
  for (u64 st = cstart; st && e < E; st &= st - 1) {
    const int sb = __builtin_ctzll(st);
    const int start = base + sb, stop = run_stop(sb);
    if (!run_kept(start, stop)) continue;
    float peak = sr[start], sum = 0.f;
    int arg = start;
    float amax = 0.f, amin = 0.f;
    if (ar) { amax = ar[start]; amin = amax; }
    for (int n = start; n < stop; n++) {
      const float v = sr[n];
      sum = sum + v;
      if (v > peak) { peak = v; arg = n; }
      if (ar) {
        const float q = ar[n];
        if (q > amax) amax = q;
        if (q < amin) amin = q;
      }
    }
    int* oi = ev_i + ((long)b * E + e) * 6;
    float* of = ev_f + ((long)b * E + e) * 4;
    oi[0] = start; oi[1] = stop - start; oi[2] = arg;
    oi[3] = ar ? count_before(W.up, W.up_before, stop) - count_before(W.up, W.up_before, start + 1) : 0;
    oi[4] = count_before(W.rawstart, W.rs_before, stop) - count_before(W.rawstart, W.rs_before, start);
    oi[5] = (start == 0 ? 1 : 0) | (stop == L ? 2 : 0);
    of[0] = peak; of[1] = sum; of[2] = amax; of[3] = amin;
    e++;
  }
}

// EEGLDM_FIR_R = 4 | 8 | 12: outputs per thread instead of the rule in eegldm_fir_same (developer switch: the result does not depend on it); EEGLDM_FIR_SEGS: at least this many segments per row
int fir_env_r() { EEG_ENV_VAR(int, r, getenv("EEGLDM_FIR_R") ? atoi(getenv("EEGLDM_FIR_R")) : 0); return r; }
int fir_env_segs() { EEG_ENV_VAR(int, n, getenv("EEGLDM_FIR_SEGS") ? atoi(getenv("EEGLDM_FIR_SEGS")) : 0); return n; }
}  // namespace

extern "C" int eegldm_fir_same(eegldm_ctx* ctx, const float* x, long ldx, const float* taps, int M, float* y, long ldy, long B, int L, int edge,
                               int mode) {
  EEG_CHECK(ctx && x && taps && y, "null argument");
  EEG_CHECK(M >= 1 && M <= FIR_MAX_M, "M %d outside [1, %d]", M, FIR_MAX_M);
  EEG_CHECK(M & 1, "M %d is even: a zero-phase filter needs a centre tap", M);
  EEG_CHECK(L >= 1 && L <= FIR_MAX_L, "L %d outside [1, %d]", L, FIR_MAX_L);
  EEG_CHECK(edge == 0 || edge == 1, "edge %d is neither 0 (zeros) nor 1 (reflect)", edge);
  EEG_CHECK(mode == 0 || mode == 1, "mode %d is neither 0 (plain) nor 1 (rms)", mode);
  EEG_CHECK(!(edge == 1 && (M - 1) / 2 > L - 1), "reflect needs (M - 1) / 2 <= L - 1, got M %d L %d", M, L);
  EEG_CHECK(B >= 0 && B <= 0x7fffffffL, "B %ld outside [0, 2^31)", B);
  EEG_CHECK(ldx >= L && ldy >= L, "row strides %ld / %ld shorter than L %d", ldx, ldy, L);
  EEG_CHECK(x != y, "in-place filtering is not supported (x == y)");
  EEG_CHECK((((uintptr_t)x | (uintptr_t)taps | (uintptr_t)y) & 3u) == 0, "float pointers must be 4-byte aligned");
  if (B == 0) return 0;
  // outputs per thread, from the measured rates (profiles/events_timing.txt; B 4096, L 3072): M = 165 runs at 60 / 54 / 47 TFLOP/s with
  // R = 4 / 8 / 12 (short filters are bound by staging and by the stores, which R = 4 spreads over three times the workgroups), M = 1101 at
  // 87 / 89 / 94.  The crossover lies somewhere between; 512 is the middle of the two measured lengths on a log scale, not a measured optimum.
  int R = fir_env_r();
  if (R != 4 && R != 8 && R != 12) R = M < 512 ? 4 : 12;
  // segments per row: as few as hold the row, more while the grid is smaller than two workgroups per CU and a segment still holds 256 outputs
  const int seg_cap = NT * R;
  int nseg = (L + seg_cap - 1) / seg_cap;
  const long want = (2L * ctx->num_cu + B - 1) / B;
  const int most = (L + 255) / 256;
  if (want > nseg) nseg = (int)(want < most ? want : most);
  if (fir_env_segs() > nseg) nseg = fir_env_segs() < (L + R - 1) / R ? fir_env_segs() : (L + R - 1) / R;
  if (nseg > 65535) nseg = 65535;
  int seg_len = (L + nseg - 1) / nseg;
  seg_len = (seg_len + R - 1) / R * R;
  nseg = (L + seg_len - 1) / seg_len;
  if (R == 4) fir_launch<4>(ctx, x, ldx, taps, M, y, ldy, B, L, seg_len, nseg, edge, mode);
  else if (R == 8) fir_launch<8>(ctx, x, ldx, taps, M, y, ldy, B, L, seg_len, nseg, edge, mode);
  else fir_launch<12>(ctx, x, ldx, taps, M, y, ldy, B, L, seg_len, nseg, edge, mode);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_threshold_events(eegldm_ctx* ctx, const float* s, long lds_, const float* aux, long ldaux, const float* thr, long B, int L,
                                       int min_len, int max_len, int merge_gap, int drop_edge, int max_events, int* counts, int* ev_i,
                                       float* ev_f) {
  EEG_CHECK(ctx && s && thr && counts && ev_i && ev_f, "null argument");
  EEG_CHECK(L >= 1 && L <= EV_MAX_L, "L %d outside [1, %d]", L, EV_MAX_L);
  EEG_CHECK(min_len >= 1, "min_len %d < 1", min_len);
  EEG_CHECK(max_len >= min_len, "max_len %d < min_len %d", max_len, min_len);
  EEG_CHECK(merge_gap >= 0, "merge_gap %d < 0", merge_gap);
  EEG_CHECK(max_events >= 1 && max_events <= EV_MAX_E, "max_events %d outside [1, %d]", max_events, EV_MAX_E);
  EEG_CHECK(lds_ >= L && (!aux || ldaux >= L), "row strides %ld / %ld shorter than L %d", lds_, ldaux, L);
  EEG_CHECK(B >= 0 && B <= 0x7fffffffL, "B %ld outside [0, 2^31)", B);
  EEG_CHECK((((uintptr_t)s | (uintptr_t)aux | (uintptr_t)thr | (uintptr_t)counts | (uintptr_t)ev_i | (uintptr_t)ev_f) & 3u) == 0,
            "pointers must be 4-byte aligned");
  if (B == 0) return 0;
  hipLaunchKernelGGL(threshold_events_kernel, dim3((unsigned)((B + EV_WAVES - 1) / EV_WAVES)), dim3(NT), 0, ctx->stream, s, lds_, aux, ldaux, thr, B,
                     L, min_len, max_len, merge_gap, drop_edge ? 1 : 0, max_events, counts, ev_i, ev_f);
  LAUNCH_CHECK();
  return 0;
}
