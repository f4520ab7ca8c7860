// k nearest neighbours of Nq query rows in a corpus streamed in chunks (memorisation audit, precision / recall / coverage):
//   score s(i, j) = xbias[j] - 2 <q_i, x_j>, smaller is nearer; the Nq x Nc score matrix never exists.
//   * knn_tile_kernel: a workgroup owns 128 queries and one slab of the chunk and walks the slab in 128-row corpus tiles.  The dot
//     products run on the f32-input MFMA (32x32x2: an exact fmaf chain in ascending k starting from 0, so the value of a pair depends on
//     the two rows alone, not on tile, slab or chunk position); operands go global -> registers -> LDS (k-major, zero-filled K tail and
//     zero rows past the edges), the next K tile's loads are in flight during the MFMAs.  The tile's scores go to LDS (over the operand
//     tiles), then every thread owns (one query row, one 64-column half) and keeps a k-list sorted by (score, index) in LDS behind a
//     threshold compare.  At the end of the slab the lists are written to the workspace [Nq][2 * slabs][k]: one writer per element.
//   * knn_merge_kernel: one wave per query folds the slab lists and the caller's running state in (score, index) order.
// No atomics, no memset: the result is a pure function of the set of (score, index) pairs, so it repeats bit for bit and does not
// depend on how the corpus is chunked.
// Helpers: fixed-order row sums of squares, row standardisation (zero mean, unit L2 norm), and the direct-form distance of the winners.
#include "common.h"

namespace {
typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int TM = 128, TN = 128, KT = 16, NT = 256;
constexpr int LDT = 132;             // row stride of the k-major operand tiles
constexpr int SLD = 129;             // row stride of the score tile
constexpr int SCORE_FLOATS = TM * SLD;
constexpr int MAX_K = 32, MAX_SLABS = 32;
static_assert(2 * KT * LDT <= SCORE_FLOATS, "the operand tiles live inside the score tile's area");

__global__ __launch_bounds__(NT) void knn_tile_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ x, long ldx,
                                                      const float* __restrict__ xbias, int Nq, int Nc, int D, int k, long index_base,
                                                      long self_base, int tiles_per_slab, int nlists, float* __restrict__ ws_s,
                                                      int* __restrict__ ws_i) {
  extern __shared__ float sm[];
  float* sA = sm;                                   // [KT][LDT] queries, k-major
  float* sB = sm + KT * LDT;                        // [KT][LDT] corpus rows, k-major
  float* S = sm;                                    // [TM][SLD] scores (after the K loop)
  float* ls = sm + SCORE_FLOATS;                    // [k][NT] list scores
  int* li = (int*)(ls + (size_t)k * NT);            // [k][NT] list indices (row within the chunk, -1 = empty)

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int q0 = blockIdx.x * TM;
  const int slab = blockIdx.y;
  const int ctiles = (Nc + TN - 1) / TN;
  const int tile_lo = slab * tiles_per_slab;
  const int tile_hi = min(ctiles, tile_lo + tiles_per_slab);
  const int nkt = (D + KT - 1) / KT;

  // staging map: thread -> (k offset lk, rows lr + 16 j)
  const int lk = t & (KT - 1), lr = t >> 4;
  // selection map: thread -> (query row sr, column half sh)
  const int sr = t & (TM - 1), sh = t >> 7;
  const int gi = q0 + sr;
  const long self_j = (self_base >= 0 && gi < Nq) ? self_base + gi - index_base : -1;      // the chunk row that is query gi itself

  for (int p = 0; p < k; p++) { ls[p * NT + t] = INFINITY; li[p * NT + t] = -1; }
  float thr = INFINITY;

  for (int tile = tile_lo; tile < tile_hi; tile++) {
    const int c0 = tile * TN;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

    float ra[8], rb[8];
    auto load_regs = [&](int k0) {
      const int kk = k0 + lk;
      const bool kin = kk < D;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int qi = q0 + lr + 16 * j, xi = c0 + lr + 16 * j;
        ra[j] = (kin && qi < Nq) ? q[(long)qi * ldq + kk] : 0.f;
        rb[j] = (kin && xi < Nc) ? x[(long)xi * ldx + kk] : 0.f;
      }
    };
    load_regs(0);
    for (int kt = 0; kt < nkt; kt++) {
      __syncthreads();                    // the previous K tile's reads (first K tile: the previous corpus tile's selection) are done
#pragma unroll
      for (int j = 0; j < 8; j++) { sA[lk * LDT + lr + 16 * j] = ra[j]; sB[lk * LDT + lr + 16 * j] = rb[j]; }
      __syncthreads();
      if (kt + 1 < nkt) load_regs((kt + 1) * KT);
#pragma unroll
      for (int k2 = 0; k2 < KT / 2; k2++) {
        const int kk = 2 * k2 + (lane >> 5);
        float a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; m++) {
          a[m] = sA[kk * LDT + wm * 64 + m * 32 + (lane & 31)];
          b[m] = sB[kk * LDT + wn * 64 + m * 32 + (lane & 31)];
        }
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
          for (int n = 0; n < 2; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[n], acc[m][n], 0, 0, 0);
      }
    }
    __syncthreads();                      // every wave has read its last operands: the area becomes the score tile
#pragma unroll
    for (int n = 0; n < 2; n++) {
      const int col = wn * 64 + n * 32 + (lane & 31);
      const float xb = (xbias != nullptr && c0 + col < Nc) ? xbias[c0 + col] : 0.f;
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          S[row * SLD + col] = fmaf(-2.0f, acc[m][n][r], xb);
        }
    }
    __syncthreads();
    if (gi < Nq) {
      const int cbase = c0 + sh * 64;
      const int ncols = min(64, Nc - cbase);
      for (int c = 0; c < ncols; c++) {
        const float s = S[sr * SLD + sh * 64 + c];
        if (s < thr) {                    // a NaN fails; candidates arrive in ascending index order, so a tie with the k-th loses
          const int j = cbase + c;
          if ((long)j == self_j) continue;
          int p = k - 1;
          while (p > 0 && ls[(p - 1) * NT + t] > s) {
            ls[p * NT + t] = ls[(p - 1) * NT + t]; li[p * NT + t] = li[(p - 1) * NT + t];
            p--;
          }
          ls[p * NT + t] = s; li[p * NT + t] = j;
          thr = ls[(k - 1) * NT + t];
        }
      }
    }
  }
  if (gi < Nq) {
    const size_t o = ((size_t)gi * nlists + (size_t)slab * 2 + sh) * k;
    for (int p = 0; p < k; p++) { ws_s[o + p] = ls[p * NT + t]; ws_i[o + p] = li[p * NT + t]; }
  }
}

__device__ __forceinline__ bool pair_less(float as, long long ai, float bs, long long bi) {
  return as < bs || (as == bs && (unsigned long long)ai < (unsigned long long)bi);      // index -1 (empty) sorts last
}

// one wave per query: lists 0 .. nlists-1 are the slab lists, list nlists is the running state; lane l owns lists l and l + 64
__global__ __launch_bounds__(64) void knn_merge_kernel(const float* __restrict__ ws_s, const int* __restrict__ ws_i, int nlists, int k,
                                                       long index_base, float* __restrict__ best_s, long long* __restrict__ best_i) {
  __shared__ float st_s[MAX_K];
  __shared__ long long st_i[MAX_K];
  const int lane = threadIdx.x;
  const size_t qi = blockIdx.x;
  if (lane < k) { st_s[lane] = best_s[qi * k + lane]; st_i[lane] = best_i[qi * k + lane]; }
  __syncthreads();
  auto head = [&](int l, int p, float& s, long long& i) {
    s = INFINITY; i = -1;
    if (l > nlists || p >= k) return;
    if (l == nlists) { s = st_s[p]; i = st_i[p]; return; }
    const size_t o = (qi * nlists + l) * k + p;
    const int j = ws_i[o];
    if (j >= 0) { s = ws_s[o]; i = (long long)index_base + j; }
  };
  int p0 = 0, p1 = 0;
  float s0, s1; long long i0, i1;
  head(lane, 0, s0, i0); head(lane + 64, 0, s1, i1);
  for (int r = 0; r < k; r++) {
    float bs = s0; long long bi = i0;
    if (pair_less(s1, i1, bs, bi)) { bs = s1; bi = i1; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const long long oi = __shfl_xor(bi, o, 64);
      if (pair_less(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    if (lane == 0) { best_s[qi * k + r] = bi < 0 ? INFINITY : bs; best_i[qi * k + r] = bi; }
    if (bi >= 0) {
      if (i0 == bi) head(lane, ++p0, s0, i0);
      if (i1 == bi) head(lane + 64, ++p1, s1, i1);
    }
  }
}

// ---- helpers: one wave per row; lane l chains elements l, l + 64, ... in ascending order, then a fixed butterfly
__global__ __launch_bounds__(NT) void rows_sqnorm_kernel(const float* __restrict__ x, long ldx, long N, int D, float* __restrict__ out) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * ldx;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) s = fmaf(xr[i], xr[i], s);
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

__global__ __launch_bounds__(NT) void rows_standardize_kernel(const float* __restrict__ x, long ldx, long N, int D, float* __restrict__ out,
                                                              long ldout) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * ldx;
  float* orow = out + row * ldout;
  float s = 0.f, lo = INFINITY, hi = -INFINITY;
  for (int i = lane; i < D; i += 64) { const float v = xr[i]; s += v; lo = fminf(lo, v); hi = fmaxf(hi, v); }
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
  const float mean = s / (float)D;
  float ss = 0.f;
  for (int i = lane; i < D; i += 64) { const float d = xr[i] - mean; ss = fmaf(d, d, ss); }
  ss = wave_sum(ss);
  const float nrm = sqrtf(ss);
  const bool flat = lo == hi || !(nrm > 0.f);          // a constant row: its rounded mean need not equal its value
  for (int i = lane; i < D; i += 64) orow[i] = flat ? 0.f : (xr[i] - mean) / nrm;
}

// one wave per (query, list slot): out_d2 = sum (q - x)^2 for the winners whose index lies in [index_base, index_base + Nc)
__global__ __launch_bounds__(NT) void knn_rescore_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ x, long ldx, long slots,
                                                         int D, int k, long index_base, long Nc, const long long* __restrict__ best_i,
                                                         float* __restrict__ out_d2) {
  const long slot = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= slots) return;
  const long long j = best_i[slot] - index_base;
  if (best_i[slot] < 0 || j < 0 || j >= Nc) return;
  const int lane = threadIdx.x & 63;
  const float* qr = q + (slot / k) * ldq;
  const float* xr = x + j * ldx;
  float s = 0.f;
  for (int i = lane; i < D; i += 64) { const float d = qr[i] - xr[i]; s = fmaf(d, d, s); }
  s = wave_sum(s);
  if (lane == 0) out_d2[slot] = s;
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
}  // namespace

extern "C" int eegldm_knn_update(eegldm_ctx* ctx, const float* q, long ldq, const float* x, long ldx, const float* xbias, int Nq, int Nc, int D,
                                 int k, long index_base, long self_base, float* best_s, int64_t* best_i) {
  EEG_CHECK(ctx && q && x && best_s && best_i, "null argument");
  EEG_CHECK(Nq >= 1 && Nc >= 0 && D >= 1, "bad sizes Nq %d Nc %d D %d", Nq, Nc, D);
  EEG_CHECK(k >= 1 && k <= MAX_K, "k %d outside [1, %d]", k, MAX_K);
  EEG_CHECK(ldq >= D && ldx >= D, "row strides %ld / %ld shorter than D %d", ldq, ldx, D);
  EEG_CHECK(index_base >= 0, "negative index_base");
  EEG_CHECK(aligned4(q) && aligned4(x) && aligned4(xbias) && aligned4(best_s), "pointers must be 4-byte aligned");
  EEG_CHECK(((uintptr_t)best_i & 7u) == 0, "best_i must be 8-byte aligned");
  if (Nc == 0) return 0;
  const int qtiles = (Nq + TM - 1) / TM, ctiles = (Nc + TN - 1) / TN;
  int want = (2 * ctx->num_cu + qtiles - 1) / qtiles;
  want = want < 1 ? 1 : want; want = want > ctiles ? ctiles : want; want = want > MAX_SLABS ? MAX_SLABS : want;
  const int tps = (ctiles + want - 1) / want;
  const int nslab = (ctiles + tps - 1) / tps;
  const int nlists = 2 * nslab;
  const size_t entries = (size_t)Nq * nlists * k;
  const size_t need = entries * (sizeof(float) + sizeof(int));
  if (ctx->splitk_ws_bytes < need) {
    if (ctx->splitk_ws) { HIP_TRY(hipStreamSynchronize(ctx->stream)); if (ctx->side_on) HIP_TRY(hipStreamSynchronize(ctx->side)); HIP_TRY(hipFree(ctx->splitk_ws)); ctx->splitk_ws = nullptr; ctx->splitk_ws_bytes = 0; }
    HIP_TRY(hipMalloc(&ctx->splitk_ws, need)); ctx->splitk_ws_bytes = need;
  }
  float* ws_s = (float*)ctx->splitk_ws;
  int* ws_i = (int*)(ws_s + entries);
  const size_t lds = sizeof(float) * SCORE_FLOATS + (size_t)k * NT * (sizeof(float) + sizeof(int));
  static DevOnce once;
  if (once.need(ctx->device))
    HIP_TRY(hipFuncSetAttribute((const void*)knn_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(sizeof(float) * SCORE_FLOATS + (size_t)MAX_K * NT * (sizeof(float) + sizeof(int)))));
  hipLaunchKernelGGL(knn_tile_kernel, dim3(qtiles, nslab), dim3(NT), lds, ctx->stream, q, ldq, x, ldx, xbias, Nq, Nc, D, k, index_base, self_base,
                     tps, nlists, ws_s, ws_i);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_merge_kernel, dim3(Nq), dim3(64), 0, ctx->stream, (const float*)ws_s, (const int*)ws_i, nlists, k, index_base, best_s,
                     (long long*)best_i);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_rows_sqnorm(eegldm_ctx* ctx, const float* x, long ldx, long N, int D, float* out) {
  EEG_CHECK(ctx && x && out, "null argument");
  EEG_CHECK(N >= 0 && D >= 1 && ldx >= D, "bad sizes N %ld D %d ldx %ld", N, D, ldx);
  EEG_CHECK(aligned4(x) && aligned4(out), "pointers must be 4-byte aligned");
  if (N == 0) return 0;
  hipLaunchKernelGGL(rows_sqnorm_kernel, dim3((unsigned)((N + 3) / 4)), dim3(NT), 0, ctx->stream, x, ldx, N, D, out);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_rows_standardize(eegldm_ctx* ctx, const float* x, long ldx, long N, int D, float* out, long ldout) {
  EEG_CHECK(ctx && x && out, "null argument");
  EEG_CHECK(N >= 0 && D >= 1 && ldx >= D && ldout >= D, "bad sizes N %ld D %d ldx %ld ldout %ld", N, D, ldx, ldout);
  EEG_CHECK(aligned4(x) && aligned4(out), "pointers must be 4-byte aligned");
  if (N == 0) return 0;
  hipLaunchKernelGGL(rows_standardize_kernel, dim3((unsigned)((N + 3) / 4)), dim3(NT), 0, ctx->stream, x, ldx, N, D, out, ldout);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_knn_rescore(eegldm_ctx* ctx, const float* q, long ldq, const float* x, long ldx, int Nq, int D, int k, long index_base,
                                  long Nc, const int64_t* best_i, float* out_d2) {
  EEG_CHECK(ctx && q && x && best_i && out_d2, "null argument");
  EEG_CHECK(Nq >= 1 && Nc >= 0 && D >= 1 && ldq >= D && ldx >= D, "bad sizes Nq %d Nc %ld D %d", Nq, Nc, D);
  EEG_CHECK(k >= 1 && k <= MAX_K, "k %d outside [1, %d]", k, MAX_K);
  EEG_CHECK(aligned4(q) && aligned4(x) && aligned4(out_d2) && ((uintptr_t)best_i & 7u) == 0, "misaligned pointer");
  if (Nc == 0) return 0;
  const long slots = (long)Nq * k;
  hipLaunchKernelGGL(knn_rescore_kernel, dim3((unsigned)((slots + 3) / 4)), dim3(NT), 0, ctx->stream, q, ldq, x, ldx, slots, D, k, index_base, Nc,
                     (const long long*)best_i, out_d2);
  LAUNCH_CHECK();
  return 0;
}
