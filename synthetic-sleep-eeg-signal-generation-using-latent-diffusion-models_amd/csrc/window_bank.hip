// Device-resident window bank (include/eegldm.h): every recording of a loader in one flat fp32 buffer, normalised in place over ragged rows
// (eegldm_bank_normalise) and cropped, padded and labelled into training batches by one launch (eegldm_window_batch).  HBM-bound passes, one
// writer per element, no atomics, no memset.
//
// Rows start at any 4-byte offset, so every kernel splits the range it owns by the ADDRESS: 0..3 scalar elements up to the next 16-byte
// line, the float4 body, a scalar tail.  Indices into the bank are 64-bit throughout (a bank may pass 2^31 elements).
//
// The normalisation is three launches over fixed BANK_CHUNK-sample chunks of a row -- min / max partial per chunk, one fold per row, apply --
// so no value depends on the grid.  Chunk c of row r writes its partial to slot row_off[r] / BANK_CHUNK + r + c: rows are disjoint and
// ascending, so floor(row_off[r + 1] / CH) + r + 1 >= floor(row_off[r] / CH) + r + ceil(len_r / CH) and no two chunks share a slot; the
// slots of a bank of n elements number at most n / BANK_CHUNK + n_rec + 1.  No table of chunks is needed.
#include "elementwise.h"

namespace {
constexpr int BANK_CHUNK = EEGLDM_BANK_CHUNK;      // samples per min / max partial: 64 per thread, 16 float4 loads in flight
constexpr long BANK_MAX_ROW = 1L << 30;

// x * fl32(1 + 1e6), rounded on its own.  The build contracts a * c - lo into an fma (-ffp-contract=fast), and this toolchain's __fmul_rn /
// __fsub_rn are the plain operators (the separately rounded OCML forms are compiled out), so the contraction is switched off at the source:
// operations formed under `fp contract(off)` carry no contract flag and stay unfused wherever they are inlined.
__device__ __forceinline__ float scaled(float x) {
#pragma clang fp contract(off)
  return x * 1000001.0f;
}

struct MinMax { float lo, hi; bool nan; };
__device__ __forceinline__ void mm_take(MinMax& m, float a) {      // fminf / fmaxf drop a NaN: numpy's min / max keep it
  m.nan |= a != a; m.lo = fminf(m.lo, a); m.hi = fmaxf(m.hi, a);
}
// block-wide fold; the result is valid in thread 0
__device__ __forceinline__ MinMax mm_block(MinMax m) {
  __shared__ float s_lo[NT / 64], s_hi[NT / 64]; __shared__ int s_nan[NT / 64];
  int nan = m.nan;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m.lo = fminf(m.lo, __shfl_xor(m.lo, o, 64)); m.hi = fmaxf(m.hi, __shfl_xor(m.hi, o, 64)); nan |= __shfl_xor(nan, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_lo[w] = m.lo; s_hi[w] = m.hi; s_nan[w] = nan; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < NT / 64; k++) { m.lo = fminf(m.lo, s_lo[k]); m.hi = fmaxf(m.hi, s_hi[k]); nan |= s_nan[k]; }
  }
  m.nan = nan != 0;
  return m;
}

// the scalar head / float4 body / scalar tail of `len` floats at p
__device__ __forceinline__ VecSplit addr_split(const float* p, long len) {
  long head = (long)((4 - (int)(((uintptr_t)p >> 2) & 3)) & 3);
  if (head > len) head = len;
  return vec_split(len, head);
}

// chunk blockIdx.x of every row blockIdx.y, blockIdx.y + gridDim.y, ...: which rows a block visits depends on the grid, what is computed
// for a chunk does not
__global__ __launch_bounds__(NT) void bank_minmax_kernel(const float* __restrict__ bank, const int64_t* __restrict__ row_off, int n_rec,
                                                         float* __restrict__ part) {
  for (int r = blockIdx.y; r < n_rec; r += gridDim.y) {
    const int64_t r0 = row_off[r], len_r = row_off[r + 1] - r0, c0 = (int64_t)blockIdx.x * BANK_CHUNK;
    if (c0 >= len_r) continue;      // (uniform over the block)
    const long len = len_r - c0 < BANK_CHUNK ? (long)(len_r - c0) : (long)BANK_CHUNK;
    const float* p = bank + r0 + c0;
    const VecSplit s = addr_split(p, len);
    MinMax m{__builtin_inff(), -__builtin_inff(), false};
    for (long i = threadIdx.x; i < s.n4; i += NT) {
      const f32x4 v = ((const f32x4*)(p + s.head))[i];
#pragma unroll
      for (int k = 0; k < 4; k++) mm_take(m, scaled(v[k]));
    }
    for (long j = threadIdx.x; j < s.nedge; j += NT) mm_take(m, scaled(p[EDGE_INDEX(s, j)]));
    m = mm_block(m);
    if (threadIdx.x == 0) {
      const int64_t slot = r0 / BANK_CHUNK + r + blockIdx.x;
      const float qnan = __builtin_nanf("");
      part[2 * slot] = m.nan ? qnan : m.lo; part[2 * slot + 1] = m.nan ? qnan : m.hi;
    }
    __syncthreads();      // mm_block's LDS is reused by the next row
  }
}

// one block per row: lohi[r] = fold of the row's partials (min and max are exact: any order gives the same value)
__global__ __launch_bounds__(NT) void bank_fold_kernel(const int64_t* __restrict__ row_off, int n_rec, const float* __restrict__ part,
                                                       float* __restrict__ lohi) {
  for (int r = blockIdx.x; r < n_rec; r += gridDim.x) {
    const int64_t r0 = row_off[r], len_r = row_off[r + 1] - r0, nc = (len_r + BANK_CHUNK - 1) / BANK_CHUNK, slot0 = r0 / BANK_CHUNK + r;
    MinMax m{__builtin_inff(), -__builtin_inff(), false};
    for (int64_t c = threadIdx.x; c < nc; c += NT) {
      const float lo = part[2 * (slot0 + c)], hi = part[2 * (slot0 + c) + 1];
      m.nan |= lo != lo; m.lo = fminf(m.lo, lo); m.hi = fmaxf(m.hi, hi);
    }
    m = mm_block(m);
    if (threadIdx.x == 0) {
      const float qnan = __builtin_nanf("");
      lohi[2 * r] = m.nan ? qnan : m.lo; lohi[2 * r + 1] = m.nan ? qnan : m.hi;
    }
    __syncthreads();
  }
}

// (a - lo) / (hi - lo), three separately rounded operations (the division is the IEEE one: HIP's default); hi == lo -> +0
__device__ __forceinline__ float normalised(float x, float lo, float span, bool flat) {
#pragma clang fp contract(off)
  const float a = scaled(x);
  const float d = a - lo;
  return flat ? 0.0f : d / span;
}
__global__ __launch_bounds__(NT) void bank_apply_kernel(float* __restrict__ bank, const int64_t* __restrict__ row_off, int n_rec,
                                                        const float* __restrict__ lohi) {
  for (int r = blockIdx.y; r < n_rec; r += gridDim.y) {
    const int64_t r0 = row_off[r], len_r = row_off[r + 1] - r0, c0 = (int64_t)blockIdx.x * BANK_CHUNK;
    if (c0 >= len_r) continue;
    const long len = len_r - c0 < BANK_CHUNK ? (long)(len_r - c0) : (long)BANK_CHUNK;
    const float lo = lohi[2 * r], hi = lohi[2 * r + 1], span = hi - lo;
    const bool flat = hi == lo;      // (false for a NaN row: the arithmetic below then gives NaN everywhere, as numpy's does)
    float* p = bank + r0 + c0;
    const VecSplit s = addr_split(p, len);
    for (long i = threadIdx.x; i < s.n4; i += NT) {
      f32x4 v = ((const f32x4*)(p + s.head))[i];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = normalised(v[k], lo, span, flat);
      ((f32x4*)(p + s.head))[i] = v;
    }
    for (long j = threadIdx.x; j < s.nedge; j += NT) { const long e = EDGE_INDEX(s, j); p[e] = normalised(p[e], lo, span, flat); }
  }
}

// ------------------------------------------------------------------ eegldm_window_batch
struct BatchArgs {
  const float* bank; int64_t bank_len;
  const int64_t* seg_first; const int64_t* seg_cum; const int32_t* seg_label; int64_t n_seg;
  const int64_t* group_bounds; int n_group; const int64_t* group; const int64_t* idx_in;
  unsigned long long seed, offset;
  int window, border; float* out; int64_t ld; int64_t* labels_out; int64_t* src_out;
};

// One block per window.  Every thread of the block forms the same idx / segment / src (uniform loads, one Philox call), then the block
// writes the row of W = window + 2 border floats: position p holds +0 in the borders and bank[src + p - border] between them.
__global__ __launch_bounds__(NT) void window_batch_kernel(BatchArgs a) {
  const int64_t b = blockIdx.x;
  const int W = a.window + 2 * a.border;
  float* row = a.out + b * a.ld;

  // 1. the cumulative range of the window's group
  int64_t lo = 0, hi = a.seg_cum[a.n_seg];
  if (a.group) {
    const int64_t g = a.group[b];
    if (g < 0 || g >= a.n_group) { lo = 0; hi = 0; }
    else {
      const int64_t s0 = a.group_bounds[g], s1 = a.group_bounds[g + 1];
      if (s0 < 0 || s1 > a.n_seg || s0 > s1) { lo = 0; hi = 0; } else { lo = a.seg_cum[s0]; hi = a.seg_cum[s1]; }
    }
  }
  // 2. / 3. the index: given, or the value eegldm_randint(high = hi - lo, seed, offset) writes to element b, shifted by lo
  bool ok = hi > lo;
  int64_t idx = 0;
  if (ok) {
    if (a.idx_in) { idx = a.idx_in[b]; ok = idx >= lo && idx < hi; }
    else {
      unsigned w[4]; philox(a.seed, a.offset + (unsigned long long)b, w);
      const unsigned long long v = ((unsigned long long)w[0] << 32) | w[1];
      idx = lo + (int64_t)(v % (unsigned long long)(hi - lo));
    }
  }
  // 4. / 5. the segment j with seg_cum[j] <= idx < seg_cum[j + 1] (runs are never empty, so it is unique)
  int64_t src = -1; int32_t lab = 0;
  if (ok) {
    int64_t j0 = 0, j1 = a.n_seg;      // answer in [j0, j1)
    while (j1 - j0 > 1) { const int64_t mid = j0 + ((j1 - j0) >> 1); if (a.seg_cum[mid] <= idx) j0 = mid; else j1 = mid; }
    src = a.seg_first[j0] + (idx - a.seg_cum[j0]); lab = a.seg_label[j0];
    ok = src >= 0 && src + a.window <= a.bank_len;      // a table that points outside the bank reads nothing
  }
  if (threadIdx.x == 0) {
    if (a.labels_out) a.labels_out[b] = ok ? (int64_t)lab : INT64_MIN;
    if (a.src_out) a.src_out[b] = ok ? src : -1;
  }
  // 6. the row.  16-byte stores when the row starts on a 16-byte line; a group of four takes one 16-byte load when it lies inside the
  // window and its source does too, else its elements one by one (no read outside [src, src + window)).
  const float qnan = __builtin_nanf("");
  const float* sp = a.bank + (ok ? src : 0) - a.border;      // sp[p] is position p's source (dereferenced between the borders only)
  const int in0 = a.border, in1 = a.border + a.window;
  const bool vec = (((uintptr_t)row) & 15) == 0;
  const int n4 = vec ? W >> 2 : 0;
  for (int i = threadIdx.x; i < n4; i += NT) {
    const int p = 4 * i;
    f32x4 v;
    if (!ok) { v[0] = qnan; v[1] = qnan; v[2] = qnan; v[3] = qnan; }
    else if (p >= in0 && p + 4 <= in1 && (((uintptr_t)(sp + p)) & 15) == 0) v = *(const f32x4*)(sp + p);
    else {
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = (p + k >= in0 && p + k < in1) ? sp[p + k] : 0.0f;
    }
    *(f32x4*)(row + p) = v;
  }
  for (int p = 4 * n4 + threadIdx.x; p < W; p += NT) row[p] = !ok ? qnan : (p >= in0 && p < in1) ? sp[p] : 0.0f;
}
}  // namespace

extern "C" int eegldm_bank_normalise(eegldm_ctx* ctx, float* bank, const int64_t* row_off, const int64_t* row_off_host, int n_rec, float* lohi,
                                     float* ws, long ws_floats) {
  EEG_CHECK(ctx && bank && row_off && row_off_host && lohi && ws, "null argument");
  EEG_CHECK(n_rec >= 1, "n_rec (%d) must be >= 1", n_rec);
  EEG_CHECK(((uintptr_t)bank & 3) == 0 && ((uintptr_t)lohi & 3) == 0 && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)row_off & 7) == 0,
            "float buffers must be 4-byte aligned, row_off 8-byte aligned");
  EEG_CHECK(row_off_host[0] >= 0, "row_off[0] = %lld is negative", (long long)row_off_host[0]);
  int64_t longest = 0;
  for (int r = 0; r < n_rec; r++) {
    const int64_t len = row_off_host[r + 1] - row_off_host[r];
    EEG_CHECK(len >= 1 && len <= BANK_MAX_ROW, "row %d has %lld samples: need 1 .. 2^30", r, (long long)len);
    if (len > longest) longest = len;
  }
  const int64_t slots = row_off_host[n_rec] / BANK_CHUNK + n_rec + 1;
  EEG_CHECK((int64_t)ws_floats >= 2 * slots, "workspace of %ld floats, need %lld (2 * (row_off[n_rec] / %d + n_rec + 1))", ws_floats,
            (long long)(2 * slots), BANK_CHUNK);
  const unsigned nchunk = (unsigned)((longest + BANK_CHUNK - 1) / BANK_CHUNK), ny = (unsigned)(n_rec < 65535 ? n_rec : 65535);
  hipLaunchKernelGGL(bank_minmax_kernel, dim3(nchunk, ny), dim3(NT), 0, ctx->stream, (const float*)bank, row_off, n_rec, ws);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(bank_fold_kernel, dim3((unsigned)n_rec), dim3(NT), 0, ctx->stream, row_off, n_rec, (const float*)ws, lohi);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(bank_apply_kernel, dim3(nchunk, ny), dim3(NT), 0, ctx->stream, bank, row_off, n_rec, (const float*)lohi);
  LAUNCH_CHECK(); return 0;
}

extern "C" int eegldm_window_batch(eegldm_ctx* ctx, const float* bank, long bank_len, const int64_t* seg_first, const int64_t* seg_cum,
                                   const int32_t* seg_label, long n_seg, const int64_t* group_bounds, int n_group, const int64_t* group,
                                   const int64_t* idx_in, uint64_t seed, uint64_t offset, int window, int border, float* out, long ld,
                                   int64_t* labels_out, int64_t* src_out, int B) {
  EEG_CHECK(ctx && bank && seg_first && seg_cum && seg_label && out, "null argument");
  EEG_CHECK(!group || group_bounds, "group needs group_bounds");
  EEG_CHECK(window >= 1, "window (%d) must be >= 1", window);
  EEG_CHECK(border >= 0, "border (%d) must be >= 0", border);
  EEG_CHECK((long)window + 2L * border <= 0x7fffffffL, "window + 2 border overflows");
  EEG_CHECK(ld >= (long)window + 2L * border, "ld (%ld) is smaller than window + 2 border = %ld", ld, (long)window + 2L * border);
  EEG_CHECK(B >= 1, "B (%d) must be >= 1", B);
  EEG_CHECK(n_seg >= 1 && bank_len >= window, "n_seg (%ld) must be >= 1 and bank_len (%ld) >= window", n_seg, bank_len);
  EEG_CHECK(!group || n_group >= 1, "n_group (%d) must be >= 1", n_group);
  EEG_CHECK(((uintptr_t)bank & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)seg_label & 3) == 0, "float and int32 buffers must be 4-byte aligned");
  for (const void* q : {(const void*)seg_first, (const void*)seg_cum, (const void*)group_bounds, (const void*)group, (const void*)idx_in,
                        (const void*)labels_out, (const void*)src_out})
    EEG_CHECK(((uintptr_t)q & 7) == 0, "int64 buffers must be 8-byte aligned");
  BatchArgs a{bank, (int64_t)bank_len, seg_first, seg_cum, seg_label, (int64_t)n_seg, group_bounds, group ? n_group : 0, group, idx_in,
              seed, offset, window, border, out, (int64_t)ld, labels_out, src_out};
  hipLaunchKernelGGL(window_batch_kernel, dim3((unsigned)B), dim3(NT), 0, ctx->stream, a);
  LAUNCH_CHECK(); return 0;
}
