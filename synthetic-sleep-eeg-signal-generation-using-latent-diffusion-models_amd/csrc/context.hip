// Context conditioning (include/eegldm.h): the random keep-masks of training, the train step's noised sample and context in ONE launch, and
// the masked window the context encode starts from.  HBM-bound, one pass over the data each, one writer per element, no atomics, no memset.
//
// All three kernels walk ROW CHUNKS: a block owns CX_CHUNK consecutive positions of one sample and visits every channel row of that sample
// there, one float4 per thread and row.  The buffers of one call have different row counts per sample (C signal rows, C + 1 context rows, one
// mask row), so for L % 4 != 0 their rows start at different offsets inside a 16-byte line: the scalar head of the 16-byte body is therefore
// chosen per row chunk from the addresses themselves -- equal offsets: 0..3 scalar elements, the float4 body, a scalar tail; else the
// whole chunk goes one by one.  Any 4-byte alignment of any buffer is therefore fine.
#include "elementwise.h"
#include "internal.h"

namespace {
constexpr int CX_CHUNK = 4 * NT;

// The draw of one sample's mask (include/eegldm.h): the positions [r0, r1) are regenerated (mask 0), the rest kept (mask 1).
struct MaskDraw { unsigned long long seed, offset; float p_none, p_sum; int span_min, span_max; };
__device__ __forceinline__ void context_draw(const MaskDraw& d, long b, int L, int& r0, int& r1) {
  unsigned w[4]; philox(d.seed, d.offset + (unsigned long long)b, w);
  const float u0 = (float)w[0] * 2.3283064365386963e-10f;      // compared as label_dropout_kernel compares its word
  if (u0 < d.p_none) { r0 = 0; r1 = L; }                      // no context at all
  else if (u0 < d.p_sum) {                                     // continuation: keep [0, s)
    r0 = L > 1 ? 1 + (int)(((unsigned long long)w[1] * (unsigned)(L - 1)) >> 32) : 0; r1 = L;
  } else {                                                     // one span
    const int len = d.span_min + (int)(((unsigned long long)w[1] * (unsigned)(d.span_max - d.span_min + 1)) >> 32);
    r0 = (int)(((unsigned long long)w[2] * (unsigned)(L - len + 1)) >> 32); r1 = r0 + len;
  }
}
__device__ __forceinline__ float keep_at(int l, int r0, int r1) { return (l >= r0 && l < r1) ? 0.0f : 1.0f; }

// offset of a pointer inside its 16-byte line, in floats; a null pointer matches anything
__device__ __forceinline__ bool same_line(const void* p, int mis) { return !p || (int)(((uintptr_t)p >> 2) & 3) == mis; }
__device__ __forceinline__ VecSplit chunk_split(int len, const void* p0, const void* p1, const void* p2 = nullptr, const void* p3 = nullptr,
                                                const void* p4 = nullptr, const void* p5 = nullptr) {
  const int mis = (int)(((uintptr_t)p0 >> 2) & 3);
  const bool same = same_line(p1, mis) && same_line(p2, mis) && same_line(p3, mis) && same_line(p4, mis) && same_line(p5, mis);
  long head = same ? (long)((4 - mis) & 3) : (long)len;
  if (head > len) head = len;
  return vec_split(len, head);
}

// The mask row of one chunk: m from the buffer (DRAW false) or from the interval, written to o0 and (nullable) o1.
template <bool DRAW>
__device__ __forceinline__ void mask_row(const float* __restrict__ mp, int p0, int len, int r0, int r1, float* __restrict__ o0, float* __restrict__ o1) {
  const VecSplit s = chunk_split(len, o0, o1, DRAW ? nullptr : mp);
  const int i = threadIdx.x;
  if (i < s.n4) {
    f32x4 mv;
    if (DRAW) {
#pragma unroll
      for (int k = 0; k < 4; k++) mv[k] = keep_at(p0 + (int)s.head + 4 * i + k, r0, r1);
    } else mv = ((const f32x4*)(mp + s.head))[i];
    ((f32x4*)(o0 + s.head))[i] = mv;
    if (o1) ((f32x4*)(o1 + s.head))[i] = mv;
  }
  for (long j = i; j < s.nedge; j += NT) {      // (up to the whole chunk when the row's buffers do not share a 16-byte offset)
    const long e = EDGE_INDEX(s, j);
    const float m = DRAW ? keep_at(p0 + (int)e, r0, r1) : mp[e];
    o0[e] = m;
    if (o1) o1[e] = m;
  }
}

__global__ __launch_bounds__(NT) void context_mask_kernel(float* __restrict__ mask, int L, int nchunk, MaskDraw d) {
  const long b = blockIdx.x / nchunk; const int p0 = (int)(blockIdx.x - b * nchunk) * CX_CHUNK;
  const int len = L - p0 < CX_CHUNK ? L - p0 : CX_CHUNK;
  int r0, r1; context_draw(d, b, L, r0, r1);
  mask_row<true>(nullptr, p0, len, r0, r1, mask + b * L + p0, nullptr);
}

// noisy = sqrt(a_t) x0 + sqrt(1 - a_t) noise (add_noise_value: the bytes of add_noise_kernel), context[:, :C] = m * src, context[:, C] = m,
// mask_out (nullable) = m.  src may be x0 itself.
template <bool DRAW>
__global__ __launch_bounds__(NT) void add_noise_context_kernel(const float* __restrict__ x0, const float* __restrict__ src, const float* __restrict__ noise,
                                                               const int64_t* __restrict__ t, const float* __restrict__ acp,
                                                               const float* __restrict__ mask, MaskDraw d, float* __restrict__ noisy,
                                                               float* __restrict__ context, float* __restrict__ mask_out, int C, int L, int nchunk) {
  const long b = blockIdx.x / nchunk; const int p0 = (int)(blockIdx.x - b * nchunk) * CX_CHUNK;
  const int len = L - p0 < CX_CHUNK ? L - p0 : CX_CHUNK;
  const float a = acp[t[b]];
  const float sa = sqrtf(a), sb = sqrtf(1.0f - a);
  int r0 = 0, r1 = 0;
  if (DRAW) context_draw(d, b, L, r0, r1);
  const float* mp = DRAW ? nullptr : mask + b * L + p0;
  const int i = threadIdx.x;
  for (int c = 0; c < C; c++) {
    const long ox = (b * C + c) * L + p0, oc = (b * (C + 1) + c) * L + p0;
    const float* xp = x0 + ox; const float* sp = src + ox; const float* zp = noise + ox;
    float* yp = noisy + ox; float* cp = context + oc;
    const VecSplit s = chunk_split(len, xp, sp, zp, yp, cp, mp);
    if (i < s.n4) {
      const f32x4 xv = ((const f32x4*)(xp + s.head))[i], zv = ((const f32x4*)(zp + s.head))[i], sv = ((const f32x4*)(sp + s.head))[i];
      f32x4 mv, yv, cv;
      if (!DRAW) mv = ((const f32x4*)(mp + s.head))[i];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (DRAW) mv[k] = keep_at(p0 + (int)s.head + 4 * i + k, r0, r1);
        yv[k] = add_noise_value(xv[k], zv[k], sa, sb);
        cv[k] = mv[k] * sv[k];
      }
      ((f32x4*)(yp + s.head))[i] = yv;
      ((f32x4*)(cp + s.head))[i] = cv;
    }
    for (long j = i; j < s.nedge; j += NT) {
      const long e = EDGE_INDEX(s, j);
      const float m = DRAW ? keep_at(p0 + (int)e, r0, r1) : mp[e];
      yp[e] = add_noise_value(xp[e], zp[e], sa, sb);
      cp[e] = m * sp[e];
    }
  }
  mask_row<DRAW>(mp, p0, len, r0, r1, context + (b * (C + 1) + C) * L + p0, mask_out ? mask_out + b * L + p0 : nullptr);
}

// out[b][c][l] = windows[b][c][l] * mask[b][l / down]: rows of Lw = L * down samples, the mask row read at latent resolution
__global__ __launch_bounds__(NT) void context_window_kernel(const float* __restrict__ win, const float* __restrict__ mask, int down,
                                                            float* __restrict__ out, int Co, int Lw, int nchunk) {
  const long row = blockIdx.x / nchunk; const int p0 = (int)(blockIdx.x - row * nchunk) * CX_CHUNK;
  const int len = Lw - p0 < CX_CHUNK ? Lw - p0 : CX_CHUNK;
  const long b = row / Co;
  const float* mrow = mask + b * (Lw / down);
  const float* wp = win + row * Lw + p0; float* op = out + row * Lw + p0;
  const VecSplit s = chunk_split(len, wp, op);
  const int i = threadIdx.x;
  if (i < s.n4) {
    f32x4 v = ((const f32x4*)(wp + s.head))[i];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = v[k] * mrow[(p0 + (int)s.head + 4 * i + k) / down];
    ((f32x4*)(op + s.head))[i] = v;
  }
  for (long j = i; j < s.nedge; j += NT) {
    const long e = EDGE_INDEX(s, j);
    op[e] = wp[e] * mrow[(p0 + (int)e) / down];
  }
}

bool ov(const float* p, long np, const float* q, long nq) { return p && q && p < q + nq && q < p + np; }

// the draw's parameters, refused before any launch
int draw_check(int L, float p_none, float p_prefix, int span_min, int span_max, uint64_t seed, uint64_t offset, MaskDraw* d) {
  EEG_CHECK(p_none >= 0.0f && p_none <= 1.0f && p_prefix >= 0.0f && p_prefix <= 1.0f, "p_none %g and p_prefix %g must lie in [0, 1]", (double)p_none,
            (double)p_prefix);
  const float p_sum = p_none + p_prefix;
  EEG_CHECK(p_sum <= 1.0f, "p_none + p_prefix = %g exceeds 1", (double)p_sum);
  EEG_CHECK(span_min >= 1 && span_max >= span_min && span_max <= L, "span [%d, %d] must satisfy 1 <= span_min <= span_max <= L = %d", span_min,
            span_max, L);
  d->seed = seed; d->offset = offset; d->p_none = p_none; d->p_sum = p_sum; d->span_min = span_min; d->span_max = span_max;
  return 0;
}
int chunks_of(int rows_outer, long rows_inner, int L, unsigned* blocks, int* nchunk) {
  const long nc = ((long)L + CX_CHUNK - 1) / CX_CHUNK, nb = (long)rows_outer * rows_inner * nc;
  EEG_CHECK(nb <= 0x7fffffffL, "%ld blocks: too many", nb);
  *blocks = (unsigned)nb; *nchunk = (int)nc;
  return 0;
}
}  // namespace

extern "C" int eegldm_context_mask(eegldm_ctx* ctx, float* mask, int B, int L, float p_none, float p_prefix, int span_min, int span_max,
                                   uint64_t seed, uint64_t offset) {
  EEG_CHECK(ctx && mask, "null argument");
  EEG_CHECK(B >= 1 && L >= 1, "B (%d) and L (%d) must be >= 1", B, L);
  EEG_CHECK(((uintptr_t)mask & 3) == 0, "buffers must be 4-byte aligned");
  MaskDraw d; EEG_TRY(draw_check(L, p_none, p_prefix, span_min, span_max, seed, offset, &d));
  unsigned blocks; int nchunk; EEG_TRY(chunks_of(B, 1, L, &blocks, &nchunk));
  hipLaunchKernelGGL(context_mask_kernel, dim3(blocks), dim3(NT), 0, ctx->stream, mask, L, nchunk, d);
  LAUNCH_CHECK(); return 0;
}

extern "C" int eegldm_add_noise_context(eegldm_ctx* ctx, const float* x0, const float* ctx_src, const float* noise, const int64_t* t,
                                        const float* acp, const float* mask, float p_none, float p_prefix, int span_min, int span_max,
                                        uint64_t seed, uint64_t offset, float* noisy, float* context, float* mask_out, int B, int C, int L) {
  EEG_CHECK(ctx && x0 && noise && t && acp && noisy && context, "null argument");
  EEG_CHECK(B >= 1 && C >= 1 && L >= 1, "B (%d), C (%d) and L (%d) must be >= 1", B, C, L);
  if (!ctx_src) ctx_src = x0;
  MaskDraw d{};
  if (!mask) EEG_TRY(draw_check(L, p_none, p_prefix, span_min, span_max, seed, offset, &d));
  for (const void* q : {(const void*)x0, (const void*)ctx_src, (const void*)noise, (const void*)mask, (const void*)noisy, (const void*)context,
                        (const void*)mask_out})
    EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
  const long n = (long)B * C * L, nc = (long)B * (C + 1) * L, nm = (long)B * L;
  const float* outs[3] = {noisy, context, mask_out}; const long on[3] = {n, nc, nm};
  for (int k = 0; k < 3; k++) {
    EEG_CHECK(!ov(outs[k], on[k], x0, n) && !ov(outs[k], on[k], ctx_src, n) && !ov(outs[k], on[k], noise, n) && !ov(outs[k], on[k], mask, nm),
              "an output aliases an input");
    for (int j = k + 1; j < 3; j++) EEG_CHECK(!ov(outs[k], on[k], outs[j], on[j]), "two outputs alias");
  }
  unsigned blocks; int nchunk; EEG_TRY(chunks_of(B, 1, L, &blocks, &nchunk));
  if (mask) hipLaunchKernelGGL((add_noise_context_kernel<false>), dim3(blocks), dim3(NT), 0, ctx->stream, x0, ctx_src, noise, t, acp, mask, d, noisy,
                               context, mask_out, C, L, nchunk);
  else hipLaunchKernelGGL((add_noise_context_kernel<true>), dim3(blocks), dim3(NT), 0, ctx->stream, x0, ctx_src, noise, t, acp, mask, d, noisy,
                          context, mask_out, C, L, nchunk);
  LAUNCH_CHECK(); return 0;
}

extern "C" int eegldm_context_window(eegldm_ctx* ctx, const float* windows, const float* mask, int down, float* out, int B, int Co, int Lw) {
  EEG_CHECK(ctx && windows && mask && out, "null argument");
  EEG_CHECK(B >= 1 && Co >= 1 && Lw >= 1 && down >= 1 && Lw % down == 0, "B (%d), Co (%d), Lw (%d) >= 1 and Lw a multiple of down (%d)", B, Co, Lw, down);
  for (const void* q : {(const void*)windows, (const void*)mask, (const void*)out}) EEG_CHECK(((uintptr_t)q & 3) == 0, "buffers must be 4-byte aligned");
  const long n = (long)B * Co * Lw, nm = (long)B * (Lw / down);
  EEG_CHECK(!ov(out, n, windows, n) && !ov(out, n, mask, nm), "out aliases an input");
  unsigned blocks; int nchunk; EEG_TRY(chunks_of(B, Co, Lw, &blocks, &nchunk));
  hipLaunchKernelGGL(context_window_kernel, dim3(blocks), dim3(NT), 0, ctx->stream, windows, mask, down, out, Co, Lw, nchunk);
  LAUNCH_CHECK(); return 0;
}
