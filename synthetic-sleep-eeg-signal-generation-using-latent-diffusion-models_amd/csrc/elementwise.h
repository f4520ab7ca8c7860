// Launch geometry and the float4 body / scalar edge split shared by the streaming kernels of elementwise.hip, sampler_steps.hip and
// context.hip.  Internal to those translation units: everything here has internal linkage.
#pragma once
#include <initializer_list>

#include "common.h"

namespace {
constexpr int NT = 256;

inline int grid1d(long n, eegldm_ctx* ctx, int per_thread = 1) {
  long blocks = (n + (long)NT * per_thread - 1) / ((long)NT * per_thread);
  long cap = (long)ctx->num_cu * 16;
  if (blocks < 1) blocks = 1;
  return (int)(blocks < cap ? blocks : cap);
}
#define GRID_STRIDE(i, n) for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// Streaming passes over a flat fp32 buffer with 16-byte accesses.  Elements [0, head) and the last (n - head) % 4 go one by one, the
// body [head, head + 4 * n4) as float4: the launcher picks `head` so that the body of EVERY buffer is 16-byte aligned, which needs all of
// them to share one misalignment; if they do not, head = n and the whole range takes the scalar loop.  n is arbitrary.
struct VecSplit { long head, n4, tail0, nedge; };
__device__ __forceinline__ VecSplit vec_split(long n, long head) {
  VecSplit s; s.head = head; s.n4 = (n - head) >> 2; s.tail0 = head + (s.n4 << 2); s.nedge = head + (n - s.tail0);
  return s;
}
#define EDGE_INDEX(s, j) ((j) < (s).head ? (j) : (s).tail0 + ((j) - (s).head))

// Scalar elements ahead of the float4 body: 0..3 when every buffer has the same offset inside a 16-byte line, else all n of them.
inline long vec_head(long n, std::initializer_list<const void*> ptrs) {
  const uintptr_t mis = (uintptr_t)*ptrs.begin() & 15;
  for (const void* q : ptrs) if (((uintptr_t)q & 15) != mis) return n;
  const long head = (long)(((16 - mis) & 15) >> 2);
  return head < n ? head : n;
}
// blocks for n elements of which the body goes four per thread; 8 blocks per CU keep every CU's memory queue full
inline int grid_vec(long n, long head, eegldm_ctx* ctx) {
  const long work = head >= n ? n : (n - head) >> 2;      // (the <= 6 edge elements fit the first block)
  long blocks = (work + NT - 1) / NT, cap = (long)ctx->num_cu * 8;
  if (blocks < 1) blocks = 1;
  return (int)(blocks < cap ? blocks : cap);
}

// DDPMScheduler.add_noise on one element (sa = sqrt(a_t), sb = sqrt(1 - a_t)): ONE function for add_noise_kernel (sampler_steps.hip) and the
// train step's fused add_noise_context_kernel (context.hip), so both round alike.  A plain expression, contracted the same way wherever it is inlined.
__device__ __forceinline__ float add_noise_value(float x, float nz, float sa, float sb) { return sa * x + sb * nz; }

// ------------------------------------------------------------------ Philox4x32-10 (perf-path RNG; parity runs pass noise in)
__device__ __forceinline__ void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}
__device__ __forceinline__ void philox(unsigned long long seed, unsigned long long ctr, unsigned r[4]) {
  unsigned c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32), c2 = 0, c3 = 0;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; i++) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}
// the four N(0, 1) values of counter `ctr`: Box-Muller on the word pairs (0, 1) and (2, 3).  ONE function for randn_kernel and for the draw
// inside edit_jump_kernel (sampler_steps.hip), so that value e of a stream is the same bits wherever it is formed.
__device__ __forceinline__ void philox_normal4(unsigned long long seed, unsigned long long ctr, float z[4]) {
  unsigned r[4]; philox(seed, ctr, r);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float u1 = ((float)r[2 * h] + 1.0f) * 2.3283064365386963e-10f;   // (0,1]
    const float u2 = (float)r[2 * h + 1] * 2.3283064365386963e-10f;
    const float rad = sqrtf(-2.0f * logf(u1));
    z[2 * h] = rad * cosf(6.283185307179586f * u2); z[2 * h + 1] = rad * sinf(6.283185307179586f * u2);
  }
}
}  // namespace
