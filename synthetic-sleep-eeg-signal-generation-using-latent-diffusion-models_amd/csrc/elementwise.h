// Launch geometry and the float4 body / scalar edge split shared by the streaming kernels of elementwise.hip and sampler_steps.hip.
// Internal to those two translation units: everything here has internal linkage.
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
}  // namespace
