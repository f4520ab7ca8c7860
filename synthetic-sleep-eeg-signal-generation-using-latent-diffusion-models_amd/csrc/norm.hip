// GroupNorm (+SiLU, + fused AvgPool2 / nearest-x2 resampling) forward and backward on the
// NLC layout.  Reference: nn.GroupNorm(32, C, eps=1e-6) at /root/reference/src/models/unet.py:71-74
// used by ResBlock (:260-262, :286-288) and AttentionBlock (:157); MONAI AutoencoderKL uses
// G = norm_num_groups = 1 (config_aekl_eeg.yaml:25).  Up/down ResBlocks resample AFTER the
// activation, on both h and the raw x (unet.py:308-313).
//
// HBM-bound.  Statistics are reduced per (sample, group) with fp32 thread partials (a few
// dozen elements each), LDS float atomics per block, then fp64 global atomics -- biased
// variance from fp64 sums, so E[x^2]-mean^2 cancellation stays below fp32 rounding.
#include "common.h"
#include "internal.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int NT = 256;
constexpr int MAXG_LDS = 1024;   // LDS accumulators per block (groups / channels)
constexpr int GN_NSLOT = 64;     // partial dgamma/dbeta buffers
constexpr int GN_FOLD_MAX = 96;                          // batched folds per flush (the config_ldm UNet has 42 + 7)
constexpr size_t GN_REGION_FLOATS = (size_t)GN_NSLOT * 2 * 1024;   // one launch's slot region (C <= 1024): 512 KiB
constexpr size_t GN_SLOT_OFFSET = 1u << 20;   // byte offset of the slot area inside ctx->scratch (64 slots x 2C floats <= 512 KiB)
constexpr size_t GN_SLOT_OFFSET_B = (1u << 20) + (512u << 10);   // second slot area: partials whose fold the caller runs later (side stream)
// third / fourth slot areas (alternating): folds the caller runs one ResBlock later, inside that block's side-stream section
constexpr size_t GN_SLOT_OFFSET_C[2] = {24u << 20, (24u << 20) + (512u << 10)};
static inline size_t gn_slot_region(int region) { return region == 0 ? GN_SLOT_OFFSET_B : GN_SLOT_OFFSET_C[(region - 1) & 1]; }

template <typename T, int V> struct Vec;
template <> struct Vec<float, 4> { typedef float4 type; };
template <> struct Vec<bf16_t, 4> { typedef uint2 type; };
template <> struct Vec<f16_t, 4> { typedef uint2 type; };

template <typename T> __device__ __forceinline__ void load4(const T* p, float v[4]);
template <> __device__ __forceinline__ void load4<float>(const float* p, float v[4]) {
  float4 t = *(const float4*)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
template <> __device__ __forceinline__ void load4<bf16_t>(const bf16_t* p, float v[4]) {
  uint2 t = *(const uint2*)p;
  v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
  v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
}
template <> __device__ __forceinline__ void load4<f16_t>(const f16_t* p, float v[4]) {
  uint2 t = *(const uint2*)p;
  v[0] = w16_lo<f16_t>(t.x); v[1] = w16_hi<f16_t>(t.x); v[2] = w16_lo<f16_t>(t.y); v[3] = w16_hi<f16_t>(t.y);
}
template <typename T> __device__ __forceinline__ void unpack4(const typename Vec<T, 4>::type& t, float v[4]);
template <> __device__ __forceinline__ void unpack4<f16_t>(const uint2& t, float v[4]) {
  v[0] = w16_lo<f16_t>(t.x); v[1] = w16_hi<f16_t>(t.x); v[2] = w16_lo<f16_t>(t.y); v[3] = w16_hi<f16_t>(t.y);
}
template <> __device__ __forceinline__ void unpack4<float>(const float4& t, float v[4]) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
template <> __device__ __forceinline__ void unpack4<bf16_t>(const uint2& t, float v[4]) {
  v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
  v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
}
template <typename T> __device__ __forceinline__ void store4(T* p, const float v[4]);
template <> __device__ __forceinline__ void store4<float>(float* p, const float v[4]) {
  *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, const float v[4]) {
  uint2 t;
  t.x = pack_bf16x2(v[0], v[1]);
  t.y = pack_bf16x2(v[2], v[3]);
  *(uint2*)p = t;
}
template <> __device__ __forceinline__ void store4<f16_t>(f16_t* p, const float v[4]) {
  uint2 t; t.x = pack_f16x2(v[0], v[1]); t.y = pack_f16x2(v[2], v[3]); *(uint2*)p = t;
}
template <typename T, int V> __device__ __forceinline__ void loadv(const T* p, float v[V]) {
  if constexpr (V == 4) load4<T>(p, v); else v[0] = ld_f32(p);
}
template <typename T, int V> __device__ __forceinline__ void storev(T* p, const float v[V]) {
  if constexpr (V == 4) store4<T>(p, v); else st_f32(p, v[0]);
}

// 1 / (elements per group) for the fp64 group sums.  16-bit engines: the fp64 reciprocal (a float one is inexact unless cpg * L is a power of
// two, and the one-pass variance multiplies that error by mean^2 / var).  The fp32 engine keeps the float reciprocal it always had, widened,
// and in the split backward the float product: its arithmetic, two-pass statistics included, is untouched so that its outputs stay bit-equal.
template <typename T> __device__ __forceinline__ double gn_inv_n(int cpg, int L) {
  if constexpr (sizeof(T) == 2) return 1.0 / ((double)cpg * (double)L);
  else return (double)(1.0f / ((float)cpg * (float)L));
}
template <typename T> __device__ __forceinline__ float gn_split_group_mean(double sum, double inv_n) {
  if constexpr (sizeof(T) == 2) return (float)(sum * inv_n);
  else return (float)sum * (float)inv_n;
}

// thread -> (column-vector, row-lane) decomposition of a block
struct ColMap { int TX, TY, ncols; };
__device__ __forceinline__ ColMap colmap(int C, int V) {
  ColMap m; m.ncols = C / V;
  if (m.ncols >= NT) { m.TX = NT; m.TY = 1; } else { m.TX = m.ncols; m.TY = NT / m.ncols; }
  return m;
}

// ------------------------------------------------------------------ forward statistics
// grid (LSPLIT, B); sums: double [B][G][2] (pre-zeroed)
template <typename T, int V>
__global__ __launch_bounds__(NT) void gn_stats_kernel(const T* __restrict__ x, long ldx, double* __restrict__ sums,
                                                      int L, int C, int G, int rows_per_block) {
  __shared__ double acc[2 * MAXG_LDS];   // fp64 like the global sums: the arrival order of the threads must not show in the statistics (reproducible forward)
  const int b = blockIdx.y, tid = threadIdx.x;
  const int cpg = C / G;
  for (int i = tid; i < 2 * G; i += NT) acc[i] = 0.0;
  __syncthreads();
  const ColMap cm = colmap(C, V);
  const int l0 = blockIdx.x * rows_per_block, l1 = min(L, l0 + rows_per_block);
  if (tid < cm.TX * cm.TY) {
    const int tx = tid % cm.TX, ty = tid / cm.TX;
    for (int col = tx; col < cm.ncols; col += cm.TX) {
      const int c = col * V;
      float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
      for (int l = l0 + ty; l < l1; l += cm.TY) {
        float v[V];
        loadv<T, V>(x + ((long)b * L + l) * ldx + c, v);
#pragma unroll
        for (int k = 0; k < V; k++) { s1 += v[k]; s2 += v[k] * v[k]; }
      }
      const int g = c / cpg;
      atomicAdd(&acc[2 * g], (double)s1);
      atomicAdd(&acc[2 * g + 1], (double)s2);
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * G; i += NT) atomicAdd(&sums[(long)b * G * 2 + i], acc[i]);
}

// (self-cleaning: the accumulators are zeroed again for the next GroupNorm, so no memset launches are needed)
__global__ void gn_finalize_kernel(double* __restrict__ sums, float* __restrict__ stats, int BG, double n, float eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BG) return;
  const double mean = sums[2 * i] / n;
  double var = sums[2 * i + 1] / n - mean * mean;
  sums[2 * i] = 0.0; sums[2 * i + 1] = 0.0;
  if (var < 0) var = 0;
  stats[2 * i] = (float)mean;
  stats[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

// ------------------------------------------------------------------ forward apply
// grid (row chunks, B): block = one sample, a run of WORK rows (work row = output row for avgpool, input row
// otherwise).  Threads tile (column vector, row lane) like the statistics kernel, so the element loop has no
// integer division; per-thread scale/shift are hoisted out of the row loop.
// resample: 0 none, 1 avgpool2 (pairs of input rows -> one output row), 2 nearest x2 (one input row -> two output rows)
template <typename T, int V>
__global__ __launch_bounds__(NT) void gn_apply_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ stats,
                                                      T* __restrict__ y, long ldy, T* __restrict__ xr, long ldxr,
                                                      int L, int C, int G, int silu, int resample, int rows_per_block) {
  const int b = blockIdx.y, tid = threadIdx.x, cpg = C / G;
  const ColMap cm = colmap(C, V);
  if (tid >= cm.TX * cm.TY) return;
  const int tx = tid % cm.TX, ty = tid / cm.TX;
  const int Lw = (resample == 1) ? L / 2 : L;
  const int l0 = blockIdx.x * rows_per_block, l1 = min(Lw, l0 + rows_per_block);
  const T* xb = x + (long)b * L * ldx;
  for (int col = tx; col < cm.ncols; col += cm.TX) {
    const int c = col * V, g = c / cpg;
    const float mean = stats[((long)b * G + g) * 2], rstd = stats[((long)b * G + g) * 2 + 1];
    float ga[V], be[V];
#pragma unroll
    for (int k = 0; k < V; k++) { ga[k] = gamma[c + k] * rstd; be[k] = beta[c + k] - mean * ga[k]; }
    if (resample == 1) {
      T* yb = y + (long)b * Lw * ldy; T* xrb = xr ? xr + (long)b * Lw * ldxr : nullptr;
      for (int lw = l0 + ty; lw < l1; lw += cm.TY) {
        float v0[V], v1[V], o[V], r[V];
        loadv<T, V>(xb + (long)(2 * lw) * ldx + c, v0);
        loadv<T, V>(xb + (long)(2 * lw + 1) * ldx + c, v1);
#pragma unroll
        for (int k = 0; k < V; k++) {
          float z0 = v0[k] * ga[k] + be[k], z1 = v1[k] * ga[k] + be[k];
          if (silu) { z0 = silu_f(z0); z1 = silu_f(z1); }
          o[k] = 0.5f * (z0 + z1); r[k] = 0.5f * (v0[k] + v1[k]);
        }
        storev<T, V>(yb + (long)lw * ldy + c, o);
        if (xrb) storev<T, V>(xrb + (long)lw * ldxr + c, r);
      }
    } else if (resample == 0) {
      T* yb = y + (long)b * L * ldy;
#pragma unroll 4
      for (int lw = l0 + ty; lw < l1; lw += cm.TY) {
        float v[V], o[V];
        loadv<T, V>(xb + (long)lw * ldx + c, v);
#pragma unroll
        for (int k = 0; k < V; k++) { float z = v[k] * ga[k] + be[k]; o[k] = silu ? silu_f(z) : z; }
        storev<T, V>(yb + (long)lw * ldy + c, o);
      }
    } else {
      T* yb = y + (long)b * 2 * L * ldy; T* xrb = xr ? xr + (long)b * 2 * L * ldxr : nullptr;
      for (int lw = l0 + ty; lw < l1; lw += cm.TY) {
        float v[V], o[V];
        loadv<T, V>(xb + (long)lw * ldx + c, v);
#pragma unroll
        for (int k = 0; k < V; k++) { float z = v[k] * ga[k] + be[k]; o[k] = silu ? silu_f(z) : z; }
        storev<T, V>(yb + (long)(2 * lw) * ldy + c, o); storev<T, V>(yb + (long)(2 * lw + 1) * ldy + c, o);
        if (xrb) { storev<T, V>(xrb + (long)(2 * lw) * ldxr + c, v); storev<T, V>(xrb + (long)(2 * lw + 1) * ldxr + c, v); }
      }
    }
  }
}

// ------------------------------------------------------------------ backward
// effective upstream gradient at input row (b,l), channels c..c+V-1
// (resample mode as a compile-time constant inside streaming loops: a run-time branch around the load makes hipcc wait
//  for every load separately instead of keeping an unrolled batch in flight)
template <typename T, int V, int RS>
__device__ __forceinline__ void load_dy_eff_c(const T* dy, long lddy, int b, int l, int L, int c, float d[V]) {
  if constexpr (RS == 0) {
    loadv<T, V>(dy + ((long)b * L + l) * lddy + c, d);
  } else if constexpr (RS == 1) {
    loadv<T, V>(dy + ((long)b * (L / 2) + (l >> 1)) * lddy + c, d);
#pragma unroll
    for (int k = 0; k < V; k++) d[k] *= 0.5f;
  } else {
    float e[V];
    loadv<T, V>(dy + ((long)b * 2 * L + 2 * l) * lddy + c, d);
    loadv<T, V>(dy + ((long)b * 2 * L + 2 * l + 1) * lddy + c, e);
#pragma unroll
    for (int k = 0; k < V; k++) d[k] += e[k];
  }
}

// grid (LSPLIT, B): group sums S1 = sum dz*gamma, S2 = sum dz*gamma*xhat -> gsums double [B][G][2];
// dgamma[c] += sum dz*xhat, dbeta[c] += sum dz (fp32 atomics)
template <typename T, int V, int RS>
__global__ __launch_bounds__(NT) void gn_bwd_reduce_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ stats,
                                                           const T* __restrict__ dy, long lddy, double* __restrict__ gsums,
                                                           float* __restrict__ slots,
                                                           int L, int C, int G, int silu, int rows_per_block, int nslot) {
  __shared__ double accg[2 * MAXG_LDS];  // group sums feed dx: fp64 so that the thread arrival order does not show (see gn_stats_kernel)
  __shared__ double accc[2 * MAXG_LDS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int cpg = C / G;
  for (int i = tid; i < 2 * G; i += NT) accg[i] = 0.0;
  for (int i = tid; i < 2 * C; i += NT) accc[i] = 0.0;
  __syncthreads();
  const ColMap cm = colmap(C, V);
  const int l0 = blockIdx.x * rows_per_block, l1 = min(L, l0 + rows_per_block);
  if (tid < cm.TX * cm.TY) {
    const int tx = tid % cm.TX, ty = tid / cm.TX;
    for (int col = tx; col < cm.ncols; col += cm.TX) {
      const int c = col * V, g = c / cpg;
      const float mean = stats[((long)b * G + g) * 2], rstd = stats[((long)b * G + g) * 2 + 1];
      float ga[V], be[V], dg[V], db[V];
#pragma unroll
      for (int k = 0; k < V; k++) { ga[k] = gamma[c + k]; be[k] = beta[c + k]; dg[k] = 0.f; db[k] = 0.f; }
      float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
      for (int l = l0 + ty; l < l1; l += cm.TY) {
        float v[V], d[V];
        loadv<T, V>(x + ((long)b * L + l) * ldx + c, v);
        load_dy_eff_c<T, V, RS>(dy, lddy, b, l, L, c, d);
#pragma unroll
        for (int k = 0; k < V; k++) {
          const float xh = (v[k] - mean) * rstd;
          float dz = d[k];
          if (silu) dz *= silu_grad_f(ga[k] * xh + be[k]);
          dg[k] += dz * xh; db[k] += dz;
          s1 += dz * ga[k]; s2 += dz * ga[k] * xh;
        }
      }
      atomicAdd(&accg[2 * g], (double)s1); atomicAdd(&accg[2 * g + 1], (double)s2);
#pragma unroll
      for (int k = 0; k < V; k++) { atomicAdd(&accc[c + k], (double)dg[k]); atomicAdd(&accc[C + c + k], (double)db[k]); }
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * G; i += NT) atomicAdd(&gsums[(long)b * G * 2 + i], accg[i]);
  // per-channel sums go to one of NSLOT partial buffers (thousands of blocks hammering 2C addresses serialise in L2)
  if (slots) {
    float* sl = slots + (size_t)((blockIdx.y * gridDim.x + blockIdx.x) % nslot) * 2 * C;
    for (int i = tid; i < 2 * C; i += NT) atomicAdd(&sl[i], (float)accc[i]);
  }
}

// runs AFTER the backward apply kernel: folds the slots into dgamma/dbeta and re-zeroes slots and group sums
__global__ void gn_slot_reduce_kernel(float* __restrict__ slots, float* __restrict__ dgamma, float* __restrict__ dbeta, int C,
                                      double* __restrict__ gsums, int n_gsums, int nslot = GN_NSLOT) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  for (int k = i; k < n_gsums; k += gridDim.x * blockDim.x) gsums[k] = 0.0;
  if (i >= 2 * C || !slots) return;
  float s = 0.f;
  for (int k = 0; k < nslot; k++) { s += slots[(size_t)k * 2 * C + i]; slots[(size_t)k * 2 * C + i] = 0.f; }
  if (i < C) dgamma[i] += s; else dbeta[i - C] += s;
}

// dx = rstd * (dz*gamma - S1/n - xhat*S2/n) [+ resample^T(dxr)];  grid (row chunks, B), same tiling as the forward
template <typename T, int V, int RS>
__global__ __launch_bounds__(NT) void gn_bwd_apply_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ stats,
                                                          const T* __restrict__ dy, long lddy, const double* __restrict__ gsums,
                                                          T* __restrict__ dx, long lddx, const T* __restrict__ dxr, long lddxr,
                                                          int L, int C, int G, int silu, int rows_per_block) {
  const int b = blockIdx.y, tid = threadIdx.x, cpg = C / G;
  const ColMap cm = colmap(C, V);
  if (tid >= cm.TX * cm.TY) return;
  const int tx = tid % cm.TX, ty = tid / cm.TX;
  const double inv_n = gn_inv_n<T>(cpg, L);
  const int l0 = blockIdx.x * rows_per_block, l1 = min(L, l0 + rows_per_block);
  for (int col = tx; col < cm.ncols; col += cm.TX) {
    const int c = col * V, g = c / cpg;
    const float mean = stats[((long)b * G + g) * 2], rstd = stats[((long)b * G + g) * 2 + 1];
    const float m1 = gn_split_group_mean<T>(gsums[((long)b * G + g) * 2], inv_n), m2 = gn_split_group_mean<T>(gsums[((long)b * G + g) * 2 + 1], inv_n);
    float ga[V], be[V];
#pragma unroll
    for (int k = 0; k < V; k++) { ga[k] = gamma[c + k]; be[k] = beta[c + k]; }
#pragma unroll 2
    for (int l = l0 + ty; l < l1; l += cm.TY) {
      const long row = (long)b * L + l;
      float v[V], d[V], o[V];
      loadv<T, V>(x + row * ldx + c, v);
      load_dy_eff_c<T, V, RS>(dy, lddy, b, l, L, c, d);
#pragma unroll
      for (int k = 0; k < V; k++) {
        const float xh = (v[k] - mean) * rstd;
        float dz = d[k];
        if (silu) dz *= silu_grad_f(ga[k] * xh + be[k]);
        o[k] = rstd * (dz * ga[k] - m1 - xh * m2);
      }
      if (dxr) {
        float e[V];
        load_dy_eff_c<T, V, RS>(dxr, lddxr, b, l, L, c, e);
#pragma unroll
        for (int k = 0; k < V; k++) o[k] += e[k];
      }
      storev<T, V>(dx + row * lddx + c, o);
    }
  }
}

// effective upstream gradient from a wave-uniform per-sample base and 32-bit byte offsets (the one-pass kernels: per-lane
// 64-bit pointer arithmetic was ~30 % of their VALU instructions, and they are VALU-bound)
template <typename T>
__device__ __forceinline__ void load_dy_eff32(const char* base, unsigned ldb, unsigned cb, int l, int resample, float d[4]) {
  if (resample == 0) {
    load4<T>((const T*)(base + ((unsigned)l * ldb + cb)), d);
  } else if (resample == 1) {
    load4<T>((const T*)(base + ((unsigned)(l >> 1) * ldb + cb)), d);
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] *= 0.5f;
  } else {
    float e[4];
    load4<T>((const T*)(base + ((unsigned)(2 * l) * ldb + cb)), d);
    load4<T>((const T*)(base + ((unsigned)(2 * l + 1) * ldb + cb)), e);
#pragma unroll
    for (int k = 0; k < 4; k++) d[k] += e[k];
  }
}
__device__ __forceinline__ long dy_rows(int L, int resample) { return resample == 1 ? L / 2 : (resample == 2 ? 2L * L : L); }

// ------------------------------------------------------------------ register-resident one-pass GroupNorm
// A 1024-thread block owns ONE sample x a chunk of CC channels (whole groups) over the full length L and keeps its
// rows in registers: x (and dy) are read from HBM exactly once, statistics / group sums are reduced inside the
// block (no global atomics, no finalize launch), and the normalised output / input gradient is produced from the
// registers.  HBM traffic: forward 1R+1W (was 2R+1W), backward 2R+1W (was 4R+1W).
// Thread (tx, ty): tx = 4-channel vector column of the chunk, ty = row lane; row k of a thread is k*TY + ty, or in
// pair mode (avgpool) rows 2*((k/2)*TY + ty) + k%2 so that both rows of a pooling pair live in one thread.
constexpr int NTB = 1024;
constexpr int RES_MAXG = 64;     // local groups per chunk
constexpr int RES_MAXC = 256;    // channels per chunk

struct ResMap { int TX, TY, tx, ty, c, gl, b; bool act; };
// The grid is 1-D: linear id -> (channel chunk, sample).  Plain order = chunk fastest.  XCD-aware order (`xcd` != 0, B % 8 == 0): the
// hardware deals consecutive workgroup ids round-robin to the 8 XCDs, so ids = x (mod 8) run on XCD x in increasing order; the j-th of
// them is chunk j % nchunk of sample (j / nchunk) * 8 + x -- all chunks of one sample run back to back on ONE XCD, so a 128-byte line
// that several narrow chunks share is fetched from HBM once and served to its other readers by that XCD's L2.
template <int NTH>
__device__ __forceinline__ ResMap resmap(int CC, int C, int cpg, int xcd) {
  ResMap m; m.TX = CC / 4; m.TY = NTH / m.TX;
  const int tid = threadIdx.x;
  const int nchunk = C / CC, lin = blockIdx.x;
  int chunk, b;
  if (xcd) { const int x = lin & 7, j = lin >> 3; b = (j / nchunk) * 8 + x; chunk = j % nchunk; }
  else { chunk = lin % nchunk; b = lin / nchunk; }
  m.b = b;
  m.tx = tid % m.TX; m.ty = tid / m.TX;
  m.c = chunk * CC + m.tx * 4; m.gl = (m.tx * 4) / cpg;
  m.act = tid < m.TX * m.TY && m.c < C;
  return m;
}
__device__ __forceinline__ int res_row(int k, int ty, int TY, bool pair) {
  return pair ? 2 * ((k >> 1) * TY + ty) + (k & 1) : k * TY + ty;
}
// Full-slab backward, between pass 1 and pass 2: the packed rows pass through an empty asm statement, so that pass 2 unpacks them again.
// Without it hipcc carries xhat of pass 1 over the barriers in place of the packed rows -- twice the registers -- and spills.  No
// instruction is emitted and no value changes.
// compiler-only fence (no instruction): the loads above it stay in front of the loads below it in the in-order memory queue
__device__ __forceinline__ void gn_issue_order() { asm volatile("" ::: "memory"); }
__device__ __forceinline__ void keep_packed(uint2& r) { asm volatile("" : "+v"(r.x), "+v"(r.y)); }
__device__ __forceinline__ void keep_packed(float4& r) { asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w)); }

#ifdef EEG_STAGE_TIMING
__device__ unsigned long long gn_tlog[4096 * 8];
#define GN_TSTAMP(k) do { if (threadIdx.x == 0) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); gn_tlog[((size_t)blockIdx.y * gridDim.x + blockIdx.x) % 4096 * 8 + (k)] = __builtin_readcyclecounter(); } } while (0)
#else
#define GN_TSTAMP(k) do {} while (0)
#endif
template <typename T, int RPT, int NTH>
__global__ __launch_bounds__(NTH) void gn_fwd_resident_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, T* __restrict__ y, long ldy,
                                                              T* __restrict__ xr, long ldxr, float* __restrict__ stats,
                                                              int L, int C, int G, float eps, int silu, int resample, int CC, int xcd) {
  // fp64 LDS accumulators: the order in which the waves arrive no longer shows in the fp32 mean / rstd, so the forward (and with it
  // seeded sampling) is reproducible run to run -- fp32 atomics differed in the last bit and bf16 roundings downstream flipped
  __shared__ double red[2 * RES_MAXG];
  GN_TSTAMP(0);
  const int cpg = C / G;
  const ResMap m = resmap<NTH>(CC, C, cpg, xcd);
  const int b = m.b;
  const bool pair = resample == 1;
  for (int i = threadIdx.x; i < 2 * RES_MAXG; i += NTH) red[i] = 0.0;
  typename Vec<T, 4>::type raw[RPT];
  const T* xb = x + (long)b * L * ldx + m.c;
  float pv = 0.f;      // 16-bit engines: the group's first element, the pivot of the one-pass statistics below (first in the load queue)
  if constexpr (sizeof(T) == 2) { if (m.act) pv = ld_f32<T>(x + (long)b * L * ldx + (m.c / cpg) * cpg); }
  if (m.act) {
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      const int l = res_row(k, m.ty, m.TY, pair);
      if (l < L) raw[k] = *(const typename Vec<T, 4>::type*)(xb + (long)l * ldx);
    }
  }
  GN_TSTAMP(1);
  __syncthreads();
  GN_TSTAMP(2);
  const double inv_n = gn_inv_n<T>(cpg, L);
  float mean = 0.f, rstd = 0.f;
  if constexpr (sizeof(T) == 2) {
    // 16-bit storage: ONE reduction round.  Sum and sum of squares are taken in fp32 per thread (<= 48 elements) about a PIVOT that every
    // thread of the (sample, group) shares -- the group's first element, one extra broadcast load issued with the rows -- accumulated in
    // fp64 across the block, and mean = pivot + E[d], var = E[d^2] - E[d]^2 in fp64 with d = x - pivot.  The differences are exact in fp32
    // for 16-bit inputs of similar magnitude, and the relative error of the fp32 partials (~1e-7) is amplified by 1 + (mean - pivot)^2 / var,
    // a few units whatever the mean is.  Saves the second barrier round of the two-pass form (mean first, then centred squares: 5.3 k of
    // the block's 28 k cycles, tools/debug/gn_timing.py).  The fp32 engine keeps two passes.
    // What was found here: until this form the sums were taken about zero and scaled by a FLOAT 1 / n.  Both errors are ~1e-7 relative but
    // enter var = E[x^2] - mean^2 multiplied by mean^2 / var (900 at mean 30 x std): the inexact reciprocal shifts var by
    // e (E[x^2] - 2 mean^2) on every group alike (-2.7e-5 relative in bf16, whose partials are exact), and the fp32 partial of x^2 (4e4 after
    // 48 elements of 30^2, fp16 squares need 2^-12) rounds without averaging out over a group's threads.  At mean 30 x std the fp16 output
    // carried +0.07 ulp of bias (8 % of its elements off the correctly rounded value), the bf16 data gradient differed on 0.3 %
    // (tests/test_groupnorm_numerics_cpu.py restates both arithmetics on the CPU; tests/test_gpu_groupnorm_rounding.py holds the kernels).
    float s1 = 0.f, s2 = 0.f;
    if (m.act) {
#pragma unroll
      for (int k = 0; k < RPT; k++) {
        if (res_row(k, m.ty, m.TY, pair) < L) {
          float v[4]; unpack4<T>(raw[k], v);
#pragma unroll
          for (int j = 0; j < 4; j++) v[j] -= pv;
          s1 += (v[0] + v[1]) + (v[2] + v[3]);
          s2 = fmaf(v[0], v[0], s2); s2 = fmaf(v[1], v[1], s2); s2 = fmaf(v[2], v[2], s2); s2 = fmaf(v[3], v[3], s2);
        }
      }
      atomicAdd(&red[m.gl], (double)s1); atomicAdd(&red[RES_MAXG + m.gl], (double)s2);
    }
    __syncthreads();
    GN_TSTAMP(3);
    GN_TSTAMP(4);
    if (!m.act) return;
    const double md = red[m.gl] * inv_n;
    double var = red[RES_MAXG + m.gl] * inv_n - md * md; if (var < 0.0) var = 0.0;
    mean = (float)((double)pv + md);
    rstd = rsqrtf((float)var + eps);
  } else {
  float s = 0.f;
  if (m.act) {
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      if (res_row(k, m.ty, m.TY, pair) < L) { float v[4]; unpack4<T>(raw[k], v); s += (v[0] + v[1]) + (v[2] + v[3]); }
    }
    atomicAdd(&red[m.gl], (double)s);
  }
  __syncthreads();
  GN_TSTAMP(3);
  if (m.act) {
    mean = (float)(red[m.gl] * inv_n);
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      if (res_row(k, m.ty, m.TY, pair) < L) {
        float v[4]; unpack4<T>(raw[k], v);
#pragma unroll
        for (int j = 0; j < 4; j++) { const float d = v[j] - mean; q += d * d; }
      }
    }
    atomicAdd(&red[RES_MAXG + m.gl], (double)q);
  }
  __syncthreads();
  GN_TSTAMP(4);
  if (!m.act) return;
  rstd = rsqrtf((float)(red[RES_MAXG + m.gl] * inv_n) + eps);
  }
  if (m.ty == 0 && (m.tx * 4) % cpg == 0) { float* st = stats + ((long)b * G + m.c / cpg) * 2; st[0] = mean; st[1] = rstd; }
  float ga[4], be[4];
#pragma unroll
  for (int j = 0; j < 4; j++) { ga[j] = gamma[m.c + j] * rstd; be[j] = beta[m.c + j] - mean * ga[j]; }
  if (resample == 1) {
    T* yb = y + (long)b * (L / 2) * ldy + m.c; T* xrb = xr ? xr + (long)b * (L / 2) * ldxr + m.c : nullptr;
#pragma unroll
    for (int k = 0; k + 1 < RPT; k += 2) {
      const int l = res_row(k, m.ty, m.TY, true);
      if (l + 1 < L) {
        float v0[4], v1[4], o[4], r[4];
        unpack4<T>(raw[k], v0); unpack4<T>(raw[k + 1], v1);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          float z0 = v0[j] * ga[j] + be[j], z1 = v1[j] * ga[j] + be[j];
          if (silu) { z0 = silu_f(z0); z1 = silu_f(z1); }
          o[j] = 0.5f * (z0 + z1); r[j] = 0.5f * (v0[j] + v1[j]);
        }
        store4<T>(yb + (long)(l >> 1) * ldy, o);
        if (xrb) store4<T>(xrb + (long)(l >> 1) * ldxr, r);
      }
    }
  } else {
    const int up = resample == 2 ? 2 : 1;
    T* yb = y + (long)b * up * L * ldy + m.c; T* xrb = (xr && up == 2) ? xr + (long)b * 2 * L * ldxr + m.c : nullptr;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      const int l = res_row(k, m.ty, m.TY, false);
      if (l < L) {
        float v[4], o[4];
        unpack4<T>(raw[k], v);
#pragma unroll
        for (int j = 0; j < 4; j++) { const float z = v[j] * ga[j] + be[j]; o[j] = silu ? silu_f(z) : z; }
        if (up == 1) store4<T>(yb + (long)l * ldy, o);
        else {
          store4<T>(yb + (long)(2 * l) * ldy, o); store4<T>(yb + (long)(2 * l + 1) * ldy, o);
          if (xrb) { store4<T>(xrb + (long)(2 * l) * ldxr, v); store4<T>(xrb + (long)(2 * l + 1) * ldxr, v); }
        }
      }
    }
  }
  GN_TSTAMP(5);
}

// backward: dgamma/dbeta partials go to the slot buffers (folded by gn_slot_reduce_kernel); colsum_ps (optional) receives
// the per-sample column sums of the written dx -- the block owns (sample, channels) over all of L, so no atomics.
// RAW0: resample == 0 specialisation that fetches the gradient rows packed, in the same predicated block as the x rows (the
// conversion in place makes hipcc wait for every load separately: 12 serialised HBM latencies, 19 k of the block's 57 k cycles)
template <typename T, int RPT, bool RAW0, bool SILU, int NTH>
__global__ __launch_bounds__(NTH) void gn_bwd_resident_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ stats,
                                                              const T* __restrict__ dy, long lddy, T* __restrict__ dx, long lddx,
                                                              const T* __restrict__ dxr, long lddxr, float* __restrict__ slots,
                                                              float* __restrict__ colsum_ps, long ldps,
                                                              int L, int C, int G, int silu, int resample, int CC,
                                                              const T* __restrict__ dxr2, long lddxr2, int xcd, int nslot) {
  // fp64 LDS accumulators (as in the forward): dx must not depend on the order in which the waves arrive -- an fp32 one-ulp
  // difference in the group sums flips bf16 roundings of dx and the flips compound through the remaining layers
  __shared__ double redg[2 * RES_MAXG];
  __shared__ double redc[3 * RES_MAXC];
  GN_TSTAMP(0);
  const int cpg = C / G;
  const ResMap m = resmap<NTH>(CC, C, cpg, xcd);
  const int b = m.b;
  for (int i = threadIdx.x; i < 2 * RES_MAXG + 3 * RES_MAXC; i += NTH) { if (i < 2 * RES_MAXG) redg[i] = 0.0; else redc[i - 2 * RES_MAXG] = 0.0; }
  typename Vec<T, 4>::type raw[RPT];
  float d[RPT][4];
  // wave-uniform per-sample bases + 32-bit byte offsets (scalar-base addressing: one VALU add per access)
  const char* xs = (const char*)(x + (long)b * L * ldx);
  const char* dys = (const char*)(dy + (long)b * dy_rows(L, resample) * lddy);
  const unsigned cb = (unsigned)m.c * (unsigned)sizeof(T);
  const unsigned ldxb = (unsigned)ldx * (unsigned)sizeof(T), lddyb = (unsigned)lddy * (unsigned)sizeof(T);
  typename Vec<T, 4>::type dr[RAW0 ? RPT : 1];
  if (m.act) {
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      const int l = k * m.TY + m.ty;
      if (l < L) {
        raw[k] = *(const typename Vec<T, 4>::type*)(xs + ((unsigned)l * ldxb + cb));
        if constexpr (RAW0) dr[k] = *(const typename Vec<T, 4>::type*)(dys + ((unsigned)l * lddyb + cb));
      }
    }
    if constexpr (!RAW0) {
#pragma unroll
      for (int k = 0; k < RPT; k++) {
        const int l = k * m.TY + m.ty;
        if (l < L) load_dy_eff32<T>(dys, lddyb, cb, l, resample, d[k]);
      }
    }
  }
  GN_TSTAMP(1);
  __syncthreads();
  GN_TSTAMP(2);
  float mean = 0.f, rstd = 0.f, ga[4], be[4];
  if (m.act) {
    const float* st = stats + ((long)b * G + m.c / cpg) * 2;
    mean = st[0]; rstd = st[1];
    float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; j++) { ga[j] = gamma[m.c + j]; be[j] = beta[m.c + j]; }
    // pass 1 is VALU issue-bound (profiles/r01_gemm_stage_timing.txt): xhat as one FMA, SiLU' evaluated unconditionally and
    // selected (no per-element branch), and the group sums S1 = sum dz*gamma, S2 = sum dz*gamma*xhat are NOT accumulated per
    // element -- they follow from the per-channel sums after the block reduction (S1 = sum_c gamma_c db_c, S2 = sum_c gamma_c dg_c)
    const float nmr = -mean * rstd;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      if (k * m.TY + m.ty < L) {
        float v[4]; unpack4<T>(raw[k], v);
        if constexpr (RAW0) unpack4<T>(dr[k], d[k]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float xh = fmaf(v[j], rstd, nmr);
          float dz = d[k][j];
          if constexpr (SILU) dz *= silu_grad_f(fmaf(ga[j], xh, be[j]));   // (compile-time: a run-time select cost one v_cndmask per element)
          d[k][j] = dz;
          dg[j] = fmaf(dz, xh, dg[j]); db[j] += dz;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) { atomicAdd(&redc[m.tx * 4 + j], (double)dg[j]); atomicAdd(&redc[RES_MAXC + m.tx * 4 + j], (double)db[j]); }
  }
  // the residual-path addend(s) of dx are fetched HERE, packed and unconditionally (clamped row), so their round trip runs under the
  // two barriers and the group-sum phase: loaded inside pass 2 they were twelve load-wait-use chains per thread (the first GroupNorm of
  // every ResBlock has such an addend: those launches took ~70 us against 45 us without)
  typename Vec<T, 4>::type er[RAW0 ? RPT : 1];      // (the rarer second addend stays an in-loop load: both arrays spill at 12 rows per thread)
  if constexpr (RAW0) {
    if (m.act && dxr) {
      const char* q = (const char*)(dxr + (long)b * L * lddxr);
      const unsigned ldb = (unsigned)lddxr * (unsigned)sizeof(T);
#pragma unroll
      for (int k = 0; k < RPT; k++) { const int l = k * m.TY + m.ty, lc = l < L ? l : L - 1; er[k] = *(const typename Vec<T, 4>::type*)(q + ((unsigned)lc * ldb + cb)); }
    }
  }
  __syncthreads();
  if (m.act && m.ty == 0) {
    double p1 = 0.0, p2 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) { p1 += (double)ga[j] * redc[RES_MAXC + m.tx * 4 + j]; p2 += (double)ga[j] * redc[m.tx * 4 + j]; }
    atomicAdd(&redg[2 * m.gl], p1); atomicAdd(&redg[2 * m.gl + 1], p2);
  }
  GN_TSTAMP(3);
  __syncthreads();
  GN_TSTAMP(4);
  if (m.act) {
    const double inv_n = gn_inv_n<T>(cpg, L);
    const float m1 = (float)(redg[2 * m.gl] * inv_n), m2 = (float)(redg[2 * m.gl + 1] * inv_n);
    if (slots && m.ty == 0) {
      float* sl = slots + (size_t)(b % nslot) * 2 * C;
#pragma unroll
      for (int j = 0; j < 4; j++) { atomicAdd(&sl[m.c + j], (float)redc[m.tx * 4 + j]); atomicAdd(&sl[C + m.c + j], (float)redc[RES_MAXC + m.tx * 4 + j]); }
    }
    // dx = rstd * (dz*gamma - m1 - xhat*m2) with the per-thread constants folded
    const float rm1 = rstd * m1, rm2 = rstd * m2;
    float gr[4];
#pragma unroll
    for (int j = 0; j < 4; j++) gr[j] = ga[j] * rstd;
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
    char* dxs = (char*)(dx + (long)b * L * lddx);
    const char* dxrs = dxr ? (const char*)(dxr + (long)b * dy_rows(L, resample) * lddxr) : nullptr;
    const unsigned lddxb = (unsigned)lddx * (unsigned)sizeof(T), lddxrb = (unsigned)lddxr * (unsigned)sizeof(T);
    const char* dxr2s = dxr2 ? (const char*)(dxr2 + (long)b * L * lddxr2) : nullptr;
    const unsigned lddxr2b = (unsigned)lddxr2 * (unsigned)sizeof(T);
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      const int l = k * m.TY + m.ty;
      if (l < L) {
        float v[4], o[4]; unpack4<T>(raw[k], v);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float xh = fmaf(v[j], rstd, -mean * rstd);
          o[j] = fmaf(d[k][j], gr[j], fmaf(xh, -rm2, -rm1));
        }
        if (dxr) {
          float e[4];
          if constexpr (RAW0) unpack4<T>(er[k], e); else load_dy_eff32<T>(dxrs, lddxrb, cb, l, resample, e);
#pragma unroll
          for (int j = 0; j < 4; j++) o[j] += e[j];
        }
        if (dxr2) {      // second addend at dx's own resolution (UNet skip gradient): saves a separate read-modify-write pass over dx
          float e[4];
          load4<T>((const T*)(dxr2s + ((unsigned)l * lddxr2b + cb)), e);
#pragma unroll
          for (int j = 0; j < 4; j++) o[j] += e[j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) cs[j] += o[j];
        store4<T>((T*)(dxs + ((unsigned)l * lddxb + cb)), o);
      }
    }
    if (colsum_ps) {
#pragma unroll
      for (int j = 0; j < 4; j++) atomicAdd(&redc[2 * RES_MAXC + m.tx * 4 + j], (double)cs[j]);
    }
  }
  GN_TSTAMP(5);
  if (colsum_ps) {
    __syncthreads();
    if (m.act && m.ty == 0) {
#pragma unroll
      for (int j = 0; j < 4; j++) colsum_ps[(long)b * ldps + m.c + j] = (float)redc[2 * RES_MAXC + m.tx * 4 + j];
    }
  }
}

// FULL-SLAB form of the backward (1024 threads, every thread active, RPT * TY == L), bit-identical to gn_bwd_resident_kernel: same partial
// sums in the same order, same fp64 accumulators, same mapping.  What differs is what the memory queue sees ("Counting vmcnt"):
//   * no `l < L` / `m.act` predicate; the resampling mode (RS) and the presence of the addends and of the column sums (FL: bit 0 dxr, 1 dxr2,
//     2 colsum_ps) are compile-time, so no unrolled loop contains a branch and hipcc keeps count of the outstanding loads and stores
//     (`slots` stays a run-time test: it guards eight atomics of the ty == 0 threads in front of pass 2, not a loop);
//   * (mean, rstd), gamma and beta are loaded FIRST, in front of the rows: pass 1 (VALU-bound: exp + rcp per element) starts on row 0 while
//     rows 1.. are still in flight (vmcnt counts down) -- loaded behind the rows, their first use waited for the whole slab;
//   * pass 2 stores free-running: the predicated kernel waits vmcnt(1) / vmcnt(0) in every row = for the previous row's store to be acknowledged;
//   * every tensor is addressed as (wave-uniform base + k * row-lane stride) + ONE per-thread offset: twelve per-row offsets per tensor in
//     VGPRs are what pushed the addend variants over 128 registers.
// The gradient rows are fetched packed at every RS (RS 2: both rows of the pair) and converted in pass 1; a lone first addend is fetched
// packed under the barrier rounds at RS 0 / 1.  What stays a load inside pass 2 -- a further 12-row register array (24 at RS 2) does not
// fit 128 VGPRs -- is the first addend at RS 2 and BOTH addends where there are two (seven of the LDM UNet's launches per step: the skip gradient);
// in straight-line code hipcc issues those loads rows ahead of their use and waits with a count.
template <typename T, int RS> struct GnDyRow {      // dy-resolution row(s) of the thread's row k = k * TY + ty (TY is even: resident_full_slab)
  unsigned stride, off;                              // bytes: per k (wave-uniform), per thread
  __device__ __forceinline__ GnDyRow(int ty, int TY, unsigned ldb, unsigned cb) {
    stride = (RS == 0 ? (unsigned)TY : RS == 1 ? (unsigned)TY >> 1 : 2u * (unsigned)TY) * ldb;
    off = (RS == 0 ? (unsigned)ty : RS == 1 ? (unsigned)ty >> 1 : 2u * (unsigned)ty) * ldb + cb;
  }
  __device__ __forceinline__ typename Vec<T, 4>::type ld(const char* base, int k, unsigned second) const {
    return *(const typename Vec<T, 4>::type*)(base + (size_t)k * stride + (off + second));
  }
};
// effective gradient of one row from its packed row(s): the arithmetic of load_dy_eff32
template <typename T, int RS>
__device__ __forceinline__ void gn_dy_eff(const typename Vec<T, 4>::type& a, const typename Vec<T, 4>::type& a2, float d[4]) {
  unpack4<T>(a, d);
  if constexpr (RS == 1) {
#pragma unroll
    for (int j = 0; j < 4; j++) d[j] *= 0.5f;
  } else if constexpr (RS == 2) {
    float e[4]; unpack4<T>(a2, e);
#pragma unroll
    for (int j = 0; j < 4; j++) d[j] += e[j];
  }
}
template <typename T, int RPT, int RS, bool SILU, int FL>
__global__ __launch_bounds__(NTB) void gn_bwd_resident_full_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, const float* __restrict__ stats,
                                                                   const T* __restrict__ dy, long lddy, T* __restrict__ dx, long lddx,
                                                                   const T* __restrict__ dxr, long lddxr, float* __restrict__ slots,
                                                                   float* __restrict__ colsum_ps, long ldps, int L, int C, int G, int CC,
                                                                   const T* __restrict__ dxr2, long lddxr2, int xcd, int nslot) {
  typedef typename Vec<T, 4>::type V4;
  constexpr bool HAS_DXR = (FL & 1) != 0, HAS_DXR2 = (FL & 2) != 0, HAS_CS = (FL & 4) != 0;
  constexpr int NDY = RS == 2 ? 2 : 1;      // packed gradient rows per row
  __shared__ double redg[2 * RES_MAXG];
  __shared__ double redc[3 * RES_MAXC];
  const int cpg = C / G;
  const ResMap m = resmap<NTB>(CC, C, cpg, xcd);
  const int b = m.b;
  const float* st = stats + ((long)b * G + m.c / cpg) * 2;
  const float mean = st[0], rstd = st[1];
  float ga[4], be[4];
#pragma unroll
  for (int j = 0; j < 4; j++) { ga[j] = gamma[m.c + j]; be[j] = beta[m.c + j]; }
  gn_issue_order();
  V4 raw[RPT], dr[NDY * RPT];
  float d[RPT][4];
  const unsigned cb = (unsigned)m.c * (unsigned)sizeof(T);
  const unsigned ldxb = (unsigned)ldx * (unsigned)sizeof(T), lddyb = (unsigned)lddy * (unsigned)sizeof(T);
  const char* xs = (const char*)(x + (long)b * L * ldx);
  const char* dys = (const char*)(dy + (long)b * dy_rows(L, RS) * lddy);
  const GnDyRow<T, 0> rx(m.ty, m.TY, ldxb, cb);
  const GnDyRow<T, RS> rdy(m.ty, m.TY, lddyb, cb);
#pragma unroll
  for (int k = 0; k < RPT; k++) {
    raw[k] = rx.ld(xs, k, 0);
    dr[NDY * k] = rdy.ld(dys, k, 0);
    if constexpr (RS == 2) dr[2 * k + 1] = rdy.ld(dys, k, lddyb);
    gn_issue_order();      // rows land in the order pass 1 consumes them (hipcc's scheduler moved row 0 to the back of the queue)
  }
  for (int i = threadIdx.x; i < 2 * RES_MAXG + 3 * RES_MAXC; i += NTB) { if (i < 2 * RES_MAXG) redg[i] = 0.0; else redc[i - 2 * RES_MAXG] = 0.0; }
  __syncthreads();
  {
    float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
    const float nmr = -mean * rstd;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      float v[4]; unpack4<T>(raw[k], v);
      gn_dy_eff<T, RS>(dr[NDY * k], dr[NDY * k + NDY - 1], d[k]);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float xh = fmaf(v[j], rstd, nmr);
        float dz = d[k][j];
        if constexpr (SILU) dz *= silu_grad_f(fmaf(ga[j], xh, be[j]));
        d[k][j] = dz;
        dg[j] = fmaf(dz, xh, dg[j]); db[j] += dz;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) { atomicAdd(&redc[m.tx * 4 + j], (double)dg[j]); atomicAdd(&redc[RES_MAXC + m.tx * 4 + j], (double)db[j]); }
  }
#pragma unroll
  for (int k = 0; k < RPT; k++) keep_packed(raw[k]);
  // the first addend's rows, packed: their round trip runs under the two barrier rounds (as in the predicated kernel)
  constexpr bool ER_BATCH = HAS_DXR && !HAS_DXR2 && RS != 2;
  V4 er[ER_BATCH ? RPT : 1];
  const char* dxrs = HAS_DXR ? (const char*)(dxr + (long)b * dy_rows(L, RS) * lddxr) : nullptr;
  const unsigned lddxrb = (unsigned)lddxr * (unsigned)sizeof(T);
  const GnDyRow<T, RS> rer(m.ty, m.TY, lddxrb, cb);
  if constexpr (ER_BATCH) {
#pragma unroll
    for (int k = 0; k < RPT; k++) er[k] = rer.ld(dxrs, k, 0);
  }
  __syncthreads();
  if (m.ty == 0) {
    double p1 = 0.0, p2 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) { p1 += (double)ga[j] * redc[RES_MAXC + m.tx * 4 + j]; p2 += (double)ga[j] * redc[m.tx * 4 + j]; }
    atomicAdd(&redg[2 * m.gl], p1); atomicAdd(&redg[2 * m.gl + 1], p2);
  }
  __syncthreads();
  const double inv_n = gn_inv_n<T>(cpg, L);
  const float m1 = (float)(redg[2 * m.gl] * inv_n), m2 = (float)(redg[2 * m.gl + 1] * inv_n);
  if (slots && m.ty == 0) {
    float* sl = slots + (size_t)(b % nslot) * 2 * C;
#pragma unroll
    for (int j = 0; j < 4; j++) { atomicAdd(&sl[m.c + j], (float)redc[m.tx * 4 + j]); atomicAdd(&sl[C + m.c + j], (float)redc[RES_MAXC + m.tx * 4 + j]); }
  }
  const float rm1 = rstd * m1, rm2 = rstd * m2;
  float gr[4];
#pragma unroll
  for (int j = 0; j < 4; j++) gr[j] = ga[j] * rstd;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  char* dxs = (char*)(dx + (long)b * L * lddx);
  const char* dxr2s = HAS_DXR2 ? (const char*)(dxr2 + (long)b * L * lddxr2) : nullptr;
  const GnDyRow<T, 0> rdx(m.ty, m.TY, (unsigned)lddx * (unsigned)sizeof(T), cb), rdx2(m.ty, m.TY, (unsigned)lddxr2 * (unsigned)sizeof(T), cb);
#pragma unroll
  for (int k = 0; k < RPT; k++) {
    float v[4], o[4]; unpack4<T>(raw[k], v);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float xh = fmaf(v[j], rstd, -mean * rstd);
      o[j] = fmaf(d[k][j], gr[j], fmaf(xh, -rm2, -rm1));
    }
    if constexpr (HAS_DXR) {
      float e[4];
      if constexpr (ER_BATCH) gn_dy_eff<T, RS>(er[k], er[k], e);
      else gn_dy_eff<T, RS>(rer.ld(dxrs, k, 0), rer.ld(dxrs, k, lddxrb), e);
#pragma unroll
      for (int j = 0; j < 4; j++) o[j] += e[j];
    }
    if constexpr (HAS_DXR2) {
      float e[4]; unpack4<T>(rdx2.ld(dxr2s, k, 0), e);
#pragma unroll
      for (int j = 0; j < 4; j++) o[j] += e[j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) cs[j] += o[j];
    store4<T>((T*)(dxs + (size_t)k * rdx.stride + rdx.off), o);
  }
  if constexpr (HAS_CS) {
#pragma unroll
    for (int j = 0; j < 4; j++) atomicAdd(&redc[2 * RES_MAXC + m.tx * 4 + j], (double)cs[j]);
    __syncthreads();
    if (m.ty == 0) {
#pragma unroll
      for (int j = 0; j < 4; j++) colsum_ps[(long)b * ldps + m.c + j] = (float)redc[2 * RES_MAXC + m.tx * 4 + j];
    }
  }
}

// ------------------------------------------------------------------ pipelined form of the one-pass backward (round 4; bf16, resample 0)
// gn_bwd_resident_kernel is a chain per workgroup -- load the slab, pass 1, two barrier rounds, pass 2, store -- and with one 1024-thread
// workgroup per CU nothing overlaps the chain: HBM idles while the VALU runs and the other way round (in the LDM step 47 us per 50 MB
// tensor, 3.2 TB/s for x + dy + dx).  Here ONE persistent workgroup per CU walks slabs of the same size in threads (6 rows of 4 channels
// per thread = 48 KB per tensor), and the NEXT slab's x, dy, residual-path addend and (mean, rstd) pairs are fetched by LDS-DMA into a
// 3 x 48 KB landing area while the current slab is processed from registers: the loads of slab k+1 and the stores of slab k both run
// under the VALU phases.  gfx950 retires loads and stores through one in-order vmcnt, so "slab k+1 has landed" is vmcnt(#stores of slab k)
// = vmcnt(6): every vector-memory instruction a wave issues behind its DMAs is a store or a no-return atomic (gamma / beta are loaded
// once in front of the loop -- a block keeps its channel chunk -- and the statistics arrive by DMA as well), so the compiler never waits on
// vmcnt inside the loop and extra stores of some waves (column sums, slot atomics) only make the counted wait stricter.  Barriers are
// raw s_barrier with lgkmcnt(0): __syncthreads() carries a release fence = s_waitcnt vmcnt(0) = wait for the prefetch.
// Same arithmetic and the same fp64 LDS accumulators as the resident kernel: dx and the per-sample column sums are bit-identical to it.
constexpr int PIPE_RPT = 6;
constexpr int PIPE_SLAB = PIPE_RPT * NTB * 8;                 // bytes of one tensor's slab: 49 152
constexpr int PIPE_OFF_ST = 3 * PIPE_SLAB;                    // 1 KB landing area of the statistics DMA
constexpr int PIPE_OFF_RED = PIPE_OFF_ST + 1024;              // redg[2 * RES_MAXG] | redc[3 * RES_MAXC] (doubles)
constexpr int PIPE_LDS = PIPE_OFF_RED + (2 * RES_MAXG + 3 * RES_MAXC) * 8;      // 155 648 of 163 840

__device__ __forceinline__ void pipe_dma(const void* base, unsigned voff, unsigned lds_off) {      // as gemm_big.hip's dma16s
  const unsigned long long u = (unsigned long long)base;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  const unsigned long long b = ((unsigned long long)hi << 32) | lo;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(__builtin_amdgcn_readfirstlane(lds_off)), "v"(voff), "s"(b) : "memory", "m0");
}
#define PIPE_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#ifdef EEG_STAGE_TIMING      // (make dbg, tools/debug/gn_pipe_timing.py) eight stamps per slab, thread 0, NO memory waits of their own
#define PIPE_TSTAMP(k, i) do { if (threadIdx.x == 0 && (k) < 8) gn_tlog[(size_t)(blockIdx.x % 512) * 64 + (k) * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
#else
#define PIPE_TSTAMP(k, i) do {} while (0)
#endif

template <bool SILU, bool HAS_ER, typename T16 = bf16_t>
__global__ __launch_bounds__(NTB) void gn_bwd_pipe_kernel(const bf16_t* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ stats,
                                                          const bf16_t* __restrict__ dy, long lddy, bf16_t* __restrict__ dx, long lddx,
                                                          const bf16_t* __restrict__ dxr, long lddxr, float* __restrict__ slots,
                                                          float* __restrict__ colsum_ps, long ldps, int B, int L, int C, int G, int CC, int ndg) {
  extern __shared__ __attribute__((aligned(16))) char psm[];
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  double* const redg = (double*)(psm + PIPE_OFF_RED);
  double* const redc = redg + 2 * RES_MAXG;
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned wave_u = __builtin_amdgcn_readfirstlane((unsigned)(tid >> 6));
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr_t)psm;
  const int cpg = C / G, nchunk = C / CC;
  const int TX = CC >> 2, TY = NTB / TX;                  // L == PIPE_RPT * TY: every thread owns exactly PIPE_RPT rows
  const int tx = tid % TX, ty = tid / TX;
  // slab list: workgroup ids = xc (mod 8) run on XCD xc; within an XCD the chunks of one sample are neighbours (they share 128-byte lines
  // when a chunk row is 64 bytes) and a workgroup keeps its chunk for all its samples
  const int xc = blockIdx.x & 7, mb = blockIdx.x >> 3, MB = gridDim.x >> 3;
  const int chunk = mb % nchunk, slot = mb / nchunk, nslot = MB / nchunk;
  const int c = chunk * CC + tx * 4, gl = (tx * 4) / cpg;
  const int noct = B >> 3;
  const int nk = slot < noct ? (noct - slot + nslot - 1) / nslot : 0;
  float ga[4], gl2[4], bl2[4];
#pragma unroll
  for (int j = 0; j < 4; j++) { ga[j] = gamma[c + j]; gl2[j] = ga[j] * 1.4426950408889634f; bl2[j] = beta[c + j] * 1.4426950408889634f; }
  for (int i = tid; i < 2 * RES_MAXG + 3 * RES_MAXC; i += NTB) redg[i] = 0.0;
  // the loads above have to be back before the first DMA: a compiler wait for them behind it would wait for the DMA too
  asm volatile("" :: "v"(ga[0]), "v"(ga[1]), "v"(ga[2]), "v"(ga[3]), "v"(bl2[0]), "v"(bl2[1]), "v"(bl2[2]), "v"(bl2[3]));
  // DMA lane map: 16-byte piece q = (i * 16 + wave) * 64 + lane of the slab, row q / LPR, piece q % LPR; LDS keeps the pieces in q order
  const int LPR = CC >> 3;
  const int drow = (int)(wave_u * 64 + lane) / LPR, dcol = lane % LPR;
  const unsigned vx = (unsigned)drow * (unsigned)ldx * 2u + (unsigned)dcol * 16u, sx = (unsigned)(1024 / LPR) * (unsigned)ldx * 2u;
  const unsigned vd = (unsigned)drow * (unsigned)lddy * 2u + (unsigned)dcol * 16u, sd = (unsigned)(1024 / LPR) * (unsigned)lddy * 2u;
  const unsigned ve = (unsigned)drow * (unsigned)lddxr * 2u + (unsigned)dcol * 16u, se = (unsigned)(1024 / LPR) * (unsigned)lddxr * 2u;
  const unsigned st_bytes = (unsigned)B * (unsigned)G * 8u;
  const unsigned st_sub = ((unsigned)(chunk * (CC / cpg)) * 8u) & 15u;        // (b G + g0) * 8 mod 16: G = 32 makes it independent of b
  // x, dy and the (mean, rstd) pairs of a slab: 7 DMA instructions per wave (every wave fetches the same statistics pieces to the same
  // place, so that all waves count alike); the residual-path addend goes separately: it is read from LDS in pass 2 only
  auto issue_xd = [&](int b) __attribute__((always_inline)) {
    const char* xs = (const char*)(x + (long)b * L * ldx + chunk * CC);
    const char* ds = (const char*)(dy + (long)b * L * lddy + chunk * CC);
#pragma unroll
    for (int i = 0; i < 3; i++) pipe_dma(xs, vx + i * sx, lds0 + (unsigned)(i * 16 + wave_u) * 1024u);
#pragma unroll
    for (int i = 0; i < 3; i++) pipe_dma(ds, vd + i * sd, lds0 + PIPE_SLAB + (unsigned)(i * 16 + wave_u) * 1024u);
    {       // 16-byte pieces from the aligned-down address of the chunk's first pair, clamped to the buffer (the needed pieces never are)
      const unsigned a0 = (((unsigned)b * (unsigned)G + (unsigned)(chunk * (CC / cpg))) * 8u) & ~15u;
      unsigned a = a0 + (unsigned)lane * 16u; if (a > st_bytes - 16u) a = st_bytes - 16u;
      pipe_dma(stats, a, lds0 + PIPE_OFF_ST);
    }
  };
  auto issue_e = [&](int b) __attribute__((always_inline)) {
    const char* es = (const char*)(dxr + (long)b * L * lddxr + chunk * CC);
#pragma unroll
    for (int i = 0; i < 3; i++) pipe_dma(es, ve + i * se, lds0 + 2 * PIPE_SLAB + (unsigned)(i * 16 + wave_u) * 1024u);
  };
  if (nk > 0) { issue_xd(slot * 8 + xc); if constexpr (HAS_ER) issue_e(slot * 8 + xc); }
  const double inv_n = gn_inv_n<T16>(cpg, L);
  const unsigned rowb = (unsigned)CC * 2u;
  const unsigned lrd0 = (unsigned)ty * rowb + (unsigned)tx * 8u, lrds = (unsigned)TY * rowb;      // this thread's piece of row ty; rows step by TY
  const unsigned lddxb = (unsigned)lddx * 2u;
  const unsigned st0 = (unsigned)ty * lddxb + (unsigned)c * 2u, sts = (unsigned)TY * lddxb;      // the same for the dx rows (32-bit offsets off a uniform base)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  for (int k = 0; k < nk; k++) {
    const int b = (slot + k * nslot) * 8 + xc;
    PIPE_TSTAMP(k, 0);
    PIPE_BARRIER();                                           // every wave's pieces of slab k have landed (counted wait at the bottom of slab k-1)
    PIPE_TSTAMP(k, 1);
    uint2 raw[PIPE_RPT], dr[PIPE_RPT];
#pragma unroll
    for (int r = 0; r < PIPE_RPT; r++) {
      const unsigned off = lrd0 + (unsigned)r * lrds;
      raw[r] = *(const uint2*)(psm + off); dr[r] = *(const uint2*)(psm + PIPE_SLAB + off);
    }
    const float2 mr = *(const float2*)(psm + PIPE_OFF_ST + st_sub + (unsigned)gl * 8u);
    PIPE_BARRIER();                                           // everybody holds its copy: the x / dy landing areas may be refilled
    PIPE_TSTAMP(k, 2);
    if (k + 1 < nk) issue_xd((slot + (k + 1) * nslot) * 8 + xc);
    PIPE_TSTAMP(k, 3);
    const float mean = mr.x, rstd = mr.y, nmr = -mean * rstd;
    float d[PIPE_RPT][4];
    {
      // the kernel is VALU-bound (tools/debug/gn_pipe_timing.py: pass 1 is 8 k of a slab's 12.5 k cycles), so SiLU' is taken from
      // t = z log2(e) directly: s = 1 / (1 + 2^-t), SiLU' = s (1 + z (1 - s)) = s fma(t, ln2 (1 - s), 1) -- one multiply less per element
      float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < PIPE_RPT; r++) {
        float v[4]; unpack4<T16>(raw[r], v); unpack4<T16>(dr[r], d[r]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float xh = fmaf(v[j], rstd, nmr);
          float dz = d[r][j];
          if constexpr (SILU) {
            const float t = fmaf(gl2[j], xh, bl2[j]);
            const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-t));
            dz *= sg * fmaf(t, fmaf(-0.6931471805599453f, sg, 0.6931471805599453f), 1.0f);
          }
          d[r][j] = dz;
          dg[j] = fmaf(dz, xh, dg[j]); db[j] += dz;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) { atomicAdd(&redc[tx * 4 + j], (double)dg[j]); atomicAdd(&redc[RES_MAXC + tx * 4 + j], (double)db[j]); }
    }
    PIPE_TSTAMP(k, 4);
    PIPE_BARRIER();
    if (ty == 0) {
      double p1 = 0.0, p2 = 0.0;
#pragma unroll
      for (int j = 0; j < 4; j++) { p1 += (double)ga[j] * redc[RES_MAXC + tx * 4 + j]; p2 += (double)ga[j] * redc[tx * 4 + j]; }
      atomicAdd(&redg[2 * gl], p1); atomicAdd(&redg[2 * gl + 1], p2);
    }
    if constexpr (HAS_ER) {       // this slab's addend (issued at the end of slab k-1) is older than the 7 DMAs of slab k+1
      if (k + 1 < nk) asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    PIPE_BARRIER();
    PIPE_TSTAMP(k, 5);
    {
      const float m1 = (float)(redg[2 * gl] * inv_n), m2 = (float)(redg[2 * gl + 1] * inv_n);
      if (slots && ty == 0) {
        float* sl = slots + (size_t)(b % ndg) * 2 * C;
#pragma unroll
        for (int j = 0; j < 4; j++) { atomicAdd(&sl[c + j], (float)redc[tx * 4 + j]); atomicAdd(&sl[C + c + j], (float)redc[RES_MAXC + tx * 4 + j]); }
      }
      // dx = rstd (dz gamma - m1 - xhat m2), xhat = x rstd + nmr, as two FMAs per element on the raw x: the per-thread constants carry the rest
      const float rm1 = rstd * m1, rm2 = rstd * m2;
      const float a2 = -rm2 * rstd, b2 = fmaf(-rm2, nmr, -rm1);
      float gr[4];
#pragma unroll
      for (int j = 0; j < 4; j++) gr[j] = ga[j] * rstd;
      float cs[4] = {0.f, 0.f, 0.f, 0.f};
      char* dxs = (char*)(dx + (long)b * L * lddx);
#pragma unroll
      for (int r = 0; r < PIPE_RPT; r++) {
        float v[4], o[4]; unpack4<T16>(raw[r], v);
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = fmaf(d[r][j], gr[j], fmaf(v[j], a2, b2));
        if constexpr (HAS_ER) {
          float e[4]; unpack4<T16>(*(const uint2*)(psm + 2 * PIPE_SLAB + lrd0 + (unsigned)r * lrds), e);
#pragma unroll
          for (int j = 0; j < 4; j++) o[j] += e[j];
        }
        if (colsum_ps) {
#pragma unroll
          for (int j = 0; j < 4; j++) cs[j] += o[j];
        }
        store4<T16>((T16*)(dxs + (st0 + (unsigned)r * sts)), o);
      }
      if (colsum_ps) {
#pragma unroll
        for (int j = 0; j < 4; j++) atomicAdd(&redc[2 * RES_MAXC + tx * 4 + j], (double)cs[j]);
      }
    }
    PIPE_TSTAMP(k, 6);
    PIPE_BARRIER();
    if (ty == 0) {       // column sums out, this thread's accumulators back to zero (next touched behind the two barriers at the top of slab k+1)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (colsum_ps) colsum_ps[(long)b * ldps + c + j] = (float)redc[2 * RES_MAXC + tx * 4 + j];
        redc[tx * 4 + j] = 0.0; redc[RES_MAXC + tx * 4 + j] = 0.0; redc[2 * RES_MAXC + tx * 4 + j] = 0.0;
      }
    }
    if (tid < 2 * RES_MAXG) redg[tid] = 0.0;
    // x / dy of slab k+1 have landed when at most this slab's PIPE_RPT stores and the three addend DMAs, all issued behind them, are in flight
    if (k + 1 < nk) {
      if constexpr (HAS_ER) { issue_e((slot + (k + 1) * nslot) * 8 + xc); asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); }
      else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    }
    PIPE_TSTAMP(k, 7);
  }
}


// last forward / backward route (eegldm_debug_gn_last_route: the route-aware tests confirm that a case ran on the kernel it names).
// family: 1 split kernels, 2 resident, 3 pipelined persistent backward, 4 flat G = 1, 5 wide flat forward; vec = 4-wide (1) or scalar (0)
// loads of the split kernels; nth threads per block; rpt the rows-per-thread (flat: chunks-per-thread) instantiation; cc chunk width in
// channels; xcd the XCD-aware block order.  Host-side bookkeeping, one record per host thread (thread_local: the
// read-out reports the calling thread's own last launch), nothing the kernels read.
struct GnRoute { int family, vec, nth, rpt, cc, xcd; };
static thread_local GnRoute g_gn_route[2] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
// body of the last resident backward: 1 the straight-line full-slab kernel, 2 the predicated one; 0 for every other family
static thread_local int g_gn_bwd_body = 0;
inline void gn_note(int bwd, int family, int vec, int nth, int rpt, int cc, int xcd) {
  g_gn_route[bwd] = GnRoute{family, vec, nth, rpt, cc, xcd};
  if (bwd) g_gn_bwd_body = 0;
}

// chunk width for the resident kernels: the widest whole-group chunk (<= 256 channels, dividing C) whose rows fit the
// per-thread register budget; 0 = not eligible (fall back to the split kernels)
int resident_chunk(int L, int C, int G, int resample_pair, int rpt_max, int* rpt_out, int nth = NTB) {
  const int cpg = C / G;
  if (C % 4 != 0 || cpg % 4 != 0) return 0;
  int best = 0, best_rpt = 0;
  for (int mlt = 1; mlt * cpg <= RES_MAXC && mlt <= RES_MAXG; mlt++) {
    const int cc = mlt * cpg;
    if (C % cc != 0) continue;
    const int tx = cc / 4, ty = nth / tx;
    if (ty < 1) break;
    int rpt = resample_pair ? 2 * ((L / 2 + ty - 1) / ty) : (L + ty - 1) / ty;
    if (rpt > rpt_max) break;
    best = cc; best_rpt = rpt;
  }
  *rpt_out = best_rpt;
  return best;
}

// full slab of the 1024-thread resident kernels: the chunk's columns divide the block, and the instantiation's rows per thread times the
// row lanes are exactly L -- every thread is active and no row needs the `l < L` predicate (pair mode: rows 2 * ((k / 2) * TY + ty) + k % 2
// cover [0, RPT * TY) as well, RPT being even; an even TY lets the backward address the half-resolution rows l / 2 as k * TY / 2 + ty / 2)
bool resident_full_slab(int L, int cc, int rpt_inst) {
  const int tx = cc / 4;
  return tx >= 1 && NTB % tx == 0 && (NTB / tx) % 2 == 0 && rpt_inst % 2 == 0 && (long)rpt_inst * (NTB / tx) == L;
}

// f(std::integral_constant<int, v>) for the run-time v in [0, N): turns a small run-time index into a template argument
template <int N, typename F> void gn_static_switch(int v, F&& f) {
  if (v == N - 1) f(std::integral_constant<int, N - 1>());
  else if constexpr (N > 1) gn_static_switch<N - 1>(v, f);
}

// f(GnType<T>()) with T the storage type that `dtype` names: turns the run-time dtype into a template argument
template <typename T> struct GnType { typedef T type; };
template <typename F> int gn_dtype_switch(int dtype, F&& f) {
  if (dtype == EEGLDM_F32) return f(GnType<float>());
  if (dtype == EEGLDM_BF16) return f(GnType<bf16_t>());
  if (dtype == EEGLDM_F16) return f(GnType<f16_t>());
  EEG_FAIL(EEGLDM_ERR_UNSUPPORTED, "dtype %d", dtype);
}

// row-chunk split of one sample: `per_cu` blocks per CU in total, at least `min_rows` rows per block.
// Reductions want few long chunks (fewer atomics), streaming apply kernels want many short ones.
int pick_lsplit(int B, int L, int C, eegldm_ctx* ctx, int* rows_per_block, int per_cu = 8, int min_rows = 16) {
  int want = (ctx->num_cu * per_cu + B - 1) / B;
  int maxsplit = (L + min_rows - 1) / min_rows;
  int ls = want < 1 ? 1 : (want > maxsplit ? maxsplit : want);
  int rpb = (L + ls - 1) / ls;
  *rows_per_block = rpb;
  return (L + rpb - 1) / rpb;
}

// ------------------------------------------------------------------ the resident route, forward and backward: one pick
// {chunk width, rows per thread, threads per block, XCD-aware block order}; cc == 0: not this route (EEGLDM_GN_NO_RESIDENT=1: never)
struct GnResPick { int cc, rpt, nth, xcd; };
inline int gn_block_threads(int asked) { return (asked == 512 || asked == 256) ? asked : 1024; }      // EEGLDM_GN_FWD_NTH / _BWD_NTH
// esize: bytes per element; pair: the avgpool forward (both rows of a pooling pair in one thread); rpt_max: rows per thread the kernel's
// registers hold; blocks_per_cu: the launch must fit that many 1024-thread blocks per CU (callers: what was measured); nth: threads per
// block asked for; few_slab_narrow: the forward's narrowing of launches that leave most of the chip idle
GnResPick gn_resident_pick(const eegldm_ctx* ctx, int B, int L, int C, int G, int esize, bool pair, int rpt_max, long blocks_per_cu, int nth,
                           bool few_slab_narrow) {
  EEG_ENV_VAR(bool, off, getenv("EEGLDM_GN_NO_RESIDENT") != nullptr);
  GnResPick p = {0, 0, nth, 0};
  if (off) return p;
  p.cc = resident_chunk(L, C, G, pair, rpt_max, &p.rpt, nth);
  // a launch that leaves most of the chip idle (sampling one window per call: 1-8 slabs) is a latency chain, not a bandwidth problem:
  // 16-channel slabs on 256 threads are 4x as many, shorter blocks (DDIM-50 at B = 1: 71.5 -> 64.5 ms).  The fp64 group sums make
  // the statistics independent of the slab shape, so the outputs do not change.
  if (few_slab_narrow && p.cc && nth == 1024 && (long)(C / p.cc) * B <= ctx->num_cu / 4) {
    int rpt2 = 0; const int cc2 = resident_chunk(L, C, G, pair, rpt_max, &rpt2, 256);
    if (cc2 && cc2 * esize >= 32) p = GnResPick{cc2, rpt2, 256, 0};
  }
  // rows of at least a 128-byte line; 32-byte rows (16-channel slabs) are fine under the XCD-aware order, which needs B % 8 == 0:
  // L = 3072 runs one-pass (pixel-space step 22.84 -> 22.64 ms)
  const bool can_xcd = B % 8 == 0;
  const int min_row = (p.nth == 1024 && !can_xcd) ? 128 : 32;
  if (p.cc && (p.cc * esize < min_row || (long)(C / p.cc) * B > blocks_per_cu * ctx->num_cu * (1024 / p.nth))) p.cc = 0;
  p.xcd = (p.cc && (p.nth < 1024 || p.cc * esize < 128) && can_xcd) ? 1 : 0;
  return p;
}

// ------------------------------------------------------------------ the dgamma / dbeta slot plan of a backward launch
// Every backward kernel adds its per-channel partials into one of `nslot` rows of 2 C floats, and a fold behind the launch adds the rows
// into dgamma / dbeta and zeroes them again.  Where the rows are, and who folds them:
//   shared     the slot area of the context scratch; folded right behind the launch (gn_slot_reduce_kernel)
//   deferred   a caller that can run the 7-us fold elsewhere (side stream) offers `slots_deferred`: the rows go to the region it names and
//              it calls op_gn_slot_reduce_deferred itself (*slots_deferred = 1)
//   batched    (the UNet backward with grouped weight gradients) the launch gets a region of gn_slot_arena of its OWN and is folded
//              together with all the others by op_gn_fold_flush -- 49 folds of 7 us become one launch (*slots_deferred = 2: nothing left
//              for the caller to fold)
//   private    deterministic mode: det_slots zeroed rows with one writer each (a sample; a block of the split route), folded right behind
//              the launch in row order
struct GnSlots { float* slots = nullptr; int nslot = GN_NSLOT; bool fold64 = false, defer = false, batched = false; };
float* gn_deferred_slots(eegldm_ctx* ctx, int region) { return (float*)((char*)ctx->scratch + gn_slot_region(region)); }

// can_defer: the resident and pipelined routes.  The split and flat routes never defer and never batch, and their deterministic fold stays
// the in-order fp32 one of gn_slot_reduce_kernel over the private rows (the other two fold in fp64, ew_fold_partials_det)
int gn_slots_begin(eegldm_ctx* ctx, float* dgamma, float* dbeta, int C, int det_slots, const int* slots_deferred, int defer_region,
                   bool can_defer, GnSlots* out) {
  GnSlots s;
  *out = s;
  if (!dgamma) return 0;
  const bool det = eeg_deterministic();
  s.fold64 = det && can_defer;
  s.defer = can_defer && slots_deferred && !det;
  s.batched = s.defer && ctx->defer_wgrad && C <= 1024 && ctx->gn_fold_count < GN_FOLD_MAX;
  if (det) {
    s.nslot = det_slots;
    EEG_TRY(eeg_det_buffer(ctx, (size_t)s.nslot * 2 * C * sizeof(float), &s.slots));
    HIP_TRY(hipMemsetAsync(s.slots, 0, (size_t)s.nslot * 2 * C * sizeof(float), ctx->stream));
  } else if (s.batched) {
    if (!ctx->gn_slot_arena) {
      HIP_TRY(hipMalloc(&ctx->gn_slot_arena, (size_t)GN_FOLD_MAX * GN_REGION_FLOATS * sizeof(float)));
      HIP_TRY(hipMemsetAsync(ctx->gn_slot_arena, 0, (size_t)GN_FOLD_MAX * GN_REGION_FLOATS * sizeof(float), ctx->stream));
    }
    s.slots = ctx->gn_slot_arena + (size_t)ctx->gn_fold_count * GN_REGION_FLOATS;
    ctx->gn_fold_pending.push_back({s.slots, dgamma, dbeta, C});
    ctx->gn_fold_count++;
  } else {
    s.slots = s.defer ? gn_deferred_slots(ctx, defer_region) : (float*)((char*)ctx->scratch + GN_SLOT_OFFSET);
  }
  *out = s;
  return 0;
}
// behind the launch.  n_gsums: the split route's group sums at the head of the scratch, zeroed again by the same fold (also without dgamma)
int gn_slots_end(eegldm_ctx* ctx, const GnSlots& s, float* dgamma, float* dbeta, int C, int* slots_deferred, int n_gsums = 0) {
  if (s.fold64) {
    EEG_TRY(ew_fold_partials_det(ctx, s.slots, s.nslot, 2 * C, 0, C, dgamma)); EEG_TRY(ew_fold_partials_det(ctx, s.slots, s.nslot, 2 * C, C, C, dbeta));
  } else if ((s.slots && !s.defer) || n_gsums) {
    const int n = 2 * C > n_gsums ? 2 * C : n_gsums;
    hipLaunchKernelGGL(gn_slot_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, s.slots, dgamma, dbeta, C, (double*)ctx->scratch, n_gsums, s.nslot);
    LAUNCH_CHECK();
  }
  if (s.defer) *slots_deferred = s.batched ? 2 : 1;
  return 0;
}

template <typename T, int V>
int gn_fwd_t(eegldm_ctx* ctx, const void* x, long ldx, const float* gamma, const float* beta, void* y, long ldy,
             float* stats, int B, int L, int C, int G, float eps, int silu, int resample, void* xr, long ldxr) {
  if constexpr (V == 4) {
    // threads per block: 1024 = one (sample, 64-channel) slab per block; 512 / 256 = narrower slabs (32 / 16 channels), 2 / 4x as many
    // independent blocks per CU whose load / reduce / store phases interleave (EEGLDM_GN_FWD_NTH; narrow slabs use the XCD-aware order)
    EEG_ENV_VAR(int, fwd_nth, getenv("EEGLDM_GN_FWD_NTH") ? atoi(getenv("EEGLDM_GN_FWD_NTH")) : 1024);
    EEG_ENV_VAR(bool, no_few, getenv("EEGLDM_GN_NO_FEW_SLAB_NARROW") != nullptr);
    // 12 rows per thread (56 VGPRs: two 1024-thread blocks per CU) measured faster than 24 (one block per CU): 24 vs 35 us.
    // 4 blocks per CU, measured (tools/debug/gn_bench.py): wins while the rows are at least a 128-byte line and the blocks fit two rounds
    // (1024 blocks = the 100 MB concat tensors of the up path: 47-48 us one-pass vs 51 us split)
    const GnResPick p = gn_resident_pick(ctx, B, L, C, G, (int)sizeof(T), resample == 1, 12, 4, gn_block_threads(fwd_nth), !no_few);
    if (p.cc) {
      const dim3 grid((unsigned)((long)(C / p.cc) * B));
      const int r12 = p.rpt <= 6 ? 0 : 1;      // resident_chunk never returns more than 12 rows per thread
      gn_note(0, 2, 1, p.nth, r12 ? 12 : 6, p.cc, p.xcd);
      gn_static_switch<6>(r12 | (p.nth == 1024 ? 0 : p.nth == 512 ? 2 : 4), [&](auto s) {
        constexpr int S = decltype(s)::value, R = (S & 1) ? 12 : 6, N = 1024 >> (S >> 1);
        hipLaunchKernelGGL((gn_fwd_resident_kernel<T, R, N>), grid, dim3(N), 0, ctx->stream, (const T*)x, ldx, gamma, beta,
                           (T*)y, ldy, (T*)xr, ldxr, stats, L, C, G, eps, silu, resample, p.cc, p.xcd);
      });
      LAUNCH_CHECK();
      return 0;
    }
  }
  double* sums = (double*)ctx->scratch;      // zero on entry (context creation / previous finalize)
  int rpb; int ls = pick_lsplit(B, L, C, ctx, &rpb);
  gn_note(0, 1, V == 4, NT, 0, 0, 0);
  hipLaunchKernelGGL((gn_stats_kernel<T, V>), dim3(ls, B), dim3(NT), 0, ctx->stream, (const T*)x, ldx, sums, L, C, G, rpb);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((B * G + 255) / 256), dim3(256), 0, ctx->stream, sums, stats, B * G,
                     (double)(C / G) * (double)L, eps);
  LAUNCH_CHECK();
  int rpb2; int ls2 = pick_lsplit(B, resample == 1 ? L / 2 : L, C, ctx, &rpb2, 16, 8);
  hipLaunchKernelGGL((gn_apply_kernel<T, V>), dim3(ls2, B), dim3(NT), 0, ctx->stream, (const T*)x, ldx, gamma,
                     beta, stats, (T*)y, ldy, (T*)xr, ldxr, L, C, G, silu, resample, rpb2);
  LAUNCH_CHECK();
  return 0;
}

template <typename T, int V>
int gn_bwd_t(eegldm_ctx* ctx, const void* x, long ldx, const float* gamma, const float* beta, const float* stats,
             const void* dy, long lddy, void* dx, long lddx, float* dgamma, float* dbeta, int B, int L, int C, int G,
             int silu, int resample, const void* dxr, long lddxr, float* colsum_ps, long ldps, int* colsum_done,
             const void* dxr2, long lddxr2, int* dxr2_done, int* slots_deferred, int defer_region) {
  if (colsum_done) *colsum_done = 0;
  if (dxr2_done) *dxr2_done = 0;
  if (slots_deferred) *slots_deferred = 0;
  if (!dxr2_done || lddxr2 % 4 != 0) dxr2 = nullptr;      // only a caller that can fall back may hand over a second addend
  GnSlots sl;
  if constexpr (V == 4) {
    EEG_ENV_VAR(int, bwd_nth, getenv("EEGLDM_GN_BWD_NTH") ? atoi(getenv("EEGLDM_GN_BWD_NTH")) : 1024);      // see gn_fwd_t
    // 256-thread blocks (EEGLDM_GN_BWD_NTH=256) measure 42-44 vs 47-49 us on the 50 MB tensors at L <= 384 (tools/debug/gn_nth.py); at step
    // level they gain nothing (19.76 vs 19.67 ms), so the default stays at 1024 threads.
    // HAZARD (the logs of the diagnosis are profiles/r04_hazard_*.txt): until round 4 these blocks returned wrong sums
    // (~1e-3, bf16 rounding flips over whole slabs) whenever they shared a CU with the fused 3-tap weight-gradient GEMM (LDS-DMA build) of
    // another stream -- 1024-thread blocks own a CU and never share it.  The errors sat in EVEN channels only = the low lane of the
    // v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32 instructions hipcc's SLP vectoriser makes of the per-channel math; LDS atomics, LDS stomping
    // and late DMA were not involved.  The library is built with -fno-slp-vectorize -fno-vectorize (Makefile), which removes the error
    // (0 of 108 noisy runs against 27 of 27).  The fence below stays as a second line: narrow blocks are refused whenever anything of this
    // library can run beside them -- the opt-in side stream, or a second live context in this process (g_eeg_live_ctx, api.hip).
    // EEGLDM_GN_NARROW_UNFENCED=1 (developer / regression switch): narrow blocks even beside a second context -- the configuration that
    // returned wrong sums until the library was built without packed-fp32 instructions (tests/test_gpu_concurrency.py runs it)
    EEG_ENV_VAR(bool, unfenced, getenv("EEGLDM_GN_NARROW_UNFENCED") != nullptr);
    const int nth = (unfenced || (!ctx->side_on && g_eeg_live_ctx <= 1)) ? gn_block_threads(bwd_nth) : 1024;
    if constexpr (sizeof(T) == 2) {
      // pipelined persistent form (gn_bwd_pipe_kernel): slabs of exactly 6 rows x 4 channels per thread, L * CC = 24 576, CC a power of two
      EEG_ENV_VAR(bool, off, getenv("EEGLDM_GN_NO_RESIDENT") != nullptr);
      EEG_ENV_VAR(bool, no_pipe, getenv("EEGLDM_GN_NO_PIPE") != nullptr);
      constexpr int pipe_min_row = 64;
      EEG_ENV_VAR(int, pipe_min_slabs, getenv("EEGLDM_GN_PIPE_MIN_SLABS") ? atoi(getenv("EEGLDM_GN_PIPE_MIN_SLABS")) : 2);
      EEG_ENV_VAR(int, pipe_max_slot, getenv("EEGLDM_GN_PIPE_MAX_SLOT") ? atoi(getenv("EEGLDM_GN_PIPE_MAX_SLOT")) : 1 << 20);
      // with a residual-path addend (a fourth 48 KB stream per slab) the kernel is bandwidth-bound like the resident one and measures
      // 3-5 % slower than it (tools/debug/gn_pipe_bench.py): those launches keep the resident kernel unless EEGLDM_GN_PIPE_ADDEND=1
      EEG_ENV_VAR(bool, pipe_addend, getenv("EEGLDM_GN_PIPE_ADDEND") != nullptr);
      const int cpg = C / G;
      const int pcc = (L > 0 && (PIPE_RPT * NTB * 4) % L == 0) ? (PIPE_RPT * NTB * 4) / L : 0;
      const bool pow2 = pcc >= 16 && pcc <= RES_MAXC && (pcc & (pcc - 1)) == 0;
      auto al16 = [](const void* p) { return ((size_t)p & 15) == 0; };
      if (!no_pipe && !off && resample == 0 && !dxr2 && (!dxr || pipe_addend) && pow2 && pcc * 2 >= pipe_min_row && C % pcc == 0 && C % G == 0 && pcc % cpg == 0 &&
          pcc / cpg <= RES_MAXG && cpg % 4 == 0 && (G * 8) % 16 == 0 && B % 8 == 0 && ldx % 8 == 0 && lddy % 8 == 0 && lddx % 4 == 0 &&
          (!dxr || lddxr % 8 == 0) && al16(x) && al16(dy) && al16(stats) && (!dxr || al16(dxr)) && (long)L * (ldx > lddy ? ldx : lddy) * 2 < (1l << 31)) {
        const int nchunk = C / pcc, per_xcd = ctx->num_cu / 8;
        int nslot = per_xcd / nchunk; if (nslot > B / 8) nslot = B / 8; if (nslot > pipe_max_slot) nslot = pipe_max_slot;
        if (nslot >= 1 && (long)nchunk * B >= (long)pipe_min_slabs * 8 * nslot * nchunk) {
          EEG_TRY(gn_slots_begin(ctx, dgamma, dbeta, C, B, slots_deferred, defer_region, true, &sl));
          static DevOnce attr_once;
          if (attr_once.need(ctx->device)) {
            HIP_TRY(hipFuncSetAttribute((const void*)gn_bwd_pipe_kernel<true, true, T>, hipFuncAttributeMaxDynamicSharedMemorySize, PIPE_LDS));
            HIP_TRY(hipFuncSetAttribute((const void*)gn_bwd_pipe_kernel<true, false, T>, hipFuncAttributeMaxDynamicSharedMemorySize, PIPE_LDS));
            HIP_TRY(hipFuncSetAttribute((const void*)gn_bwd_pipe_kernel<false, true, T>, hipFuncAttributeMaxDynamicSharedMemorySize, PIPE_LDS));
            HIP_TRY(hipFuncSetAttribute((const void*)gn_bwd_pipe_kernel<false, false, T>, hipFuncAttributeMaxDynamicSharedMemorySize, PIPE_LDS));
          }
          const dim3 grid((unsigned)(8 * nslot * nchunk));
          gn_note(1, 3, 1, NTB, PIPE_RPT, pcc, 1);
#define GN_BWD_PIPE(SL, ER) hipLaunchKernelGGL((gn_bwd_pipe_kernel<SL, ER, T>), grid, dim3(NTB), PIPE_LDS, ctx->stream, (const bf16_t*)x, ldx, gamma, beta, stats, \
                                           (const bf16_t*)dy, lddy, (bf16_t*)dx, lddx, (const bf16_t*)dxr, lddxr, sl.slots, colsum_ps, ldps, B, L, C, G, pcc, sl.nslot)
          if (silu) { if (dxr) GN_BWD_PIPE(true, true); else GN_BWD_PIPE(true, false); }
          else { if (dxr) GN_BWD_PIPE(false, true); else GN_BWD_PIPE(false, false); }
#undef GN_BWD_PIPE
          LAUNCH_CHECK();
          EEG_TRY(gn_slots_end(ctx, sl, dgamma, dbeta, C, slots_deferred));
          if (colsum_done && colsum_ps) *colsum_done = 1;
          return 0;
        }
      }
    }
    // 8 blocks per CU, measured (tools/debug/gn_bench.py): the one-pass kernel wins while its blocks fit two rounds of one block per CU
    // (1024 blocks: 112 us one-pass vs 117-120 us split on the 100 MB tensors; 2048 blocks of 96-channel chunks lose)
    constexpr int RLO = sizeof(T) == 2 ? 6 : 4, RHI = sizeof(T) == 2 ? 12 : 8;
    const GnResPick p = gn_resident_pick(ctx, B, L, C, G, (int)sizeof(T), false, RHI, 8, nth, false);
    if (p.cc) {
      const dim3 grid((unsigned)((long)(C / p.cc) * B));
      EEG_TRY(gn_slots_begin(ctx, dgamma, dbeta, C, B, slots_deferred, defer_region, true, &sl));
      const int rhi = p.rpt <= RLO ? 0 : 1;
      gn_note(1, 2, 1, p.nth, rhi ? RHI : RLO, p.cc, p.xcd);
      // same route, same geometry; a full slab runs the straight-line body, instantiated for what this launch has (EEGLDM_GN_NO_STREAM=1: never)
      EEG_ENV_VAR(bool, no_stream, getenv("EEGLDM_GN_NO_STREAM") != nullptr);
      const bool full_body = !no_stream && p.nth == NTB && resident_full_slab(L, p.cc, rhi ? RHI : RLO);
      g_gn_bwd_body = full_body ? 1 : 2;
      if (full_body) {
        const int sel = (dxr ? 1 : 0) | (dxr2 ? 2 : 0) | (colsum_ps ? 4 : 0) | (silu ? 8 : 0) | (rhi ? 16 : 0) | ((resample == 1 ? 1 : resample == 2 ? 2 : 0) << 5);
        gn_static_switch<96>(sel, [&](auto s) {
          constexpr int S = decltype(s)::value;
          hipLaunchKernelGGL((gn_bwd_resident_full_kernel<T, (S & 16) ? RHI : RLO, (S / 32), (S & 8) != 0, (S & 7)>), grid, dim3(NTB), 0, ctx->stream,
                             (const T*)x, ldx, gamma, beta, stats, (const T*)dy, lddy, (T*)dx, lddx, (const T*)dxr, lddxr, sl.slots, colsum_ps, ldps,
                             L, C, G, p.cc, (const T*)dxr2, lddxr2, p.xcd, sl.nslot);
        });
      } else {
        // bit 0 rows per thread, 1 RAW0 (resample == 0: the gradient rows fetched packed), 2 SiLU, 3.. threads per block (1024, 512, 256)
        const int sel = rhi | (resample == 0 ? 2 : 0) | (silu ? 4 : 0) | ((p.nth == 1024 ? 0 : p.nth == 512 ? 1 : 2) << 3);
        gn_static_switch<24>(sel, [&](auto s) {
          constexpr int S = decltype(s)::value, N = 1024 >> (S >> 3);
          hipLaunchKernelGGL((gn_bwd_resident_kernel<T, (S & 1) ? RHI : RLO, (S & 2) != 0, (S & 4) != 0, N>), grid, dim3(N), 0, ctx->stream,
                             (const T*)x, ldx, gamma, beta, stats, (const T*)dy, lddy, (T*)dx, lddx, (const T*)dxr, lddxr, sl.slots, colsum_ps, ldps,
                             L, C, G, silu, resample, p.cc, (const T*)dxr2, lddxr2, p.xcd, sl.nslot);
        });
      }
      LAUNCH_CHECK();
      EEG_TRY(gn_slots_end(ctx, sl, dgamma, dbeta, C, slots_deferred));
      if (colsum_done && colsum_ps) *colsum_done = 1;
      if (dxr2) *dxr2_done = 1;
      return 0;
    }
  }
  double* gsums = (double*)ctx->scratch;     // zero on entry; shared with the forward sums (stream-ordered)
  int rpb; int ls = pick_lsplit(B, L, C, ctx, &rpb);
  gn_note(1, 1, V == 4, NT, 0, 0, 0);
  EEG_TRY(gn_slots_begin(ctx, dgamma, dbeta, C, ls * B, nullptr, 0, false, &sl));      // deterministic mode: a slot per block
#define GN_BWD_SPLIT(RS) do { \
    hipLaunchKernelGGL((gn_bwd_reduce_kernel<T, V, RS>), dim3(ls, B), dim3(NT), 0, ctx->stream, (const T*)x, ldx, gamma, beta, stats, \
                       (const T*)dy, lddy, gsums, sl.slots, L, C, G, silu, rpb, sl.nslot); \
    hipLaunchKernelGGL((gn_bwd_apply_kernel<T, V, RS>), dim3(ls2, B), dim3(NT), 0, ctx->stream, (const T*)x, ldx, gamma, \
                       beta, stats, (const T*)dy, lddy, gsums, (T*)dx, lddx, (const T*)dxr, lddxr, L, C, G, silu, rpb2); } while (0)
  int rpb2; int ls2 = pick_lsplit(B, L, C, ctx, &rpb2, 16, 8);
  if (resample == 0) GN_BWD_SPLIT(0); else if (resample == 1) GN_BWD_SPLIT(1); else GN_BWD_SPLIT(2);
#undef GN_BWD_SPLIT
  LAUNCH_CHECK();
  return gn_slots_end(ctx, sl, dgamma, dbeta, C, nullptr, 2 * B * G);      // runs AFTER the apply kernel: it zeroes the group sums too
}

// ------------------------------------------------------------------ thin AutoencoderKL layers: G = 1, C in {1, 2, 4, 8}, contiguous samples
// (config_aekl_eeg_2_2_4_spec.yaml: num_channels [2, 2, 4], norm_num_groups 1).  A sample is one flat run of L*C <= 24576 elements:
// one 256-thread block keeps it in registers as 16-byte chunks of 8 elements (element j of every chunk is channel j % C), so the
// statistics, the normalisation and the whole backward are ONE launch each instead of stats + finalize + apply /
// reduce + apply (2048 blocks of one row per thread and 256-way LDS atomics on these shapes: 40 us for a 1.5 MB tensor).
constexpr int FLAT_NT = 256;
template <typename T> struct Chunk8;
template <> struct Chunk8<bf16_t> {
  typedef uint4 raw_t;
  static __device__ __forceinline__ raw_t load(const bf16_t* p) { return *(const uint4*)p; }
  static __device__ __forceinline__ void unpack(const raw_t& r, float v[8]) {
    v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u); v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
    v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u); v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
  }
  // opaque to the optimiser: keeps the packed chunk (not its eight unpacked floats) live between two passes
  static __device__ __forceinline__ void touch(raw_t& r) { asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w)); }
  static __device__ __forceinline__ void store(bf16_t* p, const float v[8]) {
    uint4 t; t.x = pack_bf16x2(v[0], v[1]); t.y = pack_bf16x2(v[2], v[3]); t.z = pack_bf16x2(v[4], v[5]); t.w = pack_bf16x2(v[6], v[7]);
    *(uint4*)p = t;
  }
};
template <> struct Chunk8<f16_t> {
  typedef uint4 raw_t;
  static __device__ __forceinline__ raw_t load(const f16_t* p) { return *(const uint4*)p; }
  static __device__ __forceinline__ void unpack(const raw_t& r, float v[8]) {
    v[0] = w16_lo<f16_t>(r.x); v[1] = w16_hi<f16_t>(r.x); v[2] = w16_lo<f16_t>(r.y); v[3] = w16_hi<f16_t>(r.y);
    v[4] = w16_lo<f16_t>(r.z); v[5] = w16_hi<f16_t>(r.z); v[6] = w16_lo<f16_t>(r.w); v[7] = w16_hi<f16_t>(r.w);
  }
  static __device__ __forceinline__ void touch(raw_t& r) { asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w)); }
  static __device__ __forceinline__ void store(f16_t* p, const float v[8]) {
    uint4 t; t.x = pack_f16x2(v[0], v[1]); t.y = pack_f16x2(v[2], v[3]); t.z = pack_f16x2(v[4], v[5]); t.w = pack_f16x2(v[6], v[7]);
    *(uint4*)p = t;
  }
};
template <> struct Chunk8<float> {
  struct raw_t { float4 a, b; };
  static __device__ __forceinline__ raw_t load(const float* p) { raw_t r; r.a = *(const float4*)p; r.b = *(const float4*)(p + 4); return r; }
  static __device__ __forceinline__ void unpack(const raw_t& r, float v[8]) {
    v[0] = r.a.x; v[1] = r.a.y; v[2] = r.a.z; v[3] = r.a.w; v[4] = r.b.x; v[5] = r.b.y; v[6] = r.b.z; v[7] = r.b.w;
  }
  static __device__ __forceinline__ void touch(raw_t&) {}
  static __device__ __forceinline__ void store(float* p, const float v[8]) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
};
// sum of K per-thread values over the block (4 waves): result in every thread
template <int K, int NW = 4> __device__ __forceinline__ void flat_block_sum(float (&v)[K], float* sm) {
#pragma unroll
  for (int k = 0; k < K; k++)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) sm[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NW; w += 4) t += (sm[w * K + k] + sm[(w + 1) * K + k]) + (sm[(w + 2) * K + k] + sm[(w + 3) * K + k]);
    v[k] = t;
  }
  __syncthreads();
}

template <typename T, int C, int MAXCH>
__global__ __launch_bounds__(FLAT_NT) void gn_flat_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              T* __restrict__ y, float* __restrict__ stats, int n, float eps, int silu) {
  __shared__ float sm[4];
  const int b = blockIdx.x, tid = threadIdx.x, nch = n >> 3;
  const T* xs = x + (long)b * n; T* ys = y + (long)b * n;
  typename Chunk8<T>::raw_t raw[MAXCH];
#pragma unroll
  for (int k = 0; k < MAXCH; k++) { const int ci = k * FLAT_NT + tid; if (ci < nch) raw[k] = Chunk8<T>::load(xs + (long)ci * 8); }
  // statistics and xhat about the sample's first element pv (one value for the whole block): the fp32 sums and the subtraction of the
  // mean then act on |x - pv| ~ std, not on |x| -- at a mean of m std the uncentred form carries ~2^-24 m of absolute error into xhat,
  // the same on every element of the sample, which an fp16 output shows (tests/test_gpu_groupnorm_rounding.py)
  const float pv = sizeof(T) == 2 ? ld_f32<T>(xs) : 0.f;      // the fp32 engine keeps its uncentred arithmetic (bit-equal outputs)
  float s[1] = {0.f};
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    if (k * FLAT_NT + tid < nch) {
      float v[8]; Chunk8<T>::unpack(raw[k], v);
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] -= pv;
      s[0] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
  }
  flat_block_sum<1>(s, sm);
  const float inv_n = 1.0f / (float)n, md = s[0] * inv_n, mean = pv + md;      // md = mean - pv
  float q[1] = {0.f};
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    if (k * FLAT_NT + tid < nch) {
      float v[8]; Chunk8<T>::unpack(raw[k], v);
#pragma unroll
      for (int j = 0; j < 8; j++) { const float d = (v[j] - pv) - md; q[0] = fmaf(d, d, q[0]); }
    }
  }
  flat_block_sum<1>(q, sm);
  const float rstd = rsqrtf(q[0] * inv_n + eps);
  if (tid == 0) { stats[2 * b] = mean; stats[2 * b + 1] = rstd; }
  float ga[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { ga[j] = gamma[j % C]; be[j] = beta[j % C]; }
  const float nmr = -mean * rstd;
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    const int ci = k * FLAT_NT + tid;
    if (ci < nch) {
      float v[8], o[8]; Chunk8<T>::unpack(raw[k], v);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float xh = sizeof(T) == 2 ? ((v[j] - pv) - md) * rstd : fmaf(v[j], rstd, nmr);
        const float z = fmaf(xh, ga[j], be[j]); o[j] = silu ? silu_f(z) : z;
      }
      Chunk8<T>::store(ys + (long)ci * 8, o);
    }
  }
}

template <typename T, int C, int MAXCH>
__global__ __launch_bounds__(FLAT_NT) void gn_flat_bwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ stats, const T* __restrict__ dy, T* __restrict__ dx,
                                                              const T* __restrict__ dxr, float* __restrict__ slots, int n, int silu, int nslot) {
  __shared__ float sm[4 * 2 * C];
  const int b = blockIdx.x, tid = threadIdx.x, nch = n >> 3;
  const T* xs = x + (long)b * n; const T* dys = dy + (long)b * n; T* dxs = dx + (long)b * n;
  typename Chunk8<T>::raw_t raw[MAXCH], rd[MAXCH];
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    const int ci = k * FLAT_NT + tid;
    if (ci < nch) { raw[k] = Chunk8<T>::load(xs + (long)ci * 8); rd[k] = Chunk8<T>::load(dys + (long)ci * 8); }
  }
  const float mean = stats[2 * b], rstd = stats[2 * b + 1], nmr = -mean * rstd;
  float ga[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { ga[j] = gamma[j % C]; be[j] = beta[j % C]; }
  float dz[MAXCH][8];
  float dg[8], db[8];
#pragma unroll
  for (int j = 0; j < 8; j++) { dg[j] = 0.f; db[j] = 0.f; }
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    if (k * FLAT_NT + tid < nch) {
      float v[8], e[8]; Chunk8<T>::unpack(raw[k], v); Chunk8<T>::unpack(rd[k], e);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float xh = fmaf(v[j], rstd, nmr);
        const float z = silu ? e[j] * silu_grad_f(fmaf(ga[j], xh, be[j])) : e[j];
        dz[k][j] = z; dg[j] = fmaf(z, xh, dg[j]); db[j] += z;
      }
    }
  }
  float r[2 * C];
#pragma unroll
  for (int c = 0; c < C; c++) {
    float a = 0.f, bb = 0.f;
#pragma unroll
    for (int j = c; j < 8; j += C) { a += dg[j]; bb += db[j]; }
    r[c] = a; r[C + c] = bb;
  }
  flat_block_sum<2 * C>(r, sm);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int c = 0; c < C; c++) { s1 = fmaf(ga[c], r[C + c], s1); s2 = fmaf(ga[c], r[c], s2); }
  if (slots && tid == 0) {
    float* sl = slots + (size_t)(b % nslot) * 2 * C;
#pragma unroll
    for (int c = 0; c < 2 * C; c++) atomicAdd(&sl[c], r[c]);
  }
  const float inv_n = 1.0f / (float)n;
  const float rm1 = rstd * s1 * inv_n, rm2 = rstd * s2 * inv_n;
  float gr[8];
#pragma unroll
  for (int j = 0; j < 8; j++) gr[j] = ga[j] * rstd;
  const T* dxrs = dxr ? dxr + (long)b * n : nullptr;
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    const int ci = k * FLAT_NT + tid;
    if (ci < nch) {
      float v[8], o[8]; Chunk8<T>::unpack(raw[k], v);
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = fmaf(dz[k][j], gr[j], fmaf(fmaf(v[j], rstd, nmr), -rm2, -rm1));
      if (dxrs) {
        float e[8]; const typename Chunk8<T>::raw_t t = Chunk8<T>::load(dxrs + (long)ci * 8); Chunk8<T>::unpack(t, e);
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] += e[j];
      }
      Chunk8<T>::store(dxs + (long)ci * 8, o);
    }
  }
}

// Same idea for the [32,32,64] AutoencoderKL (frozen encoder in front of every LDM step, decoder after sampling): G = 1, C a
// multiple of 8 that divides 8192, a sample of up to 98 304 contiguous elements resident in 1024 threads x 12 chunks.  With
// 1024 * 8 a multiple of C every thread always sees the same 8 channels.  1R + 1W instead of the split kernels' 2R + 1W.
constexpr int WIDE_NT = 1024;
template <typename T, int MAXCH>
__global__ __launch_bounds__(WIDE_NT) void gn_flat_fwd_wide_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   T* __restrict__ y, float* __restrict__ stats, int n, int C, float eps, int silu) {
  __shared__ float sm[WIDE_NT / 64];
  const int b = blockIdx.x, tid = threadIdx.x, nch = n >> 3;
  const T* xs = x + (long)b * n; T* ys = y + (long)b * n;
  typename Chunk8<T>::raw_t raw[MAXCH];
#pragma unroll
  for (int k = 0; k < MAXCH; k++) { const int ci = k * WIDE_NT + tid; if (ci < nch) raw[k] = Chunk8<T>::load(xs + (long)ci * 8); }
  // statistics and xhat about the sample's first element pv (one value for the whole block): the fp32 sums and the subtraction of the
  // mean then act on |x - pv| ~ std, not on |x| -- at a mean of m std the uncentred form carries ~2^-24 m of absolute error into xhat,
  // the same on every element of the sample, which an fp16 output shows (tests/test_gpu_groupnorm_rounding.py)
  const float pv = sizeof(T) == 2 ? ld_f32<T>(xs) : 0.f;      // the fp32 engine keeps its uncentred arithmetic (bit-equal outputs)
  float s[1] = {0.f};
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    if (k * WIDE_NT + tid < nch) {
      float v[8]; Chunk8<T>::unpack(raw[k], v);
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] -= pv;
      s[0] += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
  }
  flat_block_sum<1, WIDE_NT / 64>(s, sm);
#pragma unroll
  for (int k = 0; k < MAXCH; k++) Chunk8<T>::touch(raw[k]);
  const float inv_n = 1.0f / (float)n, md = s[0] * inv_n, mean = pv + md;      // md = mean - pv
  float q[1] = {0.f};
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    if (k * WIDE_NT + tid < nch) {
      float v[8]; Chunk8<T>::unpack(raw[k], v);
#pragma unroll
      for (int j = 0; j < 8; j++) { const float d = (v[j] - pv) - md; q[0] = fmaf(d, d, q[0]); }
    }
  }
  flat_block_sum<1, WIDE_NT / 64>(q, sm);
#pragma unroll
  for (int k = 0; k < MAXCH; k++) Chunk8<T>::touch(raw[k]);
  const float rstd = rsqrtf(q[0] * inv_n + eps);
  if (tid == 0) { stats[2 * b] = mean; stats[2 * b + 1] = rstd; }
  const int c0 = (tid * 8) % C;
  float ga[8], be[8];
  { const float4 g0 = *(const float4*)(gamma + c0), g1 = *(const float4*)(gamma + c0 + 4), b0 = *(const float4*)(beta + c0), b1 = *(const float4*)(beta + c0 + 4);
    ga[0] = g0.x; ga[1] = g0.y; ga[2] = g0.z; ga[3] = g0.w; ga[4] = g1.x; ga[5] = g1.y; ga[6] = g1.z; ga[7] = g1.w;
    be[0] = b0.x; be[1] = b0.y; be[2] = b0.z; be[3] = b0.w; be[4] = b1.x; be[5] = b1.y; be[6] = b1.z; be[7] = b1.w; }
  const float nmr = -mean * rstd;
#pragma unroll
  for (int k = 0; k < MAXCH; k++) {
    const int ci = k * WIDE_NT + tid;
    if (ci < nch) {
      float v[8], o[8]; Chunk8<T>::unpack(raw[k], v);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float xh = sizeof(T) == 2 ? ((v[j] - pv) - md) * rstd : fmaf(v[j], rstd, nmr);
        const float z = fmaf(xh, ga[j], be[j]); o[j] = silu ? silu_f(z) : z;
      }
      Chunk8<T>::store(ys + (long)ci * 8, o);
    }
  }
}
bool gn_flat_wide_ok(int L, int C, int G, int resample, long l0, long l1) {
  EEG_ENV_VAR(bool, off, getenv("EEGLDM_GN_NO_FLAT") != nullptr);
  const long n = (long)L * C;
  return !off && G == 1 && resample == 0 && C >= 16 && C % 8 == 0 && (WIDE_NT * 8) % C == 0 && n % 8 == 0 &&
         n <= (long)WIDE_NT * 8 * 12 && l0 == C && l1 == C;
}
template <typename T>
int gn_flat_fwd_wide(eegldm_ctx* ctx, const void* x, const float* gamma, const float* beta, void* y, float* stats, int B, int L, int C, float eps, int silu) {
  const int n = L * C;
  gn_note(0, 5, 1, WIDE_NT, n <= WIDE_NT * 8 * 6 ? 6 : 12, C, 0);
  if (n <= WIDE_NT * 8 * 6) hipLaunchKernelGGL((gn_flat_fwd_wide_kernel<T, 6>), dim3(B), dim3(WIDE_NT), 0, ctx->stream, (const T*)x, gamma, beta, (T*)y, stats, n, C, eps, silu);
  else hipLaunchKernelGGL((gn_flat_fwd_wide_kernel<T, 12>), dim3(B), dim3(WIDE_NT), 0, ctx->stream, (const T*)x, gamma, beta, (T*)y, stats, n, C, eps, silu);
  LAUNCH_CHECK();
  return 0;
}

bool gn_flat_ok(int L, int C, int G, int resample, long l0, long l1, long l2, long l3) {
  EEG_ENV_VAR(bool, off, getenv("EEGLDM_GN_NO_FLAT") != nullptr);
  const long n = (long)L * C;
  return !off && G == 1 && resample == 0 && (C == 1 || C == 2 || C == 4 || C == 8) && n % 8 == 0 && n <= (long)FLAT_NT * 8 * 12 &&
         l0 == C && l1 == C && (l2 == 0 || l2 == C) && (l3 == 0 || l3 == C);
}
template <typename T, int C>
int gn_flat_fwd_c(eegldm_ctx* ctx, const void* x, const float* gamma, const float* beta, void* y, float* stats, int B, int n, float eps, int silu) {
  gn_note(0, 4, 1, FLAT_NT, n <= FLAT_NT * 8 * 3 ? 3 : 12, C, 0);
  if (n <= FLAT_NT * 8 * 3) hipLaunchKernelGGL((gn_flat_fwd_kernel<T, C, 3>), dim3(B), dim3(FLAT_NT), 0, ctx->stream, (const T*)x, gamma, beta, (T*)y, stats, n, eps, silu);
  else hipLaunchKernelGGL((gn_flat_fwd_kernel<T, C, 12>), dim3(B), dim3(FLAT_NT), 0, ctx->stream, (const T*)x, gamma, beta, (T*)y, stats, n, eps, silu);
  LAUNCH_CHECK();
  return 0;
}
template <typename T>
int gn_flat_fwd(eegldm_ctx* ctx, const void* x, const float* gamma, const float* beta, void* y, float* stats, int B, int L, int C, float eps, int silu) {
  switch (C) {
    case 1: return gn_flat_fwd_c<T, 1>(ctx, x, gamma, beta, y, stats, B, L * C, eps, silu);
    case 2: return gn_flat_fwd_c<T, 2>(ctx, x, gamma, beta, y, stats, B, L * C, eps, silu);
    case 4: return gn_flat_fwd_c<T, 4>(ctx, x, gamma, beta, y, stats, B, L * C, eps, silu);
    default: return gn_flat_fwd_c<T, 8>(ctx, x, gamma, beta, y, stats, B, L * C, eps, silu);
  }
}
template <typename T, int C>
int gn_flat_bwd_c(eegldm_ctx* ctx, const void* x, const float* gamma, const float* beta, const float* stats, const void* dy, void* dx, const void* dxr,
                  float* slots, int B, int n, int silu, int nslot) {
  gn_note(1, 4, 1, FLAT_NT, n <= FLAT_NT * 8 * 3 ? 3 : 12, C, 0);
  if (n <= FLAT_NT * 8 * 3) hipLaunchKernelGGL((gn_flat_bwd_kernel<T, C, 3>), dim3(B), dim3(FLAT_NT), 0, ctx->stream, (const T*)x, gamma, beta, stats, (const T*)dy, (T*)dx, (const T*)dxr, slots, n, silu, nslot);
  else hipLaunchKernelGGL((gn_flat_bwd_kernel<T, C, 12>), dim3(B), dim3(FLAT_NT), 0, ctx->stream, (const T*)x, gamma, beta, stats, (const T*)dy, (T*)dx, (const T*)dxr, slots, n, silu, nslot);
  LAUNCH_CHECK();
  return 0;
}
template <typename T>
int gn_flat_bwd(eegldm_ctx* ctx, const void* x, const float* gamma, const float* beta, const float* stats, const void* dy, void* dx, const void* dxr,
                float* dgamma, float* dbeta, int B, int L, int C, int silu) {
  GnSlots sl;
  EEG_TRY(gn_slots_begin(ctx, dgamma, dbeta, C, B, nullptr, 0, false, &sl));
  int rc;
  switch (C) {
    case 1: rc = gn_flat_bwd_c<T, 1>(ctx, x, gamma, beta, stats, dy, dx, dxr, sl.slots, B, L * C, silu, sl.nslot); break;
    case 2: rc = gn_flat_bwd_c<T, 2>(ctx, x, gamma, beta, stats, dy, dx, dxr, sl.slots, B, L * C, silu, sl.nslot); break;
    case 4: rc = gn_flat_bwd_c<T, 4>(ctx, x, gamma, beta, stats, dy, dx, dxr, sl.slots, B, L * C, silu, sl.nslot); break;
    default: rc = gn_flat_bwd_c<T, 8>(ctx, x, gamma, beta, stats, dy, dx, dxr, sl.slots, B, L * C, silu, sl.nslot); break;
  }
  if (rc) return rc;
  return gn_slots_end(ctx, sl, dgamma, dbeta, C, nullptr);
}

int gn_check(eegldm_ctx* ctx, int B, int L, int C, int G, int resample, long ldx) {
  EEG_CHECK(B > 0 && L > 0 && C > 0 && G > 0 && C % G == 0, "bad shape B=%d L=%d C=%d G=%d", B, L, C, G);
  EEG_CHECK(G <= MAXG_LDS && C <= MAXG_LDS, "C, G must be <= %d", MAXG_LDS);
  EEG_CHECK(resample >= 0 && resample <= 2, "resample must be 0/1/2");
  EEG_CHECK(resample != 1 || L % 2 == 0, "avgpool needs even L");
  EEG_CHECK((size_t)B * G * 2 * sizeof(double) <= GN_SLOT_OFFSET, "scratch too small for B*G=%d", B * G);
  return 0;
}
bool vec4_ok(int C, int G, long a, long b, long c, long d) {
  return (C % 4 == 0) && ((C / G) % 4 == 0) && a % 4 == 0 && b % 4 == 0 && c % 4 == 0 && d % 4 == 0;
}

}  // namespace

extern "C" int eegldm_groupnorm_fwd(eegldm_ctx* ctx, const void* x, long ldx, const float* gamma, const float* beta,
                                    void* y, long ldy, float* stats, int B, int L, int C, int G, float eps,
                                    int fuse_silu, int resample, void* xr, long ldxr, int dtype) {
  EEG_TRY(gn_check(ctx, B, L, C, G, resample, ldx));
  const bool flat = gn_flat_ok(L, C, G, resample, ldx, ldy, 0, 0);
  const bool wide = gn_flat_wide_ok(L, C, G, resample, ldx, ldy) && (dtype != EEGLDM_F32 || (long)L * C <= (long)WIDE_NT * 8 * 6);   // fp32: 12 chunks of 8 floats would spill
  const bool v4 = vec4_ok(C, G, ldx, ldy, xr ? ldxr : 0, 0);
  return gn_dtype_switch(dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    if (flat) return gn_flat_fwd<T>(ctx, x, gamma, beta, y, stats, B, L, C, eps, fuse_silu);
    if (wide) return gn_flat_fwd_wide<T>(ctx, x, gamma, beta, y, stats, B, L, C, eps, fuse_silu);
    return v4 ? gn_fwd_t<T, 4>(ctx, x, ldx, gamma, beta, y, ldy, stats, B, L, C, G, eps, fuse_silu, resample, xr, ldxr)
              : gn_fwd_t<T, 1>(ctx, x, ldx, gamma, beta, y, ldy, stats, B, L, C, G, eps, fuse_silu, resample, xr, ldxr);
  });
}

// colsum_ps (optional): per-sample column sums of dx [B][ldps] fp32; *colsum_done tells the caller whether the
// one-pass kernel produced them (otherwise it runs ew_colsum itself)
int op_groupnorm_bwd(eegldm_ctx* ctx, const void* x, long ldx, const float* gamma, const float* beta,
                     const float* stats, const void* dy, long lddy, void* dx, long lddx,
                     float* dgamma, float* dbeta, int B, int L, int C, int G, int fuse_silu,
                     int resample, const void* dxr, long lddxr, int dtype, float* colsum_ps, long ldps, int* colsum_done,
                     const void* dxr2, long lddxr2, int* dxr2_done, int* slots_deferred, int defer_region) {
  if (dxr2_done) *dxr2_done = 0;
  if (slots_deferred) *slots_deferred = 0;
  EEG_TRY(gn_check(ctx, B, L, C, G, resample, ldx));
  const bool flat = gn_flat_ok(L, C, G, resample, ldx, lddy, lddx, dxr ? lddxr : 0);
  const bool v4 = vec4_ok(C, G, ldx, lddy, lddx, dxr ? lddxr : 0);
  if (flat && colsum_done) *colsum_done = 0;
  return gn_dtype_switch(dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    if (flat) return gn_flat_bwd<T>(ctx, x, gamma, beta, stats, dy, dx, dxr, dgamma, dbeta, B, L, C, fuse_silu);
#define GN_BWD_ARGS ctx, x, ldx, gamma, beta, stats, dy, lddy, dx, lddx, dgamma, dbeta, B, L, C, G, fuse_silu, resample, dxr, lddxr, colsum_ps, ldps, colsum_done, dxr2, lddxr2, dxr2_done, slots_deferred, defer_region
    return v4 ? gn_bwd_t<T, 4>(GN_BWD_ARGS) : gn_bwd_t<T, 1>(GN_BWD_ARGS);
#undef GN_BWD_ARGS
  });
}

// folds the second slot area into dgamma / dbeta (and re-zeroes it): the deferred half of op_groupnorm_bwd(..., slots_deferred)
namespace {
__global__ void gn_slot_reduce_multi_kernel(const eegldm_ctx::GnFoldRec* __restrict__ tab) {
  const eegldm_ctx::GnFoldRec r = tab[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * r.C) return;
  float s = 0.f;
  for (int k = 0; k < GN_NSLOT; k++) { s += r.slots[(size_t)k * 2 * r.C + i]; r.slots[(size_t)k * 2 * r.C + i] = 0.f; }
  if (i < r.C) r.dgamma[i] += s; else r.dbeta[i - r.C] += s;
}
}  // namespace
// folds every slot region recorded since the last flush into its dgamma / dbeta (one launch); the device copy of the table is cached
// (the same layers write the same regions step after step) and re-uploaded, after a stream drain, only when it changes
int op_gn_fold_flush(eegldm_ctx* ctx) {
  std::vector<eegldm_ctx::GnFoldRec>& pend = ctx->gn_fold_pending;
  if (pend.empty()) return 0;
  const int first = ctx->gn_fold_count - (int)pend.size();      // table position of this flush's first record
  if (!ctx->gn_fold_dev) HIP_TRY(hipMalloc(&ctx->gn_fold_dev, sizeof(eegldm_ctx::GnFoldRec) * GN_FOLD_MAX));
  if ((int)ctx->gn_fold_host.size() < GN_FOLD_MAX) ctx->gn_fold_host.resize(GN_FOLD_MAX, {nullptr, nullptr, nullptr, 0});
  bool same = true; int maxc = 0;
  for (size_t i = 0; i < pend.size(); i++) {
    const eegldm_ctx::GnFoldRec &a = pend[i], &b = ctx->gn_fold_host[first + i];
    same = same && a.slots == b.slots && a.dgamma == b.dgamma && a.dbeta == b.dbeta && a.C == b.C;
    maxc = a.C > maxc ? a.C : maxc;
  }
  if (!same) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(ctx->gn_fold_dev + first, pend.data(), sizeof(eegldm_ctx::GnFoldRec) * pend.size(), hipMemcpyHostToDevice));
    for (size_t i = 0; i < pend.size(); i++) ctx->gn_fold_host[first + i] = pend[i];
  }
  hipLaunchKernelGGL(gn_slot_reduce_multi_kernel, dim3((2 * maxc + 255) / 256, (unsigned)pend.size()), dim3(256), 0, ctx->stream, ctx->gn_fold_dev + first);
  LAUNCH_CHECK();
  pend.clear();
  return 0;
}

int op_gn_slot_reduce_deferred(eegldm_ctx* ctx, float* dgamma, float* dbeta, int C, int region) {
  hipLaunchKernelGGL(gn_slot_reduce_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, ctx->stream, gn_deferred_slots(ctx, region), dgamma, dbeta, C, (double*)ctx->scratch, 0);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_groupnorm_bwd(eegldm_ctx* ctx, const void* x, long ldx, const float* gamma, const float* beta,
                                    const float* stats, const void* dy, long lddy, void* dx, long lddx,
                                    float* dgamma, float* dbeta, int B, int L, int C, int G, int fuse_silu,
                                    int resample, const void* dxr, long lddxr, int dtype) {
  return op_groupnorm_bwd(ctx, x, ldx, gamma, beta, stats, dy, lddy, dx, lddx, dgamma, dbeta, B, L, C, G, fuse_silu, resample,
                          dxr, lddxr, dtype, nullptr, 0, nullptr);
}

// {family, chunk width, body} of the calling thread's last backward launch, for the ResBlock executor's own record (net.hip)
void gn_last_bwd_route(int out3[3]) { out3[0] = g_gn_route[1].family; out3[1] = g_gn_route[1].cc; out3[2] = g_gn_bwd_body; }

extern "C" int eegldm_debug_gn_last_route(int backward, int* out6_host) {
  if (!out6_host || backward < 0 || backward > 1) return EEGLDM_ERR_INVALID;
  const GnRoute& r = g_gn_route[backward];
  out6_host[0] = r.family; out6_host[1] = r.vec; out6_host[2] = r.nth; out6_host[3] = r.rpt; out6_host[4] = r.cc; out6_host[5] = r.xcd;
  return 0;
}

#ifdef EEG_STAGE_TIMING
extern "C" int eegldm_debug_read_gn_tlog(unsigned long long* dst_host, long n_words) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(dst_host, HIP_SYMBOL(gn_tlog), n_words * 8));
  return 0;
}
#endif
