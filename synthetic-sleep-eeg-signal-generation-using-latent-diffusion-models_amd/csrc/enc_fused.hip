// Frozen-encoder fusion (round 3): GroupNorm(G = 1) + SiLU applied on the OPERAND LOAD of the 3-tap conv that consumes it, and the
// per-sample statistics of the NEXT GroupNorm taken from this conv's epilogue -- the normalised tensor is never written to HBM and
// never read back (SURVEY hard part (iv) / VERDICT r2 item 1a, for the one sub-network where nothing has to be saved for a backward:
// the stage-1 AutoencoderKL [32, 32, 64] that train_ldm.py:145-148 runs under no_grad in every LDM step).
//
//   y[b, l, :] = bias + sum_t W[t] . act(x[b, l + t - 1, :])  (+ resid[b, l, :]),   act(v) = silu((v - mean_b) * scale_b[c] + beta[c])
//   scale_b[c] = gamma[c] * rstd_b,    (mean_b, rstd_b) from in_stats[b] = (sum, sum of squares)
//   out_stats[b] += (sum, sum of squares) of the bf16-ROUNDED y -- exactly what a GroupNorm kernel reading the stored tensor would see
//
// Both statistics producers sum in fp32 about a PIVOT p (pre_conv3: per lane, the first of its outputs; sample_stats: the sample's first
// element), D1 = sum (v - p), D2 = sum (v - p)^2, and rebuild sum v = D1 + n p, sum v^2 = D2 + p (2 D1 + n p) in fp64 before the fp64 atomics:
// the fp32 roundings then act on centred magnitudes, and var = S2 / n - mean^2 keeps no 1 + mean^2 / var amplification (one-pass sums about
// zero lost a relative 1e-5 of rstd at a mean of 30 sigma: tests/test_gpu_enc_fused_rounding.py, profiles/enc_fused_numerics.txt).
//
// One block = one tile = 256 consecutive positions of one sample, all output channels (32 or 64).  The (256 + 2) x CI input slab is one contiguous
// run of 16-byte chunks (rows are CI * 2 bytes), transformed in registers, written once to LDS as bf16 (the same rounding point as the
// unfused path, which stores the activated tensor as bf16), and read as MFMA A fragments with the tap as a row shift; the weights
// ([3][CO][CI], 6-24 KB) are register B fragments, 32 output channels at a time.  HBM traffic per layer: x once, y once (was: GroupNorm x -> a, conv a -> y).
// bf16 / fp16 (T16); channel counts {32, 64}; L % 256 == 0.  Everything else keeps the layer-by-layer path (aekl.hip).
#include "common.h"
#include "internal.h"

namespace {

template <typename T16>
__device__ __forceinline__ void mma16e(const uint4& a, const uint4& b, f32x4& acc) {
  if constexpr (Is16<T16>::f16) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
  else acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

constexpr int TR = 256;            // positions per block

template <int CI, int CO, typename T16 = bf16_t>
__global__ __launch_bounds__(256) void pre_conv3_kernel(const bf16_t* __restrict__ x, const double* __restrict__ in_stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const bf16_t* __restrict__ w, const float* __restrict__ bias,
                                                        const bf16_t* __restrict__ resid, bf16_t* __restrict__ y,
                                                        double* __restrict__ out_stats, int L, int ntiles, float eps) {
  constexpr int SEGS = CI / 8;                     // 16-byte chunks per input row
  constexpr int PA = CI * 2 + 16;                  // LDS row pitch (bytes): conflict-free b128 fragment reads
  constexpr int KS = CI / 32;                      // k-steps per tap
  constexpr int NFH = 2, NH = CO / 32;             // output channels in halves of 32 (two 16-column fragments): 48 weight registers at most
  constexpr int NCH = (TR + 2) * SEGS, NLD = (NCH + 255) / 256;
  __shared__ __attribute__((aligned(16))) char at[(TR + 2) * PA];
  const int tid = threadIdx.x, lane = tid & 63, lm = lane & 15, q = lane >> 4, wv = tid >> 6;
  const int tps = L / TR;                          // tiles per sample
  const int seg = tid % SEGS;                      // this thread's chunks all have the same channel segment (256 % SEGS == 0)
  float ga[8], be[8];
#pragma unroll
  for (int e = 0; e < 8; e++) { ga[e] = gamma[seg * 8 + e]; be[e] = beta[seg * 8 + e]; }
  // One block per tile.  (Persistent blocks that keep the NEXT tile's slab in flight in registers were tried: the weights then stay
  // live across the tile loop -- 130-256 VGPRs instead of 84-120, fewer resident blocks -- and the encode took 587 instead of 568 us.)
  uint4 raw[NLD];
  auto load_slab = [&](int tile) __attribute__((always_inline)) {
    const int b = tile / tps, l0 = (tile - b * tps) * TR;
    const bf16_t* xs = x + ((long)b * L + l0 - 1) * CI;
#pragma unroll
    for (int k = 0; k < NLD; k++) {
      const int c = tid + k * 256, l = l0 - 1 + c / SEGS;
      raw[k] = (c < NCH && l >= 0 && l < L) ? *(const uint4*)(xs + (long)c * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  const int tile = blockIdx.x;
  load_slab(tile);
  {
    const int b = tile / tps, l0 = (tile - b * tps) * TR;
    // ---- per-sample normalisation constants of this thread's 8 channels
    float sc[8], sh[8], mh;
    {
      const double n = (double)CI * (double)L;
      const double mean = in_stats[2 * b] / n;
      double var = in_stats[2 * b + 1] / n - mean * mean; if (var < 0.0) var = 0.0;
      const float rstd = (float)(1.0 / sqrt(var + (double)eps));
      // centred apply: z = (x - mh) sc + (beta - ml sc) with mean = mh + ml split into two floats.  x - mh is exact for a 16-bit x near the
      // mean, so every fp32 rounding acts on the centred value (x - mean) sc: the error of z does not grow with |mean| / sigma (a folded
      // shift beta - mean sc is rounded at the magnitude |mean| sc, the same way for every element of a channel)
      mh = (float)mean;
      const double ml = mean - (double)mh;
#pragma unroll
      for (int e = 0; e < 8; e++) { sc[e] = ga[e] * rstd; sh[e] = (float)((double)be[e] - ml * (double)sc[e]); }
    }
    // ---- slab -> act -> LDS.  Row r of the slab is position l0 - 1 + r; rows outside the sample are the conv's zero padding (of the
    // ACTIVATED tensor: zeros, not act(0))
#pragma unroll
    for (int k = 0; k < NLD; k++) {
      const int c = tid + k * 256, r = c / SEGS, l = l0 - 1 + r;
      if (c < NCH) {
        uint4 o = make_uint4(0u, 0u, 0u, 0u);
        if (l >= 0 && l < L) {
          const unsigned in[4] = {raw[k].x, raw[k].y, raw[k].z, raw[k].w};
          unsigned ov[4];
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float v0 = w16_lo<T16>(in[e]) - mh, v1 = w16_hi<T16>(in[e]) - mh;
            ov[e] = pack16x2<T16>(silu_f(fmaf(v0, sc[2 * e], sh[2 * e])), silu_f(fmaf(v1, sc[2 * e + 1], sh[2 * e + 1])));
          }
          o = make_uint4(ov[0], ov[1], ov[2], ov[3]);
        }
        *(uint4*)(at + r * PA + seg * 16) = o;
      }
    }
    __syncthreads();
    // ---- MFMA: wave wv owns rows 64 wv .. + 64 (4 row fragments); tap t reads slab row (row + t); 32 output channels per pass
    float s1 = 0.f, s2 = 0.f, pv = 0.f;      // sums of (r - pv), (r - pv)^2 over this lane's CO outputs; pv = the first of them (row 64 wv + lm, channel 4 q)
#pragma unroll
    for (int h = 0; h < NH; h++) {
      uint4 wf[3][KS][NFH];       // B fragments (n = h*32 + j*16 + lm, k-chunk q of k-step ks, tap t): 6-24 KB of weights, L1 / L2 hits
#pragma unroll
      for (int t = 0; t < 3; t++)
#pragma unroll
        for (int ks = 0; ks < KS; ks++)
#pragma unroll
          for (int j = 0; j < NFH; j++) wf[t][ks][j] = *(const uint4*)(w + ((long)t * CO + h * 32 + j * 16 + lm) * CI + ks * 32 + q * 8);
      f32x4 acc[4][NFH];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < NFH; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 3; t++)
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
          uint4 af[4];
#pragma unroll
          for (int i = 0; i < 4; i++) af[i] = *(const uint4*)(at + (wv * 64 + i * 16 + lm + t) * PA + ks * 64 + q * 16);
#pragma unroll
          for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < NFH; j++) mma16e<T16>(wf[t][ks][j], af[i], acc[i][j]);     // acc[i][j][r] = y[row i*16+lm][col h*32 + j*16 + q*4 + r]
        }
      // ---- epilogue: bias (+ residual), round, statistics of the rounded values, store
#pragma unroll
      for (int j = 0; j < NFH; j++) {
        const int col = h * 32 + j * 16 + q * 4;
        const float4 bv = *(const float4*)(bias + col);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const long row = (long)b * L + l0 + wv * 64 + i * 16 + lm;
          float v[4] = {acc[i][j][0] + bv.x, acc[i][j][1] + bv.y, acc[i][j][2] + bv.z, acc[i][j][3] + bv.w};
          if (resid) {
            const uint2 rr = *(const uint2*)(resid + row * CO + col);
            v[0] += w16_lo<T16>(rr.x); v[1] += w16_hi<T16>(rr.x);
            v[2] += w16_lo<T16>(rr.y); v[3] += w16_hi<T16>(rr.y);
          }
          uint2 o; o.x = pack16x2<T16>(v[0], v[1]); o.y = pack16x2<T16>(v[2], v[3]);
          *(uint2*)(y + row * CO + col) = o;
          if (h == 0 && j == 0 && i == 0) pv = w16_lo<T16>(o.x);
          const float r0 = w16_lo<T16>(o.x) - pv, r1 = w16_hi<T16>(o.x) - pv;
          const float r2 = w16_lo<T16>(o.y) - pv, r3 = w16_hi<T16>(o.y) - pv;
          s1 += (r0 + r1) + (r2 + r3);
          s2 += fmaf(r0, r0, r1 * r1) + fmaf(r2, r2, r3 * r3);
        }
      }
    }
    if (out_stats) {
      // this lane's CO values about its own pivot -> their (sum, sum of squares) in fp64, then the wave in fp64.  (A pivot shared by the wave
      // needs a cross-lane read inside the epilogue; with it hipcc hoists the second half's weight loads: 142 VGPRs instead of 110 at 64 -> 64,
      // and the encode at (256, 3072) took 560 instead of 552 us.  Skipping the arithmetic where out_stats is null, at run time or as a
      // template variant, had the same effect on the registers: 556-571 us.)
      const double p = (double)pv, cnt = (double)CO, d1 = (double)s1;
      double t1 = d1 + cnt * p, t2 = (double)s2 + p * (2.0 * d1 + cnt * p);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) { t1 += __shfl_xor(t1, d, 64); t2 += __shfl_xor(t2, d, 64); }
      if (lane == 0) { atomicAdd(out_stats + 2 * b, t1); atomicAdd(out_stats + 2 * b + 1, t2); }
    }
  }
}

// per-sample (sum, sum of squares) of a stored [B][n] bf16 tensor (n = L * C contiguous): the producers this file does not cover
// (conv_in, the stride-2 downsampling convs) -- read-only, one pass
template <typename T16 = bf16_t>
__global__ __launch_bounds__(256) void sample_stats_kernel(const bf16_t* __restrict__ x, long n, double* __restrict__ stats) {
  const int b = blockIdx.y;
  const uint4* p = (const uint4*)(x + (long)b * n);
  const long nch = n / 8;
  const float pv = w16_lo<T16>(*(const unsigned*)p);      // pivot: the sample's first element (n >= 8)
  float s1 = 0.f, s2 = 0.f; int cnt = 0;                  // sums of (v - pv), (v - pv)^2 and the number of chunks behind them
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nch; c += (long)gridDim.x * 256) {
    const uint4 v = p[c];
    const unsigned in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float v0 = w16_lo<T16>(in[e]) - pv, v1 = w16_hi<T16>(in[e]) - pv;
      s1 += v0 + v1; s2 += fmaf(v0, v0, v1 * v1);
    }
    cnt++;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { s1 += __shfl_xor(s1, d, 64); s2 += __shfl_xor(s2, d, 64); cnt += __shfl_xor(cnt, d, 64); }
  __shared__ float r1[4], r2[4]; __shared__ int rc[4];
  if ((threadIdx.x & 63) == 0) { r1[threadIdx.x >> 6] = s1; r2[threadIdx.x >> 6] = s2; rc[threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double pd = (double)pv, m = 8.0 * (double)(rc[0] + rc[1] + rc[2] + rc[3]);
    const double d1 = (double)r1[0] + (double)r1[1] + (double)r1[2] + (double)r1[3];
    const double d2 = (double)r2[0] + (double)r2[1] + (double)r2[2] + (double)r2[3];
    atomicAdd(stats + 2 * b, d1 + m * pd);
    atomicAdd(stats + 2 * b + 1, d2 + pd * (2.0 * d1 + m * pd));
  }
}

}  // namespace

bool pre_conv3_ok(int dtype, int Cin, int Cout, int L) {
  return (dtype == EEGLDM_BF16 || dtype == EEGLDM_F16) && (Cin == 32 || Cin == 64) && (Cout == 32 || Cout == 64) && L % TR == 0;
}

int pre_conv3_launch(eegldm_ctx* ctx, const void* x, const double* in_stats, const float* gamma, const float* beta, const void* w,
                     const float* bias, const void* resid, void* y, double* out_stats, int B, int L, int Cin, int Cout, float eps, int dtype) {
  EEG_CHECK(pre_conv3_ok(dtype, Cin, Cout, L), "pre_conv3: unsupported shape %d -> %d, L %d", Cin, Cout, L);
  const int ntiles = (L / TR) * B;
#define PRE3T(CI, CO, T) hipLaunchKernelGGL((pre_conv3_kernel<CI, CO, T>), dim3(ntiles), dim3(256), 0, ctx->stream, (const bf16_t*)x, in_stats, gamma, beta, \
                                           (const bf16_t*)w, bias, (const bf16_t*)resid, (bf16_t*)y, out_stats, L, ntiles, eps)
#define PRE3(CI, CO) do { if (dtype == EEGLDM_F16) PRE3T(CI, CO, f16_t); else PRE3T(CI, CO, bf16_t); } while (0)
  if (Cin == 32 && Cout == 32) PRE3(32, 32);
  else if (Cin == 32 && Cout == 64) PRE3(32, 64);
  else if (Cin == 64 && Cout == 64) PRE3(64, 64);
  else PRE3(64, 32);
#undef PRE3
#undef PRE3T
  LAUNCH_CHECK();
  return 0;
}

int sample_stats_launch(eegldm_ctx* ctx, const void* x, long n_per_sample, int B, double* stats, int dtype) {
  EEG_CHECK(n_per_sample % 8 == 0, "sample_stats: samples must be whole 16-byte chunks");
  long per = (n_per_sample / 8 + 255) / 256; if (per > 64) per = 64; if (per < 1) per = 1;
  if (dtype == EEGLDM_F16) hipLaunchKernelGGL(sample_stats_kernel<f16_t>, dim3((unsigned)per, B), dim3(256), 0, ctx->stream, (const bf16_t*)x, n_per_sample, stats);
  else hipLaunchKernelGGL(sample_stats_kernel<bf16_t>, dim3((unsigned)per, B), dim3(256), 0, ctx->stream, (const bf16_t*)x, n_per_sample, stats);
  LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- developer exports: the two kernels alone, behind their eligibility checks
// (tests/test_gpu_enc_fused_rounding.py holds every instantiation to float64; the encoder calls the launchers above directly)
extern "C" int eegldm_debug_pre_conv3(eegldm_ctx* ctx, int dtype, const void* x, const double* in_stats, const float* gamma, const float* beta,
                                      const void* w, const float* bias, const void* resid, void* y, double* out_stats, int B, int L, int Cin,
                                      int Cout, float eps) {
  EEG_CHECK(ctx && x && in_stats && gamma && beta && w && bias && y && B > 0 && L > 0, "bad argument");
  if (!pre_conv3_ok(dtype, Cin, Cout, L)) EEG_FAIL(EEGLDM_ERR_UNSUPPORTED, "pre_conv3: dtype %d, %d -> %d channels, L %d not eligible", dtype, Cin, Cout, L);
  return pre_conv3_launch(ctx, x, in_stats, gamma, beta, w, bias, resid, y, out_stats, B, L, Cin, Cout, eps, dtype);
}
extern "C" int eegldm_debug_sample_stats(eegldm_ctx* ctx, int dtype, const void* x, long n_per_sample, int B, double* stats) {
  EEG_CHECK(ctx && x && stats && B > 0 && n_per_sample > 0, "bad argument");
  if (dtype != EEGLDM_BF16 && dtype != EEGLDM_F16) EEG_FAIL(EEGLDM_ERR_UNSUPPORTED, "sample_stats: 16-bit storage only (dtype %d)", dtype);
  return sample_stats_launch(ctx, x, n_per_sample, B, stats, dtype);
}
