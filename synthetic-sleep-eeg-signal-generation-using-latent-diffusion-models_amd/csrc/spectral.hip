// Spectral ("Jukebox") loss, forward and gradient in one launch:
//   L = sum_k ( |FFT_ortho(recon)[k]| - |FFT_ortho(target)[k]| )^2      (two-sided, reduction="sum")
// JukeboxLoss(spatial_dims=1, reduction="sum") of the reference's src/train_autoencoderkl.py:158,208
// (MONAI; fftn over dims (1,2) -- with one channel that is a 1-D FFT of the 3072-sample window).
//
// One workgroup per window, everything LDS-resident (N = 3072: the window pair / G, the spectrum and the root table at 24 KB each,
// the padded intermediate at 24.4 KB -- 97 KB, one workgroup per CU):
//   * target and recon are transformed ONE AFTER THE OTHER, each as a real-input DFT (the first stage skips the zero imaginary
//     parts).  Of the target only the amplitudes B_k are kept, in the slots its samples occupied.  The rounding error of an fp32
//     transform is proportional to the norm of what it transforms: packed as ONE complex FFT of recon + i * target (as this kernel
//     once did) the error of R_k was a few 1e-7 of the LARGER window, and a reconstruction 1e-3 of its target -- the first steps of
//     training -- had a gradient wrong by several per cent.  Separately R_k carries a few 1e-7 of recon's own norm, which is what a
//     plain fp32 evaluation achieves (tests/test_gpu_signal_loss_rounding.py, profiles/signal_loss_numerics.txt).
//   * N = 3072 = 48 x 64 is done as a four-step FFT (48-point DFTs down the columns, twiddle,
//     64-point DFTs along the rows) with a sin/cos table of the N-th roots in LDS -- ~112 complex
//     MACs per output, negligible next to the autoencoder, exact to fp32 rounding, no bit reversal.
//   * gradient: dL/d recon[n] = Re FFT_ortho(G)[n], G[k] = 2(A_k - B_k) conj(R_k)/A_k
//     (G_k := 0 where A_k is zero to rounding, A_k^2 <= 1e-10 x the mean bin power of RECON: an exactly-zero A_k comes out of the
//      fp32 transform as rounding noise of ~1e-7 of recon's rms amplitude with a meaningless phase; torch produces NaN there --
//      the reference's README.md:17 notes that instability.  Deviation stated in INTEGRATION.md, tested in tests/test_gpu_aekl.py
//      and tests/test_gpu_signal_loss_rounding.py).
// HBM traffic = the two windows in, one gradient window out: HBM-bound, ~36 KB per window.
#include "common.h"
#include "internal.h"

namespace {
constexpr int NT = 256;

template <int N1, int N2>
struct FFT {
  static constexpr int N = N1 * N2;
  static constexpr int YP = N2 + 1;                    // padded row pitch of the intermediate
  static constexpr int LDS_BYTES = (N + N + N1 * YP) * (int)sizeof(float2);

  // forward DFT (e^{-2 pi i nk/N}) of a[0..N) -> x[0..N), natural order both sides; y is scratch [N1][YP]
  // IN: 0 = the complex a[j]; 1 / 2 = the real signal a[j].x / a[j].y (imaginary part zero: half the products of step 1)
  template <int IN>
  __device__ static void run(const float2* __restrict__ a, float2* __restrict__ x, float2* __restrict__ y, const float2* __restrict__ tw) {
    // step 1+2: Y[k1][n2] = W_N^{n2 k1} * sum_{n1} a[N2 n1 + n2] W_N1^{n1 k1}
    for (int idx = threadIdx.x; idx < N; idx += NT) {
      const int k1 = idx / N2, n2 = idx - k1 * N2;
      float re = 0.f, im = 0.f;
      int t = 0; const int step = (N2 * k1) % N;
#pragma unroll 8
      for (int n1 = 0; n1 < N1; n1++) {
        const float2 v = a[N2 * n1 + n2], w = tw[t];
        if (IN == 0) { re += v.x * w.x - v.y * w.y; im += v.x * w.y + v.y * w.x; }
        else { const float r = IN == 1 ? v.x : v.y; re += r * w.x; im += r * w.y; }
        t += step; if (t >= N) t -= N;
      }
      const float2 w = tw[(n2 * k1) % N];
      y[k1 * YP + n2] = make_float2(re * w.x - im * w.y, re * w.y + im * w.x);
    }
    __syncthreads();
    // step 3: X[k1 + N1 k2] = sum_{n2} Y[k1][n2] W_N2^{n2 k2}
    for (int idx = threadIdx.x; idx < N; idx += NT) {
      const int k2 = idx / N1, k1 = idx - k2 * N1;
      float re = 0.f, im = 0.f;
      int t = 0; const int step = (N1 * k2) % N;
#pragma unroll 8
      for (int n2 = 0; n2 < N2; n2++) {
        const float2 v = y[k1 * YP + n2], w = tw[t];
        re += v.x * w.x - v.y * w.y; im += v.x * w.y + v.y * w.x;
        t += step; if (t >= N) t -= N;
      }
      x[idx] = make_float2(re, im);
    }
    __syncthreads();
  }
};

template <int N1, int N2>
__global__ __launch_bounds__(NT) void spectral_kernel(const float* __restrict__ recon, const float* __restrict__ target, float* __restrict__ loss,
                                                      float* __restrict__ drecon, float gweight, int loss_stride) {
  using F = FFT<N1, N2>;
  constexpr int N = F::N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* bufA = (float2*)smem;
  float2* bufX = bufA + N;
  float2* bufY = bufX + N;
  __shared__ float2 tw[N];        // N-th roots of unity, e^{-2 pi i j/N}
  __shared__ float red[4];
  const long base = (long)blockIdx.x * N;
  const float scale = rsqrtf((float)N);
  float en = 0.f;
  for (int j = threadIdx.x; j < N; j += NT) {
    float s, c; sincospif(-2.0f * (float)j / (float)N, &s, &c);
    tw[j] = make_float2(c, s);
    const float2 z = make_float2(recon[base + j], target[base + j]);
    bufA[j] = z; en += z.x * z.x;
  }
  en = wave_sum(en);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = en;
  __syncthreads();
  // Parseval (ortho norm): sum_k |R_k|^2 = sum_n recon_n^2, so this is 1e-10 x the mean power of a bin of recon
  const float zero_thr = 1e-10f * (red[0] + red[1] + red[2] + red[3]) / (float)N;
  F::template run<2>(bufA, bufX, bufY, tw);      // target: only B_k = |T_k| is needed, kept where the target's samples were
  for (int k = threadIdx.x; k < N; k += NT) { const float tr = scale * bufX[k].x, ti = scale * bufX[k].y; bufA[k].y = sqrtf(tr * tr + ti * ti); }
  __syncthreads();
  F::template run<1>(bufA, bufX, bufY, tw);      // recon
  float part = 0.f;
  for (int k = threadIdx.x; k < N; k += NT) {
    const float rr = scale * bufX[k].x, ri = scale * bufX[k].y;      // R_k
    const float A = sqrtf(rr * rr + ri * ri), Bm = bufA[k].y;
    const float d = A - Bm;
    part += d * d;
    const float g = (A * A > zero_thr) ? 2.0f * d / A : (d != d ? d : 0.f);      // (gated: 0, but a NaN difference stays NaN)
    bufA[k] = make_float2(g * rr, -g * ri);      // G_k = 2(A-B) conj(R_k)/A
  }
  part = wave_sum(part);
  __syncthreads();                       // red[] was read for zero_thr above; G is complete
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss + (size_t)blockIdx.x * loss_stride, red[0] + red[1] + red[2] + red[3]);
  if (drecon) {
    F::template run<0>(bufA, bufX, bufY, tw);
    for (int n = threadIdx.x; n < N; n += NT) drecon[base + n] += gweight * scale * bufX[n].x;
  }
}

template <int N1, int N2>
int launch(eegldm_ctx* ctx, const float* recon, const float* target, float* loss, float* drecon, int B, float w) {
  auto kern = spectral_kernel<N1, N2>;
  constexpr int lds = FFT<N1, N2>::LDS_BYTES;
  static DevOnce attr;
  if (attr.need(ctx->device)) HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  float* dst = loss; int stride = 0;
  if (eeg_deterministic()) {      // a partial per window (zeroed: one writer each), then the windows in order
    EEG_TRY(eeg_det_buffer(ctx, (size_t)B * sizeof(float), &dst)); stride = 1;
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)B * sizeof(float), ctx->stream));
  }
  hipLaunchKernelGGL(kern, dim3(B), dim3(NT), lds, ctx->stream, recon, target, dst, drecon, w, stride);
  LAUNCH_CHECK();
  if (stride) EEG_TRY(ew_fold_partials_det(ctx, dst, B, 1, 0, 1, loss));
  return 0;
}
}  // namespace

// loss (device scalar) = sum over the B windows; d_recon_accum (nullable) += grad_weight * dL/d recon
extern "C" int eegldm_spectral_loss(eegldm_ctx* ctx, const float* recon, const float* target, float* loss, float* d_recon_accum,
                                    int B, int C, int L, float grad_weight) {
  EEG_CHECK(ctx && recon && target && loss && B > 0, "bad argument");
  EEG_CHECK(C == 1, "spectral loss is implemented for single-channel windows (the reference's 1ch x 3072 EEG); got C=%d", C);
  if (!ctx->loss_prezeroed) HIP_TRY(hipMemsetAsync(loss, 0, sizeof(float), ctx->stream));
  if (L == 3072) return launch<48, 64>(ctx, recon, target, loss, d_recon_accum, B, grad_weight);
  if (L == 768) return launch<24, 32>(ctx, recon, target, loss, d_recon_accum, B, grad_weight);
  if (L == 256) return launch<16, 16>(ctx, recon, target, loss, d_recon_accum, B, grad_weight);
  if (L == 96) return launch<8, 12>(ctx, recon, target, loss, d_recon_accum, B, grad_weight);
  EEG_FAIL(EEGLDM_ERR_UNSUPPORTED, "spectral loss window length %d (supported: 3072, 768, 256, 96)", L);
}
