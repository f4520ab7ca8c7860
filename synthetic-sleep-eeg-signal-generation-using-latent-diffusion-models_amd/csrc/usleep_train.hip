// U-Sleep training: the training forward (keeps a tape), the weighted stage cross-entropy and the backward of every layer of usleep.hip.
// fp32, (B, C, L) layout, direct convolutions over flattened (sample, position) rows as in the forward.  A step is launch / HBM bound
// (6.7 MMAC per window forward), so every activation is passed over once per kernel and every reduction is WRITTEN partials folded in a fixed
// order: no float atomics, no memset-then-add, one writer per element -- a step repeats bit for bit.
//
//   usleep_conv_train_kernel<K>   the forward's conv -> + bias -> ELU, writing z and per-(row block, channel) fp64 (sum, sum of squares)
//   usleep_bn_stats_kernel        ordered fold of those -> mean, rstd; running statistics (momentum 0.1, unbiased variance, counter)
//   usleep_bn_apply(_pool)_kernel y = zhat * gamma + beta out of place (z stays for the backward); encoder: + pad / MaxPool(2) in the same pass.
//                                 A NaN in either position of a pooled pair is the pair's maximum, as in torch's max_pool1d
//   usleep_bn_bwd_part / _fold / _apply_kernel   sums of dy and dy * zhat (fp64 partials, ordered fold), dgamma / dbeta +=,
//                                 dz = ELU'(z) * gamma * rstd * (dy - mean(dy) - zhat * mean(dy * zhat))
//   usleep_conv_dgrad_kernel<K>   data gradient of one part (a or b2) of the virtual input; ups: dA[q] = dv[2q] + dv[2q + 1]; cropped positions 0
//   usleep_conv_wgrad_kernel<K>   weight + bias gradient, wave = (4 output channels, 1 input channel, K taps), rows split over blockIdx.z
//   usleep_fold_kernel            grads[i] += sum_p partials[p][i] in the order p = 0, 1, ... (fp64 accumulator)
//   usleep_maxpool_bwd_kernel     gradient to the arg-max (the first NaN of a pair, else the larger; tie: lower padded index; pad wins: dropped)
//                                 + the skip connection's gradient
//   usleep_clf_fwd_train / usleep_ce / usleep_clf_bwd / usleep_clf_dpre_kernel   classifier head and weighted cross-entropy
#include <cmath>
#include <cstring>

#include "usleep.h"

namespace {
constexpr int BN_CHUNK = 2048;     // rows of one (chunk, channel) block of the BatchNorm backward sums

__device__ __forceinline__ float elu_t(float v) { return v > 0.f ? v : expm1f(v); }

// block sum of two doubles in a fixed order: per-thread value -> wave butterfly -> waves 0..3 in order
__device__ __forceinline__ void block_sum2_d(double& a, double& b) {
  __shared__ double red[2][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  a = wave_sum_d(a); b = wave_sum_d(b);
  __syncthreads();
  if (lane == 0) { red[0][wv] = a; red[1][wv] = b; }
  __syncthreads();
  a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

template <int KT>
__global__ __launch_bounds__(UT) void usleep_conv_train_kernel(ConvSrc s, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ z, double* __restrict__ part, long rows, int Cout, int kk, int left) {
  __shared__ float ws[UCI * UKMAX * UCO];                 // [ci][k][co16]
  const int K = KT ? KT : kk;
  const int Cin = s.Ca + s.Cb;
  const int lane = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * UROWS + lane;
  const int co_blk = blockIdx.y * UCO;
  const bool live = row < rows;
  const int b = live ? (int)(row / s.L) : 0, l = live ? (int)(row % s.L) : 0;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ci0 = 0; ci0 < Cin; ci0 += UCI) {
    const int nci = Cin - ci0 < UCI ? Cin - ci0 : UCI;
    __syncthreads();
    for (int i = threadIdx.x; i < nci * K * UCO; i += UT) {
      const int co = i % UCO, ck = i / UCO, c = ck / K, k = ck % K;
      ws[i] = co_blk + co < Cout ? w[((long)(co_blk + co) * Cin + ci0 + c) * K + k] : 0.f;
    }
    __syncthreads();
    if (!live) continue;
    for (int c = 0; c < nci; c++) {
      const int ci = ci0 + c;
      const float* src; int ups = 0;
      if (ci < s.Ca) { src = s.a + ((long)b * s.Ca + ci) * s.La; ups = s.ups; }
      else src = s.b2 + ((long)b * s.Cb + (ci - s.Ca)) * s.Lb;
#pragma unroll
      for (int k = 0; k < (KT ? KT : UKMAX); k++) {
        if (!KT && k >= K) break;
        const int p = l + k - left;
        const float xv = (p >= 0 && p < s.L) ? src[ups ? (p >> 1) : p] : 0.f;
        const float4 wv = *(const float4*)&ws[(c * K + k) * UCO + cg * 4];
        acc[0] = fmaf(wv.x, xv, acc[0]); acc[1] = fmaf(wv.y, xv, acc[1]); acc[2] = fmaf(wv.z, xv, acc[2]); acc[3] = fmaf(wv.w, xv, acc[3]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int co = co_blk + cg * 4 + j;                    // wave-uniform
    if (co >= Cout) break;
    float v = 0.f;
    if (live) { v = elu_t(acc[j] + bias[co]); z[((long)b * Cout + co) * s.L + l] = v; }
    const double sv = wave_sum_d(live ? (double)v : 0.0), sq = wave_sum_d(live ? (double)v * (double)v : 0.0);
    if (lane == 0) { part[((long)blockIdx.x * Cout + co) * 2] = sv; part[((long)blockIdx.x * Cout + co) * 2 + 1] = sq; }   // the one writer of this slot
  }
}

// one block per channel: the row blocks' partials in a fixed order -> mean, rstd, running statistics
__global__ __launch_bounds__(UT) void usleep_bn_stats_kernel(BnDesc d, const double* __restrict__ part, long nblk, float* __restrict__ buffers,
                                                             float* __restrict__ stat, double n, float eps, float momentum) {
  const int c = blockIdx.x;
  double s = 0.0, q = 0.0;
  for (long i = threadIdx.x; i < nblk; i += UT) { s += part[(i * d.C + c) * 2]; q += part[(i * d.C + c) * 2 + 1]; }
  block_sum2_d(s, q);
  if (threadIdx.x == 0) {
    const double mean = s / n;
    double var = q / n - mean * mean; if (var < 0.0) var = 0.0;
    stat[c] = (float)mean; stat[d.C + c] = (float)(1.0 / sqrt(var + (double)eps));
    const double unb = n > 1.0 ? var * n / (n - 1.0) : var;
    buffers[d.rm + c] = (1.f - momentum) * buffers[d.rm + c] + momentum * (float)mean;
    buffers[d.rv + c] = (1.f - momentum) * buffers[d.rv + c] + momentum * (float)unb;
    if (c == 0) buffers[d.nbt] += 1.f;
  }
}
__global__ void usleep_bn_apply_kernel(const float* __restrict__ z, const float* __restrict__ stat, const float* __restrict__ gamma,
                                       const float* __restrict__ beta, float* __restrict__ y, long n, int C, int L) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)((i / L) % C);
    y[i] = fmaf((z[i] - stat[c]) * stat[C + c], gamma[c], beta[c]);
  }
}
// encoder block: the same affine, and ConstantPad1d(1, 0) on both sides at an odd length + MaxPool1d(2) of it, in one pass over z
__global__ void usleep_bn_apply_pool_kernel(const float* __restrict__ z, const float* __restrict__ stat, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ pooled, long nrows, int C, int L, int Lo) {
  const int odd = L & 1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nrows * Lo; i += (long)gridDim.x * blockDim.x) {
    const long r = i / Lo; const int o = (int)(i % Lo), c = (int)(r % C);
    const int p0 = 2 * o - odd, p1 = p0 + 1;             // every p in [0, L) is p0 or p1 of exactly one o
    const float mean = stat[c], rstd = stat[C + c], g = gamma[c], be = beta[c];
    float a = 0.f, b = 0.f;
    if (p0 >= 0 && p0 < L) { a = fmaf((z[r * L + p0] - mean) * rstd, g, be); y[r * L + p0] = a; }
    if (p1 >= 0 && p1 < L) { b = fmaf((z[r * L + p1] - mean) * rstd, g, be); y[r * L + p1] = b; }
    pooled[i] = pool_max(a, b);
  }
}
// dx[p] = dskip[p] + (p is the arg-max of its window ? dpool[window] : 0); the first of two equal values wins, as in torch; a NaN is the
// maximum of its pair (pool_max), so the gradient goes to the first NaN of the pair
__global__ void usleep_maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dpool, const float* __restrict__ dskip,
                                          float* __restrict__ dx, long nrows, int L, int Lo) {
  const int odd = L & 1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nrows * L; i += (long)gridDim.x * blockDim.x) {
    const long r = i / L; const int p = (int)(i % L);
    const int o = (p + odd) >> 1, p0 = 2 * o - odd, p1 = p0 + 1;
    float g = 0.f;
    if (o < Lo) {
      const float a = (p0 >= 0 && p0 < L) ? x[r * L + p0] : 0.f, b = (p1 >= 0 && p1 < L) ? x[r * L + p1] : 0.f;
      const int win = (a != a || a >= b) ? p0 : p1;       // b NaN, a not: a >= b is false
      if (win == p) g = dpool[r * Lo + o];
    }
    dx[i] = dskip ? dskip[i] + g : g;
  }
}

// ---------------------------------------------------------------- ELU + train-mode BatchNorm backward
__global__ __launch_bounds__(UT) void usleep_bn_bwd_part_kernel(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, double* __restrict__ part, long rows, int C, int L) {
  const int c = blockIdx.y;
  const long r0 = (long)blockIdx.x * BN_CHUNK;
  const float mu = mean[c], rs = rstd[c];
  double s1 = 0.0, s2 = 0.0;
  for (int j = 0; j < BN_CHUNK / UT; j++) {
    const long r = r0 + (long)j * UT + threadIdx.x;
    if (r < rows) {
      const long idx = ((r / L) * C + c) * L + r % L;
      const float g = dy[idx], zh = (z[idx] - mu) * rs;
      s1 += (double)g; s2 += (double)g * (double)zh;
    }
  }
  block_sum2_d(s1, s2);
  if (threadIdx.x == 0) { part[((long)blockIdx.x * C + c) * 2] = s1; part[((long)blockIdx.x * C + c) * 2 + 1] = s2; }
}
__global__ void usleep_bn_bwd_fold_kernel(const double* __restrict__ part, long nchunk, float* __restrict__ coef, float* __restrict__ dgamma,
                                          float* __restrict__ dbeta, double n, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (long i = 0; i < nchunk; i++) { s1 += part[(i * C + c) * 2]; s2 += part[(i * C + c) * 2 + 1]; }
  coef[c] = (float)(s1 / n); coef[C + c] = (float)(s2 / n);
  dbeta[c] += (float)s1; dgamma[c] += (float)s2;
}
// (dy and dz may be the same buffer: element i is read before it is written, by the same thread)
__global__ void usleep_bn_bwd_apply_kernel(const float* dy, const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                                           const float* __restrict__ gamma, const float* __restrict__ coef, float* dz, long n, int C, int L) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)((i / L) % C);
    const float zv = z[i], zh = (zv - mean[c]) * rstd[c];
    const float t = (dy[i] - coef[c]) - zh * coef[C + c];
    dz[i] = (zv > 0.f ? 1.f : zv + 1.f) * (gamma[c] * rstd[c]) * t;
  }
}

// ---------------------------------------------------------------- convolution backward
// Data gradient of ONE part of the virtual input: channels [ci_off, ci_off + Csrc) of the conv's Cin, stored (B, Csrc, Lsrc).
// dv[p] = sum_co sum_k w[co][ci][k] * dz[co][p - k + left] for p < L; ups: the part's position q collects p = 2q and 2q + 1.
template <int KT>
__global__ __launch_bounds__(UT) void usleep_conv_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dsrc, long rows,
                                                               int Lsrc, int Csrc, int ci_off, int Cin, int Cout, int L, int ups, int kk, int left) {
  __shared__ float ws[UCI * UKMAX * UCO];                 // [co32][k][ci16]
  const int K = KT ? KT : kk;
  const int lane = threadIdx.x & 63, cg = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * UROWS + lane;
  const int ci_blk = blockIdx.y * UCO;
  const bool live = row < rows;
  const int b = live ? (int)(row / Lsrc) : 0, q = live ? (int)(row % Lsrc) : 0;
  const int npos = ups ? 2 : 1, pbase = ups ? 2 * q : q;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int co0 = 0; co0 < Cout; co0 += UCI) {
    const int nco = Cout - co0 < UCI ? Cout - co0 : UCI;
    __syncthreads();
    for (int i = threadIdx.x; i < nco * K * UCO; i += UT) {
      const int ci = i % UCO, ck = i / UCO, c = ck / K, k = ck % K;
      ws[i] = ci_blk + ci < Csrc ? w[((long)(co0 + c) * Cin + ci_off + ci_blk + ci) * K + k] : 0.f;
    }
    __syncthreads();
    if (!live) continue;
    for (int c = 0; c < nco; c++) {
      const float* dzr = dz + ((long)b * Cout + co0 + c) * L;
#pragma unroll
      for (int k = 0; k < (KT ? KT : UKMAX); k++) {
        if (!KT && k >= K) break;
        float g = 0.f;
        for (int pos = 0; pos < npos; pos++) {
          const int p = pbase + pos, l = p - k + left;
          if (p < L && l >= 0 && l < L) g += dzr[l];
        }
        const float4 wv = *(const float4*)&ws[(c * K + k) * UCO + cg * 4];
        acc[0] = fmaf(wv.x, g, acc[0]); acc[1] = fmaf(wv.y, g, acc[1]); acc[2] = fmaf(wv.z, g, acc[2]); acc[3] = fmaf(wv.w, g, acc[3]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int ci = ci_blk + cg * 4 + j;
    if (ci < Csrc) dsrc[((long)b * Csrc + ci) * Lsrc + q] = acc[j];
  }
}

// Weight and bias gradient.  Wave = 4 output channels x 1 input channel x K taps over the rows [r0, r1) of split blockIdx.z, lane = row:
// a lane's fmaf chain, then the wave butterfly.  accumulate != 0 (one split): out += the sum, else the split's slot is written.
template <int KT>
__global__ __launch_bounds__(UT) void usleep_conv_wgrad_kernel(ConvSrc s, const float* __restrict__ dz, float* __restrict__ outw, float* __restrict__ outb,
                                                               long rows, int Cout, int kk, int left, long rps, long pstride, int accumulate) {
  constexpr int KU = KT ? KT : UKMAX;
  const int K = KT ? KT : kk;
  const int Cin = s.Ca + s.Cb;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int co0 = blockIdx.x * 4, ci = blockIdx.y * 4 + wv;
  if (ci >= Cin) return;                                  // wave-uniform; no block-wide barrier below
  const long r0 = (long)blockIdx.z * rps, r1 = r0 + rps < rows ? r0 + rps : rows;
  const bool do_bias = ci == 0;
  float acc[4][KU], accb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int k = 0; k < KU; k++) acc[j][k] = 0.f;
  const float* base; long cstride; int ups = 0;
  if (ci < s.Ca) { base = s.a + (long)ci * s.La; cstride = (long)s.Ca * s.La; ups = s.ups; }
  else { base = s.b2 + (long)(ci - s.Ca) * s.Lb; cstride = (long)s.Cb * s.Lb; }
  for (long r = r0 + lane; r < r1; r += 64) {
    const int b = (int)(r / s.L), l = (int)(r % s.L);
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; j++) g[j] = co0 + j < Cout ? dz[((long)b * Cout + co0 + j) * s.L + l] : 0.f;
    const float* src = base + (long)b * cstride;
#pragma unroll
    for (int k = 0; k < KU; k++) {
      const int p = l + k - left;
      const float xv = ((KT || k < K) && p >= 0 && p < s.L) ? src[ups ? (p >> 1) : p] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j][k] = fmaf(g[j], xv, acc[j][k]);
    }
    if (do_bias) {
#pragma unroll
      for (int j = 0; j < 4; j++) accb[j] += g[j];
    }
  }
  float* pw = accumulate ? outw : outw + (long)blockIdx.z * pstride;
  float* pb = accumulate ? outb : outw + (long)blockIdx.z * pstride + (long)Cout * Cin * K;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const bool ok = co0 + j < Cout;
#pragma unroll
    for (int k = 0; k < KU; k++) {
      const float t = wave_sum(acc[j][k]);
      if (lane == 0 && ok && (KT || k < K)) { float* d = pw + ((long)(co0 + j) * Cin + ci) * K + k; *d = accumulate ? *d + t : t; }
    }
    if (do_bias) {
      const float t = wave_sum(accb[j]);
      if (lane == 0 && ok) { float* d = pb + co0 + j; *d = accumulate ? *d + t : t; }
    }
  }
}
// dw[i] += sum_p part[p][i] (i < nw), db[i - nw] += sum_p part[p][i] (i >= nw): p = 0, 1, ... in order, fp64 accumulator, one thread per element
__global__ void usleep_fold_kernel(const float* __restrict__ part, int nparts, long pstride, long nw, float* __restrict__ dw, float* __restrict__ db) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pstride) return;
  double t = 0.0;
  for (int p = 0; p < nparts; p++) t += (double)part[(long)p * pstride + i];
  if (i < nw) dw[i] += (float)t; else db[i - nw] += (float)t;
}

// ---------------------------------------------------------------- classifier head and loss
// one block per (sample, pooling window): the forward's usleep_clf_kernel, keeping the pooled tanh `m` and the pre-ELU `h` for the backward
__global__ __launch_bounds__(UT) void usleep_clf_fwd_train_kernel(const float* __restrict__ x, const float* __restrict__ w0, const float* __restrict__ b0,
                                                                  const float* __restrict__ w3, const float* __restrict__ b3, const float* __restrict__ w5,
                                                                  const float* __restrict__ b5, float* __restrict__ y, float* __restrict__ mh, int C1, int L,
                                                                  int win, int S, int ncls) {
  __shared__ float sw[16 * 16 + 16];
  __shared__ double red[4][16];
  const int b = blockIdx.x / S, sidx = blockIdx.x % S;
  for (int i = threadIdx.x; i < C1 * C1; i += UT) sw[i] = w0[i];
  for (int i = threadIdx.x; i < C1; i += UT) sw[256 + i] = b0[i];
  __syncthreads();
  double acc[16];
#pragma unroll
  for (int c = 0; c < 16; c++) acc[c] = 0.0;
  for (int p = sidx * win + threadIdx.x; p < (sidx + 1) * win; p += UT) {
    float xv[16];
#pragma unroll
    for (int c = 0; c < 16; c++) xv[c] = c < C1 ? x[((long)b * C1 + c) * L + p] : 0.f;
#pragma unroll
    for (int co = 0; co < 16; co++) {
      if (co < C1) {
        float v = sw[256 + co];
#pragma unroll
        for (int c = 0; c < 16; c++) if (c < C1) v = fmaf(sw[co * C1 + c], xv[c], v);
        acc[co] += (double)tanhf(v);
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int co = 0; co < 16; co++) { const double t = wave_sum_d(acc[co]); if (lane == 0) red[wv][co] = t; }
  __syncthreads();
  __shared__ float sm[16], sz[16];
  float* t = mh + (long)blockIdx.x * 32;
  if (threadIdx.x < 16) {
    const int co = threadIdx.x;
    const float m = co < C1 ? (float)((((red[0][co] + red[1][co]) + red[2][co]) + red[3][co]) / (double)win) : 0.f;
    sm[co] = m; t[co] = m;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int k = threadIdx.x;
    float v = 0.f;
    if (k < ncls) { v = b3[k]; for (int c = 0; c < C1; c++) v = fmaf(w3[k * C1 + c], sm[c], v); }
    sz[k] = elu_t(v); t[16 + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < ncls) {
    const int k = threadIdx.x;
    float v = b5[k];
    for (int c = 0; c < ncls; c++) v = fmaf(w5[k * ncls + c], sz[c], v);
    y[((long)b * ncls + k) * S + sidx] = v;
  }
}
// F.cross_entropy(logits (B, ncls, S), labels (B, S), weight, ignore_index = any negative label), mean reduction = sum w nll / sum w.
// One block: thread 0 folds the n = B * S windows in order (fp64), then one thread per window writes dlogits.  All ignored: 0, not NaN.
__global__ __launch_bounds__(UT) void usleep_ce_kernel(const float* __restrict__ y, const int64_t* __restrict__ labels, const float* __restrict__ cw,
                                                       float* __restrict__ loss_out, float* __restrict__ dy, int* __restrict__ flag, int B, int ncls, int S,
                                                       float grad_scale) {
  __shared__ double inv_s;
  const int n = B * S;
  if (threadIdx.x == 0) {
    double W = 0.0, Ls = 0.0;
    for (int i = 0; i < n; i++) {
      const int64_t l = labels[i];
      if (l < 0) continue;
      if (l >= ncls) { if (flag) *flag = 1; continue; }   // reported by the host at its next read of the flag; takes no part in the loss
      const int b = i / S, s = i % S;
      double mx = -INFINITY;
      for (int k = 0; k < ncls; k++) { const double v = (double)y[((long)b * ncls + k) * S + s]; mx = v > mx ? v : mx; }
      double se = 0.0;
      for (int k = 0; k < ncls; k++) se += exp((double)y[((long)b * ncls + k) * S + s] - mx);
      const double wl = cw ? (double)cw[l] : 1.0;
      W += wl; Ls += wl * (mx + log(se) - (double)y[((long)b * ncls + l) * S + s]);
    }
    *loss_out = W > 0.0 ? (float)(Ls / W) : 0.f;
    inv_s = W > 0.0 ? (double)grad_scale / W : 0.0;
  }
  __syncthreads();
  if (!dy) return;
  for (int i = threadIdx.x; i < n; i += UT) {
    const int64_t l = labels[i];
    const int b = i / S, s = i % S;
    const bool on = l >= 0 && l < ncls;
    double mx = -INFINITY, se = 0.0;
    for (int k = 0; k < ncls; k++) { const double v = (double)y[((long)b * ncls + k) * S + s]; mx = v > mx ? v : mx; }
    for (int k = 0; k < ncls; k++) se += exp((double)y[((long)b * ncls + k) * S + s] - mx);
    const double sc = on ? inv_s * (cw ? (double)cw[l] : 1.0) : 0.0;
    for (int k = 0; k < ncls; k++) {
      const double pk = exp((double)y[((long)b * ncls + k) * S + s] - mx) / se;
      dy[((long)b * ncls + k) * S + s] = on ? (float)(sc * (pk - (k == l ? 1.0 : 0.0))) : 0.f;
    }
  }
}
// dlogits -> dh (through conv1, ELU), dm (through conv1) per window; then every parameter of clf.3 / clf.5 sums its windows in order.
// One block; dhm: scratch of n * 32 floats (dh [16] | dm [16]).
__global__ __launch_bounds__(UT) void usleep_clf_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ mh, const float* __restrict__ w3,
                                                            const float* __restrict__ w5, float* dhm, float* __restrict__ gw3,
                                                            float* __restrict__ gb3, float* __restrict__ gw5, float* __restrict__ gb5, int B, int C1, int S, int ncls) {
  const int n = B * S;
  for (int i = threadIdx.x; i < n; i += UT) {
    const int b = i / S, s = i % S;
    for (int k = 0; k < ncls; k++) {
      float v = 0.f;
      for (int j = 0; j < ncls; j++) v = fmaf(w5[j * ncls + k], dy[((long)b * ncls + j) * S + s], v);
      const float h = mh[(long)i * 32 + 16 + k];
      dhm[(long)i * 32 + k] = v * (h > 0.f ? 1.f : expm1f(h) + 1.f);
    }
    for (int c = 0; c < C1; c++) {                        // (reads back what this thread has just written)
      float v = 0.f;
      for (int k = 0; k < ncls; k++) v = fmaf(w3[k * C1 + c], dhm[(long)i * 32 + k], v);
      dhm[(long)i * 32 + 16 + c] = v;
    }
  }
  __syncthreads();
  const int n5 = ncls * ncls, n3 = ncls * C1;
  for (int e = threadIdx.x; e < n5 + ncls + n3 + ncls; e += UT) {
    float t = 0.f;
    if (e < n5) {                                          // gw5[k][c] += sum_i dy[i][k] * elu(h[i][c])
      const int k = e / ncls, c = e % ncls;
      for (int i = 0; i < n; i++) t = fmaf(dy[((long)(i / S) * ncls + k) * S + i % S], elu_t(mh[(long)i * 32 + 16 + c]), t);
      gw5[e] += t;
    } else if (e < n5 + ncls) {
      const int k = e - n5;
      for (int i = 0; i < n; i++) t += dy[((long)(i / S) * ncls + k) * S + i % S];
      gb5[k] += t;
    } else if (e < n5 + ncls + n3) {                       // gw3[k][c] += sum_i dh[i][k] * m[i][c]
      const int k = (e - n5 - ncls) / C1, c = (e - n5 - ncls) % C1;
      for (int i = 0; i < n; i++) t = fmaf(dhm[(long)i * 32 + k], mh[(long)i * 32 + c], t);
      gw3[k * C1 + c] += t;
    } else {
      const int k = e - n5 - ncls - n3;
      for (int i = 0; i < n; i++) t += dhm[(long)i * 32 + k];
      gb3[k] += t;
    }
  }
}
// gradient at the output of clf.0 (before tanh): dpre[b][co][p] = dm[window][co] / win * (1 - tanh^2); positions past S * win get 0
__global__ __launch_bounds__(UT) void usleep_clf_dpre_kernel(const float* __restrict__ x, const float* __restrict__ w0, const float* __restrict__ b0,
                                                             const float* __restrict__ dhm, float* __restrict__ dpre, long rows, int C1, int L, int win, int S) {
  __shared__ float sw[16 * 16 + 16];
  for (int i = threadIdx.x; i < C1 * C1; i += UT) sw[i] = w0[i];
  for (int i = threadIdx.x; i < C1; i += UT) sw[256 + i] = b0[i];
  __syncthreads();
  const long row = (long)blockIdx.x * UT + threadIdx.x;
  if (row >= rows) return;
  const int b = (int)(row / L), p = (int)(row % L);
  const bool in = p < S * win;
  float xv[16];
#pragma unroll
  for (int c = 0; c < 16; c++) xv[c] = (in && c < C1) ? x[((long)b * C1 + c) * L + p] : 0.f;
  const float* dm = dhm + ((long)b * S + (in ? p / win : 0)) * 32 + 16;
  const float iw = 1.f / (float)win;
#pragma unroll
  for (int co = 0; co < 16; co++) {
    if (co < C1) {
      float v = sw[256 + co];
#pragma unroll
      for (int c = 0; c < 16; c++) if (c < C1) v = fmaf(sw[co * C1 + c], xv[c], v);
      const float t = tanhf(v);
      dpre[((long)b * C1 + co) * L + p] = in ? dm[co] * iw * (1.f - t * t) : 0.f;
    }
  }
}

// ================================================================ host side
inline unsigned ew_blocks(long n) { const long b = (n + 255) / 256; return (unsigned)(b < 1 ? 1 : (b < 4096 ? b : 4096)); }
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

#define KSWITCH(K, M) \
  switch (K) { case 1: M(1); break; case 2: M(2); break; case 3: M(3); break; case 5: M(5); break; case 7: M(7); break; \
               case 9: M(9); break; case 11: M(11); break; default: M(0); break; }

int src_check(const ConvSrc& s, int K) {
  EEG_CHECK(s.a && s.Ca >= 1 && s.La >= 1 && s.L >= 1 && s.L <= (s.ups ? 2 * s.La : s.La), "virtual input: part a (C=%d, L=%d, ups=%d) against L=%d", s.Ca, s.La, s.ups, s.L);
  EEG_CHECK(s.Cb == 0 || (s.b2 && s.Lb >= s.L), "virtual input: part b2 (C=%d, L=%d) against L=%d", s.Cb, s.Lb, s.L);
  EEG_CHECK(K >= 1 && K <= UKMAX, "kernel size %d not in 1..%d", K, UKMAX);
  return 0;
}

// splits of the weight gradient's rows: enough blocks to fill the chip, at least 256 rows (4 per lane) each
int auto_split(long rows, int Cout, int Cin) {
  const long tiles = (long)((Cout + 3) / 4) * ((Cin + 3) / 4);
  long ns = 1024 / tiles; if (ns < 1) ns = 1;
  const long cap = (rows + 255) / 256;
  if (ns > cap) ns = cap;
  if (ns > 1024) ns = 1024;
  return (int)(ns < 1 ? 1 : ns);
}
size_t wgrad_scratch_bytes(int nsplit, int Cout, int Cin, int K) { return nsplit > 1 ? sizeof(float) * (size_t)nsplit * ((size_t)Cout * Cin * K + Cout) : 0; }

// dw += , db += over the rows of the virtual input; scratch: wgrad_scratch_bytes(nsplit, ...)
int conv_wgrad(eegldm_ctx* ctx, const ConvSrc& s, const float* dz, int B, int Cout, int K, int nsplit, float* scratch, float* dw, float* db, long* launches) {
  const long rows = (long)B * s.L;
  const int Cin = s.Ca + s.Cb, left = (K - 1) / 2;
  const long nw = (long)Cout * Cin * K, pstride = nw + Cout;
  const long rps = (rows + nsplit - 1) / nsplit;
  nsplit = (int)((rows + rps - 1) / rps);
  const dim3 grid((unsigned)((Cout + 3) / 4), (unsigned)((Cin + 3) / 4), (unsigned)nsplit);
  const int acc = nsplit == 1;
#define WL(KT) hipLaunchKernelGGL((usleep_conv_wgrad_kernel<KT>), grid, dim3(UT), 0, ctx->stream, s, dz, acc ? dw : scratch, db, rows, Cout, K, left, rps, pstride, acc)
  KSWITCH(K, WL)
#undef WL
  LAUNCH_CHECK(); ++*launches;
  if (!acc) {
    hipLaunchKernelGGL(usleep_fold_kernel, dim3((unsigned)((pstride + 255) / 256)), dim3(256), 0, ctx->stream, scratch, nsplit, pstride, nw, dw, db);
    LAUNCH_CHECK(); ++*launches;
  }
  return 0;
}
int conv_dgrad_part(eegldm_ctx* ctx, const float* dz, const float* w, float* dsrc, int B, int Lsrc, int Csrc, int ci_off, int Cin, int Cout, int L, int ups,
                    int K, long* launches) {
  const long rows = (long)B * Lsrc;
  const int left = (K - 1) / 2;
  const dim3 grid((unsigned)((rows + UROWS - 1) / UROWS), (unsigned)((Csrc + UCO - 1) / UCO));
#define DL(KT) hipLaunchKernelGGL((usleep_conv_dgrad_kernel<KT>), grid, dim3(UT), 0, ctx->stream, dz, w, dsrc, rows, Lsrc, Csrc, ci_off, Cin, Cout, L, ups, K, left)
  KSWITCH(K, DL)
#undef DL
  LAUNCH_CHECK(); ++*launches;
  return 0;
}
size_t bn_bwd_scratch_bytes(long rows, int C) { return up256(sizeof(double) * 2 * (size_t)((rows + BN_CHUNK - 1) / BN_CHUNK) * C) + up256(sizeof(float) * 2 * C); }
int elu_bn_bwd(eegldm_ctx* ctx, const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma, float* dz, float* dgamma,
               float* dbeta, int B, int C, int L, char* scratch, long* launches) {
  const long rows = (long)B * L, nchunk = (rows + BN_CHUNK - 1) / BN_CHUNK, n = rows * C;
  double* part = (double*)scratch;
  float* coef = (float*)(scratch + up256(sizeof(double) * 2 * (size_t)nchunk * C));
  hipLaunchKernelGGL(usleep_bn_bwd_part_kernel, dim3((unsigned)nchunk, (unsigned)C), dim3(UT), 0, ctx->stream, dy, z, mean, rstd, part, rows, C, L);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(usleep_bn_bwd_fold_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, ctx->stream, part, nchunk, coef, dgamma, dbeta, (double)rows, C);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(usleep_bn_bwd_apply_kernel, dim3(ew_blocks(n)), dim3(256), 0, ctx->stream, dy, z, mean, rstd, gamma, coef, dz, n, C, L);
  LAUNCH_CHECK();
  *launches += 3;
  return 0;
}
int maxpool_bwd(eegldm_ctx* ctx, const float* x, const float* dpool, const float* dskip, float* dx, long nrows, int L, long* launches) {
  const int Lo = (L + ((L & 1) ? 2 : 0)) / 2;
  hipLaunchKernelGGL(usleep_maxpool_bwd_kernel, dim3(ew_blocks(nrows * L)), dim3(256), 0, ctx->stream, x, dpool, dskip, dx, nrows, L, Lo);
  LAUNCH_CHECK(); ++*launches;
  return 0;
}

struct ClfW { const float *w0, *b0, *w3, *b3, *w5, *b5; };
struct ClfG { float *w0, *b0, *w3, *b3, *w5, *b5; };
int clf_forward(eegldm_ctx* ctx, const float* x, const ClfW& P, float* y, float* mh, int B, int C1, int L, int win, int S, int ncls, long* launches) {
  hipLaunchKernelGGL(usleep_clf_fwd_train_kernel, dim3((unsigned)(B * S)), dim3(UT), 0, ctx->stream, x, P.w0, P.b0, P.w3, P.b3, P.w5, P.b5, y, mh, C1, L, win, S, ncls);
  LAUNCH_CHECK(); ++*launches;
  return 0;
}
int ce_loss(eegldm_ctx* ctx, const float* y, const int64_t* labels, const float* cw, float* loss_out, float* dy, int* flag, int B, int ncls, int S, float gs,
            long* launches) {
  hipLaunchKernelGGL(usleep_ce_kernel, dim3(1), dim3(UT), 0, ctx->stream, y, labels, cw, loss_out, dy, flag, B, ncls, S, gs);
  LAUNCH_CHECK(); ++*launches;
  return 0;
}
size_t clf_bwd_scratch_bytes(int B, int C1, int L, int S, int nsplit) {
  return up256(sizeof(float) * 32 * (size_t)B * S) + up256(sizeof(float) * (size_t)B * C1 * L) + up256(wgrad_scratch_bytes(nsplit, C1, C1, 1));
}
// dlogits -> the six parameter gradients (+=) and d(decoder output) (written; 0 past S * win)
int clf_backward(eegldm_ctx* ctx, const float* x, const ClfW& P, const ClfG& G, const float* dy, const float* mh, float* dx, int B, int C1, int L, int win, int S,
                 int ncls, int nsplit, char* scratch, long* launches) {
  float* dhm = (float*)scratch;
  float* dpre = (float*)(scratch + up256(sizeof(float) * 32 * (size_t)B * S));
  float* wpart = (float*)((char*)dpre + up256(sizeof(float) * (size_t)B * C1 * L));
  hipLaunchKernelGGL(usleep_clf_bwd_kernel, dim3(1), dim3(UT), 0, ctx->stream, dy, mh, P.w3, P.w5, dhm, G.w3, G.b3, G.w5, G.b5, B, C1, S, ncls);
  LAUNCH_CHECK();
  const long rows = (long)B * L;
  hipLaunchKernelGGL(usleep_clf_dpre_kernel, dim3((unsigned)((rows + UT - 1) / UT)), dim3(UT), 0, ctx->stream, x, P.w0, P.b0, dhm, dpre, rows, C1, L, win, S);
  LAUNCH_CHECK();
  *launches += 2;
  const ConvSrc s = {x, C1, L, 0, nullptr, 0, 0, L};
  EEG_TRY(conv_wgrad(ctx, s, dpre, B, C1, 1, nsplit, wpart, G.w0, G.b0, launches));
  if (dx) EEG_TRY(conv_dgrad_part(ctx, dpre, P.w0, dx, B, L, C1, 0, C1, C1, L, 0, 1, launches));
  return 0;
}

// (the layer helpers take plain pointers: the model passes slices of its flat parameter / buffer arrays, usleep_layer_train_entry its own)
int launch_conv_train(eegldm_ctx* ctx, const ConvSrc& s, const float* w, const float* bias, int cout, int k, int left, float* z, double* part, int B,
                      long* launches) {
  const long rows = (long)B * s.L;
  const dim3 grid((unsigned)((rows + UROWS - 1) / UROWS), (unsigned)((cout + UCO - 1) / UCO));
#define TL(KT) hipLaunchKernelGGL((usleep_conv_train_kernel<KT>), grid, dim3(UT), 0, ctx->stream, s, w, bias, z, part, rows, cout, k, left)
  KSWITCH(k, TL)
#undef TL
  LAUNCH_CHECK(); ++*launches;
  return 0;
}
inline int pooled_len(int L) { return (L + ((L & 1) ? 2 : 0)) / 2; }
// conv -> ELU -> train-mode BatchNorm of one layer: z, stat (mean | rstd) and y (B, cout, L) written, the running statistics at d's offsets in
// `buffers` updated; pooled != nullptr (B, cout, pooled_len(L)): the encoder's pad + MaxPool(2) rides on the affine pass
int conv_elu_bn_train(eegldm_ctx* ctx, const ConvSrc& s, const float* w, const float* bias, int cout, int k, const BnDesc& d, const float* gamma,
                      const float* beta, float* buffers, float* z, float* stat, float* y, float* pooled, int B, long* launches) {
  const long rows = (long)B * s.L, n = rows * cout, nblk = (rows + UROWS - 1) / UROWS;
  float* scratch; EEG_TRY(eeg_det_buffer(ctx, sizeof(double) * 2 * (size_t)nblk * cout, &scratch));
  double* part = (double*)scratch;
  EEG_TRY(launch_conv_train(ctx, s, w, bias, cout, k, (k - 1) / 2, z, part, B, launches));
  hipLaunchKernelGGL(usleep_bn_stats_kernel, dim3((unsigned)cout), dim3(UT), 0, ctx->stream, d, part, nblk, buffers, stat, (double)rows, 1e-5f, 0.1f);
  LAUNCH_CHECK(); ++*launches;
  if (pooled) {
    const int Lo = pooled_len(s.L);
    hipLaunchKernelGGL(usleep_bn_apply_pool_kernel, dim3(ew_blocks((long)B * cout * Lo)), dim3(256), 0, ctx->stream, z, stat, gamma, beta, y, pooled,
                       (long)B * cout, cout, s.L, Lo);
  } else {
    hipLaunchKernelGGL(usleep_bn_apply_kernel, dim3(ew_blocks(n)), dim3(256), 0, ctx->stream, z, stat, gamma, beta, y, n, cout, s.L);
  }
  LAUNCH_CHECK(); ++*launches;
  return 0;
}
// the same, taped in the model's arena
int layer_train(eegldm_usleep* u, const ConvSrc& s, const UConv& c, int bn_idx, int B, float** y_out, float** pooled_out, int* Lo_out) {
  const BnDesc& d = u->bns[bn_idx];
  const long n = (long)B * s.L * c.cout;
  ULayerTape t; t.src = s; t.c = c; t.bn = bn_idx; t.pool_Lo = 0;
  ALLOC_OR_FAIL(t.z, u->arena.alloc(sizeof(float) * (size_t)n));
  ALLOC_OR_FAIL(t.y, u->arena.alloc(sizeof(float) * (size_t)n));
  ALLOC_OR_FAIL(t.stat, u->arena.alloc(sizeof(float) * 2 * (size_t)c.cout));
  float* p = nullptr;
  if (pooled_out) {
    const int Lo = pooled_len(s.L);
    ALLOC_OR_FAIL(p, u->arena.alloc(sizeof(float) * (size_t)B * c.cout * Lo));
    *pooled_out = p; *Lo_out = Lo; t.pool_Lo = Lo;
  }
  EEG_TRY(conv_elu_bn_train(u->ctx, s, u->params + c.w, u->params + c.b, c.cout, c.k, d, u->params + d.w, u->params + d.b, u->buffers, t.z, t.stat, t.y, p, B,
                            &u->launches));
  *y_out = t.y;
  u->tape.push_back(t);
  return 0;
}
// backward of one taped layer: dy (B, cout, L) is overwritten by dz; dA / dB2 (nullable) receive the data gradient of the two parts
int layer_backward(eegldm_usleep* u, const ULayerTape& t, float* dy, float* dA, float* dB2, int B) {
  eegldm_ctx* ctx = u->ctx;
  const BnDesc& d = u->bns[t.bn];
  const ConvSrc& s = t.src;
  const long rows = (long)B * s.L;
  const int Cin = s.Ca + s.Cb, ns = auto_split(rows, t.c.cout, Cin);
  size_t need = bn_bwd_scratch_bytes(rows, t.c.cout);
  const size_t wneed = wgrad_scratch_bytes(ns, t.c.cout, Cin, t.c.k);
  if (wneed > need) need = wneed;
  float* scratch; EEG_TRY(eeg_det_buffer(ctx, need, &scratch));
  EEG_TRY(elu_bn_bwd(ctx, dy, t.z, t.stat, t.stat + t.c.cout, u->params + d.w, dy, u->grads + d.w, u->grads + d.b, B, t.c.cout, s.L, (char*)scratch, &u->launches));
  EEG_TRY(conv_wgrad(ctx, s, dy, B, t.c.cout, t.c.k, ns, scratch, u->grads + t.c.w, u->grads + t.c.b, &u->launches));
  if (dA) EEG_TRY(conv_dgrad_part(ctx, dy, u->params + t.c.w, dA, B, s.La, s.Ca, 0, Cin, t.c.cout, s.L, s.ups, t.c.k, &u->launches));
  if (dB2 && s.Cb) EEG_TRY(conv_dgrad_part(ctx, dy, u->params + t.c.w, dB2, B, s.Lb, s.Cb, s.Ca, Cin, t.c.cout, s.L, 0, t.c.k, &u->launches));
  return 0;
}
ClfW clf_weights(const eegldm_usleep* u) {
  const float* P = u->params;
  return {P + u->clf0.w, P + u->clf0.b, P + u->clf3.w, P + u->clf3.b, P + u->clf5.w, P + u->clf5.b};
}
ClfG clf_grads(const eegldm_usleep* u) {
  float* G = u->grads;
  return {G + u->clf0.w, G + u->clf0.b, G + u->clf3.w, G + u->clf3.b, G + u->clf5.w, G + u->clf5.b};
}
int bottleneck_len(const eegldm_usleep* u, int T) { int L = T; for (int i = 0; i < u->cfg.depth; i++) L = (L + ((L & 1) ? 2 : 0)) / 2; return L; }

int forward_train(eegldm_usleep* u, const float* x, float* y_pred, int B, int T) {
  EEG_CHECK(u && x && u->params && u->buffers, "null argument / unbound parameters");
  EEG_CHECK(u->grads, "gradients are not bound (eegldm_usleep_bind_grads)");
  EEG_CHECK(B >= 1 && T >= 1, "bad sizes");
  EEG_CHECK(T >= u->cfg.input_size, "T=%d is shorter than the classifier's pooling window %d", T, u->cfg.input_size);
  EEG_CHECK((long)B * bottleneck_len(u, T) >= 2, "train-mode BatchNorm needs more than one value per channel: B=%d x bottleneck length %d", B, bottleneck_len(u, T));
  const int d = u->cfg.depth;
  const std::vector<int>& ch = u->ch;
  u->arena.reset(); u->tape.clear(); u->tape_valid = false; u->launches = 0;
  std::vector<const float*> res(d); std::vector<int> resL(d);
  const float* cur = x; int Lc = T, Cc = ch[0];
  for (int i = 0; i < d; i++) {
    const ConvSrc s = {cur, Cc, Lc, 0, nullptr, 0, 0, Lc};
    float *y, *p; int Lo;
    EEG_TRY(layer_train(u, s, u->enc_c[i], i, B, &y, &p, &Lo));
    res[i] = y; resL[i] = Lc; cur = p; Lc = Lo; Cc = ch[i + 1];
  }
  { const ConvSrc s = {cur, Cc, Lc, 0, nullptr, 0, 0, Lc}; float* y; EEG_TRY(layer_train(u, s, u->bot_c, d, B, &y, nullptr, nullptr)); cur = y; Cc = ch[d + 1]; }
  for (int i = 0; i < d; i++) {
    const int co = ch[d - i], Lr = resL[d - 1 - i];
    float* pre;
    { const ConvSrc s = {cur, Cc, Lc, 1, nullptr, 0, 0, 2 * Lc}; EEG_TRY(layer_train(u, s, u->pre_c[i], d + 1 + 2 * i, B, &pre, nullptr, nullptr)); }
    int n = 2 * Lc;
    ConvSrc s2 = {pre, co, 2 * Lc, 0, nullptr, 0, 0, n};
    if (u->cfg.with_skip_connection) { n = n < Lr ? n : Lr; s2.b2 = res[d - 1 - i]; s2.Cb = co; s2.Lb = Lr; s2.L = n; }
    float* post; EEG_TRY(layer_train(u, s2, u->post_c[i], d + 2 + 2 * i, B, &post, nullptr, nullptr));
    cur = post; Lc = n; Cc = co;
  }
  const int S = Lc / u->cfg.input_size;
  EEG_CHECK(S >= 1, "decoder output length %d is shorter than the pooling window %d", Lc, u->cfg.input_size);
  ALLOC_OR_FAIL(u->t_mh, u->arena.alloc(sizeof(float) * 32 * (size_t)B * S));
  if (!y_pred) ALLOC_OR_FAIL(y_pred, u->arena.alloc(sizeof(float) * (size_t)B * u->cfg.n_classes * S));
  u->t_y = y_pred;
  EEG_TRY(clf_forward(u->ctx, cur, clf_weights(u), y_pred, u->t_mh, B, ch[1], Lc, u->cfg.input_size, S, u->cfg.n_classes, &u->launches));
  u->tB = B; u->tT = T; u->tL = Lc; u->tS = S; u->tape_valid = true;
  return 0;
}

int backward(eegldm_usleep* u, const float* dy_pred, float* dx) {
  EEG_CHECK(u && dy_pred, "null argument");
  EEG_CHECK(u->grads, "gradients are not bound (eegldm_usleep_bind_grads)");
  EEG_CHECK(u->tape_valid, "no tape: eegldm_usleep_forward_train has not run, or another forward on this object has reused its arena since");
  eegldm_ctx* ctx = u->ctx;
  const int d = u->cfg.depth, B = u->tB, C1 = u->ch[1];
  const std::vector<ULayerTape>& tp = u->tape;               // encoder 0..d-1, bottom, (preskip, postskip) x d
  const Arena::Mark mark = u->arena.mark();
  auto falloc = [&](long n) { return (float*)u->arena.alloc(sizeof(float) * (size_t)(n > 0 ? n : 1)); };
  std::vector<float*> dskip(d, nullptr);
  // classifier head
  const ULayerTape& last = tp.back();
  float* g; ALLOC_OR_FAIL(g, falloc((long)B * C1 * u->tL));
  {
    const int ns = auto_split((long)B * u->tL, C1, C1);
    float* scratch; EEG_TRY(eeg_det_buffer(ctx, clf_bwd_scratch_bytes(B, C1, u->tL, u->tS, ns), &scratch));
    EEG_TRY(clf_backward(ctx, last.y, clf_weights(u), clf_grads(u), dy_pred, u->t_mh, g, B, C1, u->tL, u->cfg.input_size, u->tS, u->cfg.n_classes, ns,
                         (char*)scratch, &u->launches));
  }
  // decoder, last block first
  for (int i = d - 1; i >= 0; i--) {
    const ULayerTape& post = tp[d + 1 + 2 * i + 1];
    const ULayerTape& pre = tp[d + 1 + 2 * i];
    float* dpre; ALLOC_OR_FAIL(dpre, falloc((long)B * post.src.Ca * post.src.La));
    float* dsk = nullptr;
    if (post.src.Cb) ALLOC_OR_FAIL(dsk, falloc((long)B * post.src.Cb * post.src.Lb));
    dskip[d - 1 - i] = dsk;
    EEG_TRY(layer_backward(u, post, g, dpre, dsk, B));
    float* dcur; ALLOC_OR_FAIL(dcur, falloc((long)B * pre.src.Ca * pre.src.La));
    EEG_TRY(layer_backward(u, pre, dpre, dcur, nullptr, B));
    g = dcur;
  }
  // bottom
  {
    const ULayerTape& t = tp[d];
    float* dp; ALLOC_OR_FAIL(dp, falloc((long)B * t.src.Ca * t.src.La));
    EEG_TRY(layer_backward(u, t, g, dp, nullptr, B));
    g = dp;
  }
  // encoder: the block output's gradient = MaxPool backward + the skip connection's gradient, written once
  for (int i = d - 1; i >= 0; i--) {
    const ULayerTape& t = tp[i];
    float* dyb; ALLOC_OR_FAIL(dyb, falloc((long)B * t.c.cout * t.src.L));
    EEG_TRY(maxpool_bwd(ctx, t.y, g, dskip[i], dyb, (long)B * t.c.cout, t.src.L, &u->launches));
    float* din = nullptr;
    if (i > 0) ALLOC_OR_FAIL(din, falloc((long)B * t.src.Ca * t.src.La));
    else din = dx;
    EEG_TRY(layer_backward(u, t, dyb, din, nullptr, B));
    g = din;
  }
  u->arena.release(mark);
  return 0;
}
}  // namespace

int usleep_layer_train_entry(eegldm_ctx* ctx, const float* a, int Ca, int La, int ups, const float* b2, int Cb, int Lb, int L, const float* w,
                             const float* bias, const float* gamma, const float* beta, float* buffers, int B, int Cout, int K, float* y, float* pooled,
                             float* z, float* stat) {
  const ConvSrc s = {a, Ca, La, ups, b2, Cb, Lb, L};
  EEG_TRY(src_check(s, K));
  BnDesc d; d.C = Cout; d.w = 0; d.b = 0; d.rm = 0; d.rv = Cout; d.nbt = 2 * (long)Cout; d.fold = 0;
  float* tmp = nullptr;                                     // the tape's z and stat when the caller does not ask for them
  const size_t nz = (size_t)B * Cout * L;
  if (!z || !stat) HIP_TRY(hipMalloc(&tmp, sizeof(float) * (nz + 2 * (size_t)Cout)));
  long launches = 0;
  const int rc = conv_elu_bn_train(ctx, s, w, bias, Cout, K, d, gamma, beta, buffers, z ? z : tmp, stat ? stat : tmp + nz, y, pooled, B, &launches);
  if (tmp) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(tmp); }
  return rc;
}

extern "C" int eegldm_usleep_bind_grads(eegldm_usleep* u, float* grads) {
  EEG_CHECK(u && grads, "null argument");
  u->grads = grads;
  return 0;
}
extern "C" int eegldm_usleep_forward_train(eegldm_usleep* u, const float* x, float* y_pred, int B, int T) {
  EEG_CHECK(y_pred, "null argument");
  return forward_train(u, x, y_pred, B, T);
}
extern "C" int eegldm_usleep_backward(eegldm_usleep* u, const float* dy_pred, float* dx) {
  if (u) u->launches = 0;
  return backward(u, dy_pred, dx);
}
extern "C" long eegldm_usleep_last_launches(const eegldm_usleep* u) { return u ? u->launches : 0; }

extern "C" int eegldm_usleep_stage_loss(eegldm_ctx* ctx, const float* logits, const int64_t* labels, const float* class_weight, int B, int n_classes, int S,
                                        float grad_scale, float* loss_out, float* dlogits, int* label_flag) {
  EEG_CHECK(ctx && logits && labels && loss_out, "null argument");
  EEG_CHECK(B >= 1 && S >= 1 && n_classes >= 1 && n_classes <= 16, "bad sizes");
  long l = 0;
  return ce_loss(ctx, logits, labels, class_weight, loss_out, dlogits, label_flag, B, n_classes, S, grad_scale, &l);
}
extern "C" int eegldm_usleep_label_error(eegldm_usleep* u, int* out) {
  EEG_CHECK(u && out, "null argument");
  *out = 0;
  if (!u->label_flag) return 0;
  HIP_TRY(hipStreamSynchronize(u->ctx->stream));
  HIP_TRY(hipMemcpy(out, u->label_flag, sizeof(int), hipMemcpyDeviceToHost));
  if (*out) HIP_TRY(hipMemset(u->label_flag, 0, sizeof(int)));
  return 0;
}
extern "C" int eegldm_usleep_train_step(eegldm_usleep* u, const float* x, const int64_t* labels, const float* class_weight, int B, int T, float grad_scale,
                                        float* loss_out, float* y_pred) {
  EEG_CHECK(u && x && labels && loss_out, "null argument");
  EEG_CHECK(u->grads, "gradients are not bound (eegldm_usleep_bind_grads)");
  EEG_CHECK(B >= 1 && T >= u->cfg.input_size, "T=%d is shorter than the classifier's pooling window %d (or B=%d < 1)", T, u->cfg.input_size, B);
  if (!u->label_flag) { HIP_TRY(hipMalloc(&u->label_flag, sizeof(int))); HIP_TRY(hipMemset(u->label_flag, 0, sizeof(int))); }
  EEG_TRY(forward_train(u, x, y_pred, B, T));
  float* dy; ALLOC_OR_FAIL(dy, u->arena.alloc(sizeof(float) * (size_t)B * u->cfg.n_classes * u->tS));
  EEG_TRY(ce_loss(u->ctx, u->t_y, labels, class_weight, loss_out, dy, u->label_flag, B, u->cfg.n_classes, u->tS, grad_scale, &u->launches));
  return backward(u, dy, nullptr);
}

// ---------------------------------------------------------------- primitive exports (tests)
extern "C" int eegldm_usleep_conv_bwd(eegldm_ctx* ctx, const float* a, int Ca, int La, int ups, const float* b2, int Cb, int Lb, int L, const float* w,
                                      const float* dz, int B, int Cout, int K, int nsplit, float* dA, float* dB2, float* dw, float* db) {
  EEG_CHECK(ctx && w && dz && B >= 1 && Cout >= 1, "bad argument");
  const ConvSrc s = {a, Ca, La, ups ? 1 : 0, b2, Cb, Lb, L};
  EEG_TRY(src_check(s, K));
  EEG_CHECK(nsplit >= 0 && nsplit <= 65535, "nsplit");
  EEG_CHECK((dw != nullptr) == (db != nullptr), "dw and db come together");
  const long rows = (long)B * L;
  const int Cin = Ca + Cb;
  long launches = 0;
  if (dw) {
    int ns = nsplit ? nsplit : auto_split(rows, Cout, Cin);
    if (ns > rows) ns = (int)rows;
    float* scratch; EEG_TRY(eeg_det_buffer(ctx, wgrad_scratch_bytes(ns, Cout, Cin, K), &scratch));
    EEG_TRY(conv_wgrad(ctx, s, dz, B, Cout, K, ns, scratch, dw, db, &launches));
  }
  if (dA) EEG_TRY(conv_dgrad_part(ctx, dz, w, dA, B, La, Ca, 0, Cin, Cout, L, s.ups, K, &launches));
  if (dB2 && Cb) EEG_TRY(conv_dgrad_part(ctx, dz, w, dB2, B, Lb, Cb, Ca, Cin, Cout, L, 0, K, &launches));
  return 0;
}
extern "C" int eegldm_usleep_elu_bn_bwd(eegldm_ctx* ctx, const float* dy, const float* z, const float* mean, const float* rstd, const float* gamma, float* dz,
                                        float* dgamma, float* dbeta, int B, int C, int L) {
  EEG_CHECK(ctx && dy && z && mean && rstd && gamma && dz && dgamma && dbeta, "null argument");
  EEG_CHECK(B >= 1 && C >= 1 && C <= 65535 && L >= 1 && (long)B * L >= 2, "bad sizes (batch statistics need B * L >= 2)");
  float* scratch; EEG_TRY(eeg_det_buffer(ctx, bn_bwd_scratch_bytes((long)B * L, C), &scratch));
  long launches = 0;
  return elu_bn_bwd(ctx, dy, z, mean, rstd, gamma, dz, dgamma, dbeta, B, C, L, (char*)scratch, &launches);
}
extern "C" int eegldm_usleep_maxpool_bwd(eegldm_ctx* ctx, const float* x, const float* dpool, const float* dskip, float* dx, long nrows, int L) {
  EEG_CHECK(ctx && x && dpool && dx && nrows >= 1 && L >= 1, "bad argument");
  long launches = 0;
  return maxpool_bwd(ctx, x, dpool, dskip, dx, nrows, L, &launches);
}
extern "C" int eegldm_usleep_clf_loss(eegldm_ctx* ctx, const float* x, const float* const* weights, float* const* grads, const int64_t* labels,
                                      const float* class_weight, int B, int C1, int L, int input_size, int n_classes, float grad_scale, float* loss_out,
                                      float* logits, float* dx, int* label_flag) {
  EEG_CHECK(ctx && x && weights && grads && labels && loss_out && logits && dx, "null argument");
  for (int i = 0; i < 6; i++) EEG_CHECK(weights[i] && grads[i], "null parameter / gradient pointer %d", i);
  EEG_CHECK(B >= 1 && C1 >= 1 && C1 <= 16 && n_classes >= 1 && n_classes <= 16 && input_size >= 1, "bad sizes");
  EEG_CHECK(L >= input_size, "L=%d is shorter than the pooling window %d", L, input_size);
  const int S = L / input_size;
  const int ns = auto_split((long)B * L, C1, C1);
  const size_t head = up256(sizeof(float) * 32 * (size_t)B * S) + up256(sizeof(float) * (size_t)B * n_classes * S);
  float* scratch; EEG_TRY(eeg_det_buffer(ctx, head + clf_bwd_scratch_bytes(B, C1, L, S, ns), &scratch));
  float* mh = scratch;
  float* dy = (float*)((char*)scratch + up256(sizeof(float) * 32 * (size_t)B * S));
  const ClfW P = {weights[0], weights[1], weights[2], weights[3], weights[4], weights[5]};
  const ClfG G = {grads[0], grads[1], grads[2], grads[3], grads[4], grads[5]};
  long launches = 0;
  EEG_TRY(clf_forward(ctx, x, P, logits, mh, B, C1, L, input_size, S, n_classes, &launches));
  EEG_TRY(ce_loss(ctx, logits, labels, class_weight, loss_out, dy, label_flag, B, n_classes, S, grad_scale, &launches));
  return clf_backward(ctx, x, P, G, dy, mh, dx, B, C1, L, input_size, S, n_classes, ns, (char*)scratch + head, &launches);
}
