// proj_out folded into the V projection of a single-head AttentionBlock (16-bit storage).
//   out = x + (P V) Wp^T + bp = x + P (xn Wvp^T + bv')      with Wvp = Wp Wv, bv' = Wp bv + bp      (every row of P sums to 1)
// This file holds the small fp32 products around that identity, batched over the blocks of a network:
//   refresh (NetBase::sync_weights):         E = [Wq ; Wk ; round(Wp Wv)] (16-bit), be = [bq | bk | Wp bv + bp] (fp32)
//   back-transform (NetBase::flush_attn_folds), from the scratch gradient g = d/dE, gb = d/dbe of one backward:
//     dWq, dWk += g rows;  dWv += Wp^T g_v;  dWp += g_v Wv^T + gb_v bv^T;  dbq, dbk += gb;  dbv += Wp^T gb_v;  dbp += gb_v
// The K projection folded into Q on top of that: the terms of Q_i . K_j that depend on the query row alone cancel in the row softmax,
//   softmax_j(Q_i . K_j) = softmax_j(Q'_i . xn_j)      with Q' = xn W'^T + c, W' = Wk^T Wq, c = Wk^T bq      (the key operand is xn itself)
//   refresh: E gains the rows round(W') behind Wvp (4C rows in all), be gains c; the route's weight is the 2C x C sub-matrix [Wvp ; W']
//   back-transform, G = d/dW', gc = d/dc:  dWq += Wk G;  dWk += Wq G^T + bq gc^T;  dbq += Wk gc;  dbk gets nothing (its true gradient is 0)
// All of it runs on the fp32 master parameters with plain FMA loops in a fixed order: one thread (or one block) owns an output element,
// nothing is added atomically, so the results are bit-reproducible run to run whatever EEGLDM_DETERMINISTIC says.
#include "common.h"
#include "internal.h"

namespace {

constexpr int FT = 64, FK = 32;      // output tile edge, K chunk

// C[m][n] (+)= sum_k A(m, k) B(k, n) (+ u[m] v[n]) for square n x n fp32 operands of leading dimension n, n % 64 == 0.
// 256 threads, a 4 x 4 register tile each; the next K chunk is fetched into registers while the current one is multiplied (a network has
// only a few hundred of these tiles: one or two blocks per CU, nothing else to hide the fetch behind).  Block (x, y): tile x of problem y.
template <typename T16>
__global__ __launch_bounds__(256) void fold_gemm_kernel(const FoldGemmBatch p) {
  __shared__ float As[FK][FT + 4], Bs[FK][FT + 4];
  const FoldGemm g = p.g[blockIdx.y];
  const int n = p.n, tiles = n / FT;
  const int m0 = (blockIdx.x / tiles) * FT, n0 = (blockIdx.x % tiles) * FT;
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = 0.f;
  // operand stored [row of the tile][k]: a thread fetches 4 consecutive k of one row, twice (k and k + 16); stored [k][row]: 4 consecutive
  // rows of one k, twice (k and k + 16)
  const int rk_r = t >> 2, rk_k = (t & 3) * 4;      // [row][k] layout
  const int kr_k = t >> 4, kr_r = (t & 15) * 4;     // [k][row] layout
  const float* pa = g.ta ? g.A + (long)kr_k * n + m0 + kr_r : g.A + (long)(m0 + rk_r) * n + rk_k;
  const float* pb = g.tb ? g.B + (long)(n0 + rk_r) * n + rk_k : g.B + (long)kr_k * n + n0 + kr_r;
  const long sa = g.ta ? (long)n : 1, sb = g.tb ? 1 : (long)n;      // element step of one k
  float4 ra[2], rb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      ra[h] = *(const float4*)(pa + (k0 + 16 * h) * sa);
      rb[h] = *(const float4*)(pb + (k0 + 16 * h) * sb);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      if (g.ta) *(float4*)&As[kr_k + 16 * h][kr_r] = ra[h];
      else { As[rk_k + 16 * h][rk_r] = ra[h].x; As[rk_k + 16 * h + 1][rk_r] = ra[h].y; As[rk_k + 16 * h + 2][rk_r] = ra[h].z; As[rk_k + 16 * h + 3][rk_r] = ra[h].w; }
      if (g.tb) { Bs[rk_k + 16 * h][rk_r] = rb[h].x; Bs[rk_k + 16 * h + 1][rk_r] = rb[h].y; Bs[rk_k + 16 * h + 2][rk_r] = rb[h].z; Bs[rk_k + 16 * h + 3][rk_r] = rb[h].w; }
      else *(float4*)&Bs[kr_k + 16 * h][kr_r] = rb[h];
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < n; k0 += FK) {
    stage();
    __syncthreads();
    if (k0 + FK < n) fetch(k0 + FK);
#pragma unroll
    for (int k = 0; k < FK; k++) {
      const float4 a = *(const float4*)&As[k][ty * 4], b = *(const float4*)&Bs[k][tx * 4];
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int m = m0 + ty * 4 + i, c = n0 + tx * 4;
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = g.u ? fmaf(g.u[m], g.v[c + j], acc[i][j]) : acc[i][j];
    if (g.out16) {
      uint2 o; o.x = pack16x2<T16>(r[0], r[1]); o.y = pack16x2<T16>(r[2], r[3]);
      *(uint2*)((T16*)g.out16 + (long)m * n + c) = o;
    } else {
      float4* d = (float4*)(g.acc + (long)m * n + c);
      float4 v = *d; v.x += r[0]; v.y += r[1]; v.z += r[2]; v.w += r[3]; *d = v;
    }
  }
}

// out[m] (+)= sum_k M[m][k] v[k] (+ add[m]), m < C: one wave per row, lanes across k (coalesced), butterfly sum (a fixed order)
template <bool ACC>
__device__ __forceinline__ void fold_matvec(const float* M, const float* v, const float* add, float* out, int C) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int m = blockIdx.x * 4 + wave; m < C; m += gridDim.x * 4) {
    float s = 0.f;
    for (int k = lane; k < C; k += 64) s = fmaf(M[(long)m * C + k], v[k], s);
    s = wave_sum(s);
    if (lane == 0) { if (add) s += add[m]; out[m] = ACC ? out[m] + s : s; }
  }
}
// out[k] (+)= sum_m M[m][k] v[m], k < C: a block takes 16 columns k, its 16 thread rows a 16th of the m range each (ascending), and thread
// k folds the 16 partial sums in slice order.  256 threads, C % 16 == 0.
template <bool ACC>
__device__ __forceinline__ void fold_tmatvec(const float* M, const float* v, float* out, int C, float (*part)[17]) {
  const int t = threadIdx.x, sl = t >> 4, c = t & 15, per = C / 16;
  for (int cb = blockIdx.x; cb < C / 16; cb += gridDim.x) {      // (block-uniform trip count: the barriers are safe)
    const int k = cb * 16 + c;
    float s = 0.f;
    for (int m = sl * per; m < (sl + 1) * per; m++) s = fmaf(M[(long)m * C + k], v[m], s);
    part[sl][c] = s;
    __syncthreads();
    if (t < 16) {
      float tot = 0.f;
#pragma unroll
      for (int j = 0; j < 16; j++) tot += part[j][t];
      out[cb * 16 + t] = ACC ? out[cb * 16 + t] + tot : tot;
    }
    __syncthreads();
  }
}

// refresh, everything but the products: Q / K rows of the 16-bit weight copied, the effective bias.  Block (x, y): slice x of block y.
// bv' = Wp bv + bp, c = Wk^T bq
__global__ __launch_bounds__(256) void fold_refresh_misc_kernel(const FoldMiscBatch p) {
  __shared__ float part[16][17];
  const FoldMisc f = p.f[blockIdx.y];
  const int C = p.n, t = threadIdx.x;
  const long nchunk = (long)2 * C * C / 8;        // 16-byte chunks of the Q and K rows
  for (long i = (long)blockIdx.x * blockDim.x + t; i < nchunk; i += (long)gridDim.x * blockDim.x)
    ((uint4*)f.e16)[i] = ((const uint4*)f.w16)[i];
  for (int i = blockIdx.x * blockDim.x + t; i < 2 * C; i += gridDim.x * blockDim.x) f.be[i] = f.bqkv[i];
  fold_matvec<false>(f.wp, f.bqkv + 2 * C, f.bp, f.be + 2 * C, C);
  fold_tmatvec<false>(f.wqkv + (long)C * C, f.bqkv, f.be + 3 * C, C, part);
}

// back-transform, everything but the products: dbv += Wp^T gb_v, dbp += gb_v; then the Q / K rows and biases pass through (qk == 0), or
// dbq += Wk gc and nothing for the K rows, whose gradient the products carry, and for bk (qk != 0; f.qk is uniform over the block)
__global__ __launch_bounds__(256) void fold_back_misc_kernel(const FoldMiscBatch p) {
  __shared__ float part[16][17];
  const FoldMisc f = p.f[blockIdx.y];
  const int C = p.n, t = threadIdx.x;
  if (!f.qk) {
    const long n4 = (long)2 * C * C / 4;
    for (long i = (long)blockIdx.x * blockDim.x + t; i < n4; i += (long)gridDim.x * blockDim.x) {
      const float4 s = ((const float4*)f.g)[i];
      float4 d = ((float4*)f.dwqkv)[i];
      d.x += s.x; d.y += s.y; d.z += s.z; d.w += s.w;
      ((float4*)f.dwqkv)[i] = d;
    }
    for (int i = blockIdx.x * blockDim.x + t; i < 2 * C; i += gridDim.x * blockDim.x) f.dbqkv[i] += f.gb[i];
  } else fold_matvec<true>(f.wqkv + (long)C * C, f.gb + 3 * C, nullptr, f.dbqkv, C);
  for (int i = blockIdx.x * blockDim.x + t; i < C; i += gridDim.x * blockDim.x) f.dbp[i] += f.gb[2 * C + i];
  fold_tmatvec<true>(f.wp, f.gb + 2 * C, f.dbqkv + 2 * C, C, part);
}

}  // namespace

int fold_gemm_launch(eegldm_ctx* ctx, const FoldGemm* probs, int nprob, int n, int dtype) {
  EEG_CHECK(n > 0 && n % FT == 0, "fold product: n = %d is not a multiple of %d", n, FT);
  for (int i = 0; i < nprob; i += FOLD_MAX_BATCH) {
    FoldGemmBatch b; b.n = n;
    const int cnt = nprob - i < FOLD_MAX_BATCH ? nprob - i : FOLD_MAX_BATCH;
    for (int j = 0; j < cnt; j++) b.g[j] = probs[i + j];
    const dim3 grid((unsigned)((n / FT) * (n / FT)), (unsigned)cnt);
    if (dtype == EEGLDM_F16) hipLaunchKernelGGL(fold_gemm_kernel<f16_t>, grid, dim3(256), 0, ctx->stream, b);
    else hipLaunchKernelGGL(fold_gemm_kernel<bf16_t>, grid, dim3(256), 0, ctx->stream, b);
    LAUNCH_CHECK();
  }
  return 0;
}
int fold_misc_launch(eegldm_ctx* ctx, const FoldMisc* blocks, int nblock, int C, int back) {
  EEG_CHECK(C > 0 && C % 8 == 0, "fold: C = %d is not a multiple of 8", C);
  for (int i = 0; i < nblock; i += FOLD_MAX_BATCH) {
    FoldMiscBatch b; b.n = C;
    const int cnt = nblock - i < FOLD_MAX_BATCH ? nblock - i : FOLD_MAX_BATCH;
    for (int j = 0; j < cnt; j++) b.f[j] = blocks[i + j];
    EEG_CHECK(C % 16 == 0, "fold: C = %d is not a multiple of 16", C);
    const dim3 grid(128, (unsigned)cnt);
    if (back) hipLaunchKernelGGL(fold_back_misc_kernel, grid, dim3(256), 0, ctx->stream, b);
    else hipLaunchKernelGGL(fold_refresh_misc_kernel, grid, dim3(256), 0, ctx->stream, b);
    LAUNCH_CHECK();
  }
  return 0;
}
