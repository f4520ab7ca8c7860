// R = K(A, B) V: a kernel matrix between two row sets times a thin weight matrix, the primitive behind MMD^2, KID, the permutation
// two-sample test and the MMD witness function (eegldm.metrics).  fp32 in, float64 out; the Na x Nb kernel matrix never exists.
//   R[i][p] = sum_j k(a_i, b_j) V[j][p], pairs with j - i == diag_off left out
//   poly: k = (gamma <a, b> + coef0)^degree;  rbf: k = (1 / S) sum_s exp(-beta_s d2), d2 = max(0, asq[i] + bsq[j] - 2 <a, b>)
//   * kmm_tile_kernel: a workgroup owns 128 rows of A and one slab of B's 128-row tiles.  Per tile the Gram block runs on the f32-input
//     MFMA (32x32x2: an exact fmaf chain in ascending k starting from 0; operands staged as in knn_tile_kernel: global -> registers ->
//     LDS, k-major, zero-filled K tail and zero rows past the edges, the next K tile's loads in flight during the MFMAs), the epilogue
//     applies the kernel function in fp32 and writes the 128 x 128 block to LDS over the operand tiles; entries past Nb or on the left-out
//     diagonal are SELECTED to zero.  A second MFMA pass multiplies the block by the tile's 128 x P slice of V (LDS, zero-filled past Nb
//     and P) in four fmaf chains of 32 rows of B, each from zero in ascending j; every thread adds each chain's fp32 result into float64
//     registers (a chain of 32 keeps the fp32 share of the error at g(33), a quarter of a whole tile's).  At the slab's end they go to the
//     workspace [slab][rows][P], one writer per element.
//   * kmm_fold_kernel: sums the slabs from zero in index order in float64 and stores the sum, or adds it onto out (accumulate).
// No atomics, no memset.  The slab partition is a function of Nb alone, so a result repeats bit for bit, a row of R does not depend on
// the other rows of A, and a column does not depend on P.
#include "common.h"

namespace {
typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int TM = 128, TN = 128, KT = 16, NT = 256;
constexpr int LDT = 132;             // row stride of the k-major operand tiles
constexpr int SLD = 129;             // row stride of the kernel-value tile
constexpr int KBLOCK_FLOATS = TM * SLD;
constexpr int MAX_P = 64, VLD = 64;  // V tile: [TN][VLD]
constexpr int SUB = 32;              // rows of B per fp32 chain of the second product
constexpr int MAX_BETAS = 8, MAX_SLABS = 32;
constexpr size_t WS_CAP = (size_t)64 << 20;      // workspace per launch group; one row block needs at most 32 * 128 * 64 * 8 = 2 MiB
static_assert(2 * KT * LDT <= KBLOCK_FLOATS, "the operand tiles live inside the kernel-value tile's area");

struct KmmFn {
  int kind, degree, n_betas;
  float gamma, coef0;
  float betas[MAX_BETAS];
};

__global__ __launch_bounds__(NT) void kmm_tile_kernel(const float* __restrict__ a, long lda, const float* __restrict__ asq,
                                                      const float* __restrict__ b, long ldb, const float* __restrict__ bsq,
                                                      const float* __restrict__ v, long ldv, int row0, int Na, int Nb, int D, int P, KmmFn fn,
                                                      long diag_off, int tiles_per_slab, int rows_ws, double* __restrict__ ws) {
  extern __shared__ float sm[];
  float* sA = sm;                                   // [KT][LDT] rows of A, k-major
  float* sB = sm + KT * LDT;                        // [KT][LDT] rows of B, k-major
  float* S = sm;                                    // [TM][SLD] kernel values (after the K loop)
  float* sV = sm + KBLOCK_FLOATS;                   // [TN][VLD] the tile's slice of V

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int q0 = row0 + blockIdx.x * TM;
  const int slab = blockIdx.y;
  const int ctiles = (Nb + TN - 1) / TN;
  const int tile_lo = slab * tiles_per_slab;
  const int tile_hi = min(ctiles, tile_lo + tiles_per_slab);
  const int nkt = (D + KT - 1) / KT;
  const int np = (P + 31) >> 5;                     // 32-column groups of V in use

  // staging map: thread -> (k offset lk, rows lr + 16 j)
  const int lk = t & (KT - 1), lr = t >> 4;
  // V staging map: thread -> (column vp, rows vr + 4 j)
  const int vp = t & (VLD - 1), vr = t >> 6;

  double dacc[2][16];
#pragma unroll
  for (int n = 0; n < 2; n++)
#pragma unroll
    for (int r = 0; r < 16; r++) dacc[n][r] = 0.0;

  // rbf: |a_i|^2 of the rows this thread's accumulator elements belong to (the same for every tile)
  float as[2][16];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int gi = q0 + wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      as[m][r] = (fn.kind == 1 && gi < Na) ? asq[gi] : 0.f;
    }

  for (int tile = tile_lo; tile < tile_hi; tile++) {
    const int c0 = tile * TN;
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int n = 0; n < 2; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[m][n][r] = 0.f;

    float ra[8], rb[8];
    auto load_regs = [&](int k0) {
      const int kk = k0 + lk;
      const bool kin = kk < D;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int ai = q0 + lr + 16 * j, bi = c0 + lr + 16 * j;
        ra[j] = (kin && ai < Na) ? a[(long)ai * lda + kk] : 0.f;
        rb[j] = (kin && bi < Nb) ? b[(long)bi * ldb + kk] : 0.f;
      }
    };
    load_regs(0);
    for (int kt = 0; kt < nkt; kt++) {
      __syncthreads();                    // the previous K tile's reads (first K tile: the previous tile's second product) are done
#pragma unroll
      for (int j = 0; j < 8; j++) { sA[lk * LDT + lr + 16 * j] = ra[j]; sB[lk * LDT + lr + 16 * j] = rb[j]; }
      __syncthreads();
      if (kt + 1 < nkt) load_regs((kt + 1) * KT);
#pragma unroll
      for (int k2 = 0; k2 < KT / 2; k2++) {
        const int kk = 2 * k2 + (lane >> 5);
        float fa[2], fb[2];
#pragma unroll
        for (int m = 0; m < 2; m++) {
          fa[m] = sA[kk * LDT + wm * 64 + m * 32 + (lane & 31)];
          fb[m] = sB[kk * LDT + wn * 64 + m * 32 + (lane & 31)];
        }
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
          for (int n = 0; n < 2; n++) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[m], fb[n], acc[m][n], 0, 0, 0);
      }
    }
    // the tile's slice of V: issued before the epilogue's arithmetic, stored after it
    float rv[32];
#pragma unroll
    for (int j = 0; j < 32; j++) {
      const int bj = c0 + vr + 4 * j;
      rv[j] = (bj < Nb && vp < P) ? v[(long)bj * ldv + vp] : 0.f;
    }
    __syncthreads();                      // every wave has read its last operands: the area becomes the kernel-value tile
#pragma unroll
    for (int n = 0; n < 2; n++) {
      const int col = wn * 64 + n * 32 + (lane & 31);
      const int gj = c0 + col;
      const bool jin = gj < Nb;
      const float bs = (fn.kind == 1 && jin) ? bsq[gj] : 0.f;
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int row = wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const int gi = q0 + row;
          const float dot = acc[m][n][r];
          float kv;
          if (fn.kind == 0) {
            const float tt = fmaf(fn.gamma, dot, fn.coef0);
            kv = tt;
            for (int d = 1; d < fn.degree; d++) kv *= tt;
          } else {
            float d2 = fmaf(-2.0f, dot, as[m][r] + bs);
            d2 = d2 < 0.f ? 0.f : d2;                    // a NaN stays a NaN
            float e = expf(-fn.betas[0] * d2);
            for (int s = 1; s < fn.n_betas; s++) e += expf(-fn.betas[s] * d2);
            kv = e / (float)fn.n_betas;
          }
          const bool out = !jin || (long)gj - (long)gi == diag_off;
          S[row * SLD + col] = out ? 0.f : kv;           // selection: a NaN or inf on a left-out pair does not reach the sum
        }
    }
#pragma unroll
    for (int j = 0; j < 32; j++) sV[(vr + 4 * j) * VLD + vp] = rv[j];
    __syncthreads();
    // second product: wave w owns rows 32 w .. 32 w + 31 of the block and all of V's columns; the fp32 chain restarts every SUB rows of B
    const float* srow = S + (wave * 32 + (lane & 31)) * SLD;
#pragma unroll 1
    for (int sub = 0; sub < TN; sub += SUB) {
      f32x16 racc[2];
#pragma unroll
      for (int n = 0; n < 2; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) racc[n][r] = 0.f;
      if (np == 2) {
#pragma unroll
        for (int j2 = 0; j2 < SUB / 2; j2++) {
          const int jj = sub + 2 * j2 + (lane >> 5);
          const float ka = srow[jj];
          const float v0 = sV[jj * VLD + (lane & 31)], v1 = sV[jj * VLD + 32 + (lane & 31)];
          racc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka, v0, racc[0], 0, 0, 0);
          racc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka, v1, racc[1], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int j2 = 0; j2 < SUB / 2; j2++) {
          const int jj = sub + 2 * j2 + (lane >> 5);
          racc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(srow[jj], sV[jj * VLD + (lane & 31)], racc[0], 0, 0, 0);
        }
      }
#pragma unroll
      for (int n = 0; n < 2; n++)
#pragma unroll
        for (int r = 0; r < 16; r++) dacc[n][r] += (double)racc[n][r];
    }
  }
  const int g0 = blockIdx.x * TM;                   // row within the launch group
#pragma unroll
  for (int n = 0; n < 2; n++) {
    const int p = n * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (q0 + row < Na && g0 + row < rows_ws && p < P) ws[((size_t)slab * rows_ws + g0 + row) * P + p] = dacc[n][r];
    }
  }
}

// out[row0 + i][p] (+)= sum over the slabs, from zero, in index order
__global__ __launch_bounds__(NT) void kmm_fold_kernel(const double* __restrict__ ws, int nslab, int rows_ws, int P, int accumulate,
                                                      double* __restrict__ out, long ldo) {
  const long e = (long)blockIdx.x * NT + threadIdx.x;
  const long total = (long)rows_ws * P;
  if (e >= total) return;
  double s = 0.0;
  for (int sl = 0; sl < nslab; sl++) s += ws[(size_t)sl * total + e];
  double* o = out + (e / P) * ldo + (e % P);
  *o = accumulate ? *o + s : s;
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
}  // namespace

extern "C" int eegldm_kernel_matmul(eegldm_ctx* ctx, const float* a, long lda, const float* asq, const float* b, long ldb, const float* bsq,
                                    const float* v, long ldv, int Na, int Nb, int D, int P, int kind, int degree, float gamma, float coef0,
                                    const float* betas_host, int n_betas, long diag_off, int accumulate, double* out, long ldo) {
  EEG_CHECK(ctx && a && out && (Nb == 0 || (b && v)), "null argument");
  EEG_CHECK(Na >= 1 && Nb >= 0, "bad sizes Na %d Nb %d", Na, Nb);
  EEG_CHECK(D >= 1, "D %d < 1", D);
  EEG_CHECK(P >= 1 && P <= MAX_P, "P %d outside [1, %d]", P, MAX_P);
  EEG_CHECK(kind == 0 || kind == 1, "kind %d is neither 0 (poly) nor 1 (rbf)", kind);
  KmmFn fn{};
  fn.kind = kind; fn.degree = 1; fn.n_betas = 1; fn.gamma = gamma; fn.coef0 = coef0;
  if (kind == 0) {
    EEG_CHECK(degree >= 1 && degree <= 4, "degree %d outside [1, 4]", degree);
    fn.degree = degree;
  } else {
    EEG_CHECK(n_betas >= 1 && n_betas <= MAX_BETAS, "n_betas %d outside [1, %d]", n_betas, MAX_BETAS);
    EEG_CHECK(betas_host, "rbf needs betas");
    EEG_CHECK(asq && bsq, "rbf needs the rows' squared norms (asq, bsq)");
    fn.n_betas = n_betas;
    for (int s = 0; s < n_betas; s++) fn.betas[s] = betas_host[s];
  }
  EEG_CHECK(lda >= D && ldb >= D, "row strides %ld / %ld shorter than D %d", lda, ldb, D);
  EEG_CHECK(ldv >= P && ldo >= P, "row strides %ld / %ld shorter than P %d", ldv, ldo, P);
  EEG_CHECK(aligned4(a) && aligned4(asq) && aligned4(b) && aligned4(bsq) && aligned4(v), "float pointers must be 4-byte aligned");
  EEG_CHECK(((uintptr_t)out & 7u) == 0, "out must be 8-byte aligned");

  const int ctiles = (Nb + TN - 1) / TN;
  const int want = ctiles < MAX_SLABS ? ctiles : MAX_SLABS;                    // a function of Nb alone
  const int tps = want ? (ctiles + want - 1) / want : 1;
  const int nslab = want ? (ctiles + tps - 1) / tps : 0;
  if (nslab == 0) {
    if (!accumulate) {
      const long total = (long)Na * P;
      hipLaunchKernelGGL(kmm_fold_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ctx->stream, (const double*)nullptr, 0, Na, P, 0,
                         out, ldo);
      LAUNCH_CHECK();
    }
    return 0;
  }
  // row blocks per launch group: the whole of A when its partials fit the cap, else as many 128-row blocks as do
  const int rblocks = (Na + TM - 1) / TM;
  const size_t per_block = (size_t)nslab * TM * P * sizeof(double);
  long gblocks = (long)(WS_CAP / per_block);
  gblocks = gblocks < 1 ? 1 : gblocks; gblocks = gblocks > rblocks ? rblocks : gblocks;
  const size_t need = (size_t)nslab * (size_t)(gblocks * TM < Na ? gblocks * TM : Na) * P * sizeof(double);
  if (ctx->splitk_ws_bytes < need) {
    if (ctx->splitk_ws) { HIP_TRY(hipStreamSynchronize(ctx->stream)); if (ctx->side_on) HIP_TRY(hipStreamSynchronize(ctx->side)); HIP_TRY(hipFree(ctx->splitk_ws)); ctx->splitk_ws = nullptr; ctx->splitk_ws_bytes = 0; }
    HIP_TRY(hipMalloc(&ctx->splitk_ws, need)); ctx->splitk_ws_bytes = need;
  }
  double* ws = (double*)ctx->splitk_ws;
  const size_t lds = sizeof(float) * (KBLOCK_FLOATS + TN * VLD);
  static DevOnce once;
  if (once.need(ctx->device))
    HIP_TRY(hipFuncSetAttribute((const void*)kmm_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (long blk = 0; blk < rblocks; blk += gblocks) {
    const int row0 = (int)(blk * TM);
    const int nb = (int)(rblocks - blk < gblocks ? rblocks - blk : gblocks);
    const int rows = Na - row0 < nb * TM ? Na - row0 : nb * TM;
    hipLaunchKernelGGL(kmm_tile_kernel, dim3(nb, nslab), dim3(NT), lds, ctx->stream, a, lda, asq, b, ldb, bsq, v, ldv, row0, Na, Nb, D, P, fn,
                       diag_off, tps, rows, ws);
    LAUNCH_CHECK();
    const long total = (long)rows * P;
    hipLaunchKernelGGL(kmm_fold_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, ctx->stream, (const double*)ws, nslab, rows, P,
                       accumulate, out + (long)row0 * ldo, ldo);
    LAUNCH_CHECK();
  }
  return 0;
}
