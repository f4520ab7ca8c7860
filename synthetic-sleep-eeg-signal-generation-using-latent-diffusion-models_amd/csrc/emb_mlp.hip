// Time-embedding MLP of the UNet on kernels written for its shapes.
//
//   forward   e0 = temb(t); h1 = e0 W0^T + b0; a1 = silu(h1); emb = a1 W2^T + b2 [+ label_emb[y]]; semb = silu(emb); emb_all = semb We^T + be
//   backward  from demb_all (n x E) and the tape (e0, h1, a1, emb, semb): the six parameter gradients (+= into the gradient buffer)
//
// n is a few hundred rows at most and every product is fp32 on the fp32 master weights, so the general 128 x 128-tile GEMM ran them on 8 to
// 104 workgroups.  Here ONE tile kernel serves every product: 64 x 64 output tiles, 4 waves of 2 x 2 v_mfma_f32_16x16x4_f32 fragments, the
// whole reduction of a tile in one workgroup in a fixed order (64-wide chunks, the next two in flight in registers while this one is
// multiplied).  The element-wise neighbours ride in its epilogue (bias, label rows, silu, silu'); temb stays its own small launch.  The one long
// reduction (dsemb = demb_all We, over E) is split into written fp32 partials that the silu' kernel folds in index order.  No atomics, no
// memset: forward and backward are bit-reproducible from run to run in every mode.
//
// Operand tiles in LDS are [outer 64][inner 64 (contiguous in memory) + 4]: "MK" operands (k contiguous: x of a Linear, dY of a data
// gradient) have outer = output index, "KM" operands (output index contiguous: W of a data gradient, both operands of a weight gradient)
// have outer = k.  Either way lane (c = lane & 15, h = lane >> 4) feeds k = 16 g + 4 h + j to step j of group g, so A and B agree on the k order.
#include "emb_mlp_plan.h"
#include "internal.h"

namespace {

enum { EPI_FWD = 0, EPI_PART = 1, EPI_DSILU = 2, EPI_WGRAD = 3 };

struct EmbGemm {
  const float* A; long lda; const float* B; long ldb;
  int M, N, K;                  // C is M x N, K the reduction length
  int avec, bvec;               // operand rows are 16-byte aligned (base and leading dimension): float4 loads
  int tiles_n;
  float* C; long ldc;
  float* C2;                    // EPI_FWD: silu(C), or null
  const float* bias;            // EPI_FWD: [N]
  const int64_t* labels; const float* table; int num_classes;      // EPI_FWD: C[m] += table[labels[m]] (rows of width N), or null
  const float* aux; long ldaux; // EPI_DSILU: C = acc * silu'(aux)
  float* colsum;                // EPI_WGRAD: colsum[m] += sum_k A[k][m] (the tiles of column block 0 do it), or null
  const float* zero;            // >= 16 zero bytes, 16-byte aligned (the context's zero page)
  int kper; long part_stride;   // EPI_PART: split z reduces [z * kper, (z + 1) * kper) into C + z * part_stride
};

// Four consecutive floats of an operand, or zeros.  Branch-free and select-free: a lane with nothing to load reads the context's page of
// zeros, so the eight loads of a chunk issue back to back and nothing touches their result before the LDS store of the next iteration (a
// per-lane branch around each load made every one wait for the one before; a select on the loaded value put the wait ahead of the MFMAs).
// The contiguous extents are multiples of 4 (emb_mlp_takes), so a group of four is inside or outside as a whole.
__device__ __forceinline__ float4 ld4(const float* __restrict__ base, long off, bool ok, bool vec, const float* __restrict__ zero) {
  const float* p = ok ? base + off : zero;
  if (vec) return *(const float4*)p;
  return make_float4(p[0], p[1], p[2], p[3]);
}
// An operand tile is T output indices x 64 k: T / 16 float4 per thread.  MK: thread (o = tid / 16 + 16 i, q = tid % 16) owns [row o][k 4 q ..];
// KM: a k row holds T / 4 float4, thread (o = tid / (T / 4) + (1024 / T) i, q = tid % (T / 4)) owns [k o][index 4 q ..].
template <bool KM, int T> struct TileMap {
  static constexpr int PITCH = KM ? T + 4 : EMB_KC + 4;      // floats; rows stay 16-byte aligned, fragment reads are conflict-free
  static constexpr int W4 = KM ? T / 4 : EMB_KC / 4, NV = T / 16, STEP = 256 / W4;
  static __device__ __forceinline__ int o(int tid, int i) { return tid / W4 + STEP * i; }
  static __device__ __forceinline__ int q(int tid) { return (tid % W4) * 4; }
};
template <bool KM, int T>
__device__ __forceinline__ void load_tile(float4 (&r)[T / 16], const float* __restrict__ X, long ld, bool vec, int x0, int xend, int k0, int kend, int tid,
                                          const float* __restrict__ zero) {
  using M = TileMap<KM, T>;
  const int q = M::q(tid);
#pragma unroll
  for (int i = 0; i < M::NV; i++) {
    const int o = M::o(tid, i);
    if constexpr (KM) { const int k = k0 + o, x = x0 + q; r[i] = ld4(X, (long)k * ld + x, k < kend && emb_valid4(x, xend) == 4, vec, zero); }
    else { const int x = x0 + o, k = k0 + q; r[i] = ld4(X, (long)x * ld + k, x < xend && emb_valid4(k, kend) == 4, vec, zero); }
  }
}
template <bool KM, int T> __device__ __forceinline__ void store_tile(float* __restrict__ s, const float4 (&r)[T / 16], int tid) {
  using M = TileMap<KM, T>;
#pragma unroll
  for (int i = 0; i < M::NV; i++) *(float4*)(s + M::o(tid, i) * M::PITCH + M::q(tid)) = r[i];
}
// the four k steps of group g for output index x (row of A / column of B)
template <bool KM, int T> __device__ __forceinline__ float4 frag(const float* __restrict__ s, int x, int g, int h) {
  constexpr int P = TileMap<KM, T>::PITCH;
  if constexpr (KM) {
    const float* p = s + (16 * g + 4 * h) * P + x;
    return make_float4(p[0], p[P], p[2 * P], p[3 * P]);
  } else return *(const float4*)(s + x * P + 16 * g + 4 * h);
}

// WGRAD launches carry two problems (blocks [0, tiles0) serve p0, the rest p1); every other launch passes p1 = p0, tiles0 = its tile count
// T x T output tiles (64, or 32 where 64 would leave most of the chip idle): 4 waves of FR x FR 16 x 16 fragments, FR = T / 32
template <bool A_KM, bool B_KM, int EPI, int T>
__global__ __launch_bounds__(256) void emb_gemm_kernel(const EmbGemm p0, const EmbGemm p1, int tiles0) {
  constexpr int FR = T / 32, NV = T / 16;
  __shared__ __attribute__((aligned(16))) float As[EMB_KC * (T + 4)];      // holds either layout: T rows of 68 or 64 rows of T + 4
  __shared__ __attribute__((aligned(16))) float Bs[EMB_KC * (T + 4)];
  // Blocks are dealt round-robin over the 8 XCDs (each with its own L2): block b of nb runs logical tile (b % 8) * (nb / 8) + b / 8, so that one
  // XCD works through a contiguous run of the tile order below and the tiles that share a large operand slab share an L2 (speed only;
  // nb % 8 != 0 keeps the plain order).  Tile order: split z outermost (EPI_PART: one slab of W and dY per split); then the operand that is
  // re-read across tiles is the small one -- forward / data gradient: tiles of one weight slab (same tn) are consecutive; weight gradient:
  // tiles of one dY slab (same tm) are consecutive.
  int bid = blockIdx.x;
  { const int nb = gridDim.x; if ((nb & 7) == 0) bid = (bid & 7) * (nb >> 3) + (bid >> 3); }
  const bool second = EPI == EPI_WGRAD && bid >= tiles0;
  const EmbGemm& p = second ? p1 : p0;
  if (second) bid -= tiles0;
  const int tiles_m = (p.M + T - 1) / T, per_split = tiles_m * p.tiles_n;
  const int z = bid / per_split;      // 0 unless EPI_PART
  bid -= z * per_split;
  int tm, tn;
  if constexpr (EPI == EPI_WGRAD) { tm = bid / p.tiles_n; tn = bid - tm * p.tiles_n; }
  else { tn = bid / tiles_m; tm = bid - tn * tiles_m; }
  const int m0 = tm * T, n0 = tn * T;
  int kbeg = 0, kend = p.K;
  if constexpr (EPI == EPI_PART) { kbeg = z * p.kper; kend = min(p.K, kbeg + p.kper); }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, h = lane >> 4, wm = w & 1, wn = w >> 1;

  f32x4 acc[FR][FR];
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int j = 0; j < FR; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 ra[2][NV], rb[2][NV];      // two chunks in flight: the loads of chunk c + 2 are issued when chunk c has been staged
  float cs = 0.f;
  const bool do_colsum = EPI == EPI_WGRAD && tn == 0 && p.colsum != nullptr;
  const bool avec = p.avec != 0, bvec = p.bvec != 0;

  // one chunk: stage buffer `buf` in LDS, refill it from two chunks ahead, multiply
  auto stage = [&](float4 (&qa)[NV], float4 (&qb)[NV], int k0) {
    __syncthreads();      // the previous chunk's fragment reads are done
    store_tile<A_KM, T>(As, qa, tid);
    store_tile<B_KM, T>(Bs, qb, tid);
    __syncthreads();
    if (k0 + 2 * EMB_KC < kend) {
      load_tile<A_KM, T>(qa, p.A, p.lda, avec, m0, p.M, k0 + 2 * EMB_KC, kend, tid, p.zero);
      load_tile<B_KM, T>(qb, p.B, p.ldb, bvec, n0, p.N, k0 + 2 * EMB_KC, kend, tid, p.zero);
    }
    if constexpr (EPI == EPI_WGRAD) {
      if (do_colsum && tid < T) {      // rows past kend and columns past M were staged as zeros
#pragma unroll 8
        for (int k = 0; k < EMB_KC; k++) cs += As[k * (T + 4) + tid];
      }
    }
#pragma unroll
    for (int g = 0; g < EMB_KC / 16; g++) {
      float4 a[FR], b[FR];
#pragma unroll
      for (int i = 0; i < FR; i++) a[i] = frag<A_KM, T>(As, wm * (T / 2) + i * 16 + c, g, h);
#pragma unroll
      for (int j = 0; j < FR; j++) b[j] = frag<B_KM, T>(Bs, wn * (T / 2) + j * 16 + c, g, h);
#pragma unroll
      for (int i = 0; i < FR; i++)
#pragma unroll
        for (int j = 0; j < FR; j++) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
        }
    }
  };

  load_tile<A_KM, T>(ra[0], p.A, p.lda, avec, m0, p.M, kbeg, kend, tid, p.zero);
  load_tile<B_KM, T>(rb[0], p.B, p.ldb, bvec, n0, p.N, kbeg, kend, tid, p.zero);
  if (kbeg + EMB_KC < kend) {
    load_tile<A_KM, T>(ra[1], p.A, p.lda, avec, m0, p.M, kbeg + EMB_KC, kend, tid, p.zero);
    load_tile<B_KM, T>(rb[1], p.B, p.ldb, bvec, n0, p.N, kbeg + EMB_KC, kend, tid, p.zero);
  }
  for (int k0 = kbeg; k0 < kend; k0 += 2 * EMB_KC) {
    stage(ra[0], rb[0], k0);
    if (k0 + EMB_KC < kend) stage(ra[1], rb[1], k0 + EMB_KC);
  }

  // acc[i][j][r] = C[m0 + wm * (T / 2) + i * 16 + 4 h + r][n0 + wn * (T / 2) + j * 16 + c].  What the epilogue reads (silu' argument, the gradient it adds to,
  // label rows) is loaded for all its elements first, from addresses clamped into the tensor, so that the loads are in flight together;
  // only the stores are guarded.
  int nn[FR]; bool nok[FR]; float bias[FR];
#pragma unroll
  for (int j = 0; j < FR; j++) {
    const int n = n0 + wn * (T / 2) + j * 16 + c;
    nok[j] = n < p.N; nn[j] = nok[j] ? n : p.N - 1; bias[j] = 0.f;
    if constexpr (EPI == EPI_FWD) bias[j] = p.bias[nn[j]];
  }
  long at[FR][4][FR]; bool ok[FR][4][FR]; float ex[FR][4][FR]; bool lok[FR][4];
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int m = m0 + wm * (T / 2) + i * 16 + 4 * h + r;
      const bool mok = m < p.M; const int mm = mok ? m : p.M - 1;
      long lab = -1; lok[i][r] = false;
      if constexpr (EPI == EPI_FWD) {
        if (p.labels) { lab = (long)p.labels[mm]; lok[i][r] = lab >= 0 && lab < p.num_classes; if (!lok[i][r]) lab = 0; }
      }
#pragma unroll
      for (int j = 0; j < FR; j++) {
        ok[i][r][j] = mok && nok[j]; at[i][r][j] = (long)mm * p.ldc + nn[j]; ex[i][r][j] = 0.f;
        if constexpr (EPI == EPI_FWD) { if (p.labels) ex[i][r][j] = p.table[lab * p.N + nn[j]]; }
        else if constexpr (EPI == EPI_DSILU) ex[i][r][j] = p.aux[(long)mm * p.ldaux + nn[j]];
        else if constexpr (EPI == EPI_WGRAD) ex[i][r][j] = p.C[at[i][r][j]];
      }
    }
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int j = 0; j < FR; j++) {
        if (!ok[i][r][j]) continue;
        const float v = acc[i][j][r];
        const long o_at = at[i][r][j];
        if constexpr (EPI == EPI_FWD) {
          float o = v + bias[j];
          if (lok[i][r]) o += ex[i][r][j];
          p.C[o_at] = o;
          if (p.C2) p.C2[o_at] = silu_f(o);
        } else if constexpr (EPI == EPI_PART) p.C[(long)z * p.part_stride + o_at] = v;
        else if constexpr (EPI == EPI_DSILU) p.C[o_at] = v * silu_grad_f(ex[i][r][j]);
        else p.C[o_at] = ex[i][r][j] + v;
      }
  if constexpr (EPI == EPI_WGRAD) {
    if (do_colsum && tid < T && m0 + tid < p.M) p.colsum[m0 + tid] += cs;
  }
}

// dsemb = sum of the split-K partials in index order; demb = dsemb * silu'(emb)
__global__ __launch_bounds__(256) void emb_fold_silu_kernel(const float* __restrict__ part, int nparts, long stride, const float* __restrict__ x,
                                                            float* __restrict__ dsemb, float* __restrict__ demb, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
#pragma unroll 4
  for (int z = 1; z < nparts; z++) s += part[(long)z * stride + i];
  if (dsemb) dsemb[i] = s;
  demb[i] = s * silu_grad_f(x[i]);
}

std::atomic<long> g_launches{0};      // kernels of this file launched so far (eegldm_debug_emb_mlp_launches)

inline int vec_ok(const float* p, long ld) { return ((uintptr_t)p & 15) == 0 && (ld & 3) == 0; }
// EEGLDM_EMB_MLP_TILE=32 / 64 forces the tile edge of every product but the split-K one (tests run both on the same shapes)
int pick_tile(long tiles64) {
  EEG_ENV_VAR(int, forced, getenv("EEGLDM_EMB_MLP_TILE") ? atoi(getenv("EEGLDM_EMB_MLP_TILE")) : 0);
  return forced == 32 || forced == 64 ? forced : emb_pick_tile(tiles64);
}
EmbGemm problem(const float* A, long lda, const float* B, long ldb, int M, int N, int K, float* C, long ldc) {
  EmbGemm g = {};
  g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K; g.C = C; g.ldc = ldc;
  g.avec = vec_ok(A, lda); g.bvec = vec_ok(B, ldb); g.kper = K;
  return g;
}
inline int tiles_of(const EmbGemm& g, int T) { return emb_tiles(g.M, T) * emb_tiles(g.N, T); }

template <bool A_KM, bool B_KM, int EPI>
int launch(eegldm_ctx* ctx, const EmbGemm& p0, const EmbGemm* p1, int splits) {
  const int T = EPI == EPI_PART ? EMB_TILE : pick_tile((long)tiles_of(p0, EMB_TILE) + (p1 ? tiles_of(*p1, EMB_TILE) : 0));
  const int t0 = tiles_of(p0, T), total = t0 + (p1 ? tiles_of(*p1, T) : 0);
  EmbGemm a = p0, b = p1 ? *p1 : p0;
  a.tiles_n = emb_tiles(a.N, T); b.tiles_n = emb_tiles(b.N, T);
  a.zero = b.zero = (const float*)ctx->zero_page;
  if (T == 32) hipLaunchKernelGGL((emb_gemm_kernel<A_KM, B_KM, EPI, 32>), dim3(total * splits), dim3(256), 0, ctx->stream, a, b, t0);
  else hipLaunchKernelGGL((emb_gemm_kernel<A_KM, B_KM, EPI, 64>), dim3(total * splits), dim3(256), 0, ctx->stream, a, b, t0);
  g_launches.fetch_add(1, std::memory_order_relaxed);
  LAUNCH_CHECK();
  return 0;
}

}  // namespace

bool emb_mlp_enabled() {
  EEG_ENV_VAR(bool, off, getenv("EEGLDM_NO_EMB_MLP") != nullptr);
  return !off;
}
// every extent is guarded element by element; the float4 paths additionally want whole 4-element groups along the contiguous dimensions
bool emb_mlp_takes(const EmbMlpNet& net, int n) {
  return n > 0 && net.mc > 0 && net.te > 0 && net.E > 0 && (net.mc & 3) == 0 && (net.te & 3) == 0 && (net.E & 3) == 0;
}

int emb_mlp_fwd(eegldm_ctx* ctx, const EmbMlpNet& net, const int64_t* tsteps, const int64_t* labels, int n, const EmbMlpTape& tp, float* emb_all) {
  const int mc = net.mc, te = net.te, E = net.E;
  EEG_CHECK(emb_mlp_takes(net, n), "shape not served (n %d, mc %d, te %d, E %d)", n, mc, te, E);
  EEG_TRY(ew_temb(ctx, tsteps, tp.e0, n, mc, EEGLDM_F32));
  {      // h1 = e0 W0^T + b0; a1 = silu(h1)
    EmbGemm g = problem(tp.e0, mc, net.w0, mc, n, te, mc, tp.h1e, te);
    g.bias = net.b0; g.C2 = tp.a1e;
    EEG_TRY((launch<false, false, EPI_FWD>(ctx, g, nullptr, 1)));
  }
  {      // emb = a1 W2^T + b2 [+ label_emb[y]]; semb = silu(emb)
    EmbGemm g = problem(tp.a1e, te, net.w2, te, n, te, te, tp.emb, te);
    g.bias = net.b2; g.C2 = tp.semb;
    if (net.num_classes > 0) { g.labels = labels; g.table = net.label; g.num_classes = net.num_classes; }
    EEG_TRY((launch<false, false, EPI_FWD>(ctx, g, nullptr, 1)));
  }
  {      // every ResBlock's projection in one product
    EmbGemm g = problem(tp.semb, te, net.we, te, n, E, te, emb_all, E);
    g.bias = net.be;
    EEG_TRY((launch<false, false, EPI_FWD>(ctx, g, nullptr, 1)));
  }
  return 0;
}

// work: split-K partials (splits * n * te) | demb (n * te) | dh1 (n * te)
long emb_mlp_bwd_work_floats(const EmbMlpNet& net, int n) {
  int splits, kper;
  emb_splitk_plan(emb_tiles(n) * emb_tiles(net.te), net.E, &splits, &kper);
  return ((long)splits + 2) * n * net.te;
}
int emb_mlp_bwd(eegldm_ctx* ctx, const EmbMlpNet& net, const EmbMlpGrads& gr, const int64_t* labels, int n, const EmbMlpTape& tp,
                const float* demb_all, float* work, float* dsemb_out) {
  const int mc = net.mc, te = net.te, E = net.E;
  EEG_CHECK(emb_mlp_takes(net, n), "shape not served (n %d, mc %d, te %d, E %d)", n, mc, te, E);
  int splits, kper;
  emb_splitk_plan(emb_tiles(n) * emb_tiles(te), E, &splits, &kper);
  const long nte = (long)n * te;
  float* part = work; float* demb = work + (long)splits * nte; float* dh1 = demb + nte;
  {      // G(emb_w) += demb_all^T semb, G(emb_b) += colsum(demb_all)
    EmbGemm g = problem(demb_all, E, tp.semb, te, E, te, n, gr.we, te);
    g.colsum = gr.be;
    EEG_TRY((launch<true, true, EPI_WGRAD>(ctx, g, nullptr, 1)));
  }
  {      // partials of dsemb = demb_all We
    EmbGemm g = problem(demb_all, E, net.we, te, n, te, E, part, te);
    g.kper = kper; g.part_stride = nte;
    EEG_TRY((launch<false, true, EPI_PART>(ctx, g, nullptr, splits)));
  }
  hipLaunchKernelGGL(emb_fold_silu_kernel, dim3((unsigned)((nte + 255) / 256)), dim3(256), 0, ctx->stream, part, splits, nte, tp.emb, dsemb_out, demb, nte);
  g_launches.fetch_add(1, std::memory_order_relaxed);
  LAUNCH_CHECK();
  if (net.num_classes > 0) EEG_TRY(ew_label_emb_grad(ctx, demb, te, labels, n, te, net.num_classes, gr.label));
  {      // dh1 = (demb W2) * silu'(h1)
    EmbGemm g = problem(demb, te, net.w2, te, n, te, te, dh1, te);
    g.aux = tp.h1e; g.ldaux = te;
    EEG_TRY((launch<false, true, EPI_DSILU>(ctx, g, nullptr, 1)));
  }
  {      // G(te2_w) += demb^T a1, G(te2_b) += colsum(demb); G(te0_w) += dh1^T e0, G(te0_b) += colsum(dh1): one launch
    EmbGemm g2 = problem(demb, te, tp.a1e, te, te, te, n, gr.w2, te);
    g2.colsum = gr.b2;
    EmbGemm g0 = problem(dh1, te, tp.e0, mc, te, mc, n, gr.w0, mc);
    g0.colsum = gr.b0;
    EEG_TRY((launch<true, true, EPI_WGRAD>(ctx, g2, &g0, 1)));
  }
  return 0;
}

extern "C" int eegldm_debug_emb_mlp_launches(long* out_host, int reset) {
  EEG_CHECK(out_host, "null argument");
  *out_host = reset ? g_launches.exchange(0) : g_launches.load();
  return 0;
}
// out12: tiles of the three forward products (3), of the weight gradients of emb_layers / time_embed.2 / time_embed.0 (3), of dsemb,
// its splits and kper, tiles of dh1, backward work floats (low 31 bits, high bits); tile edges as emb_pick_tile chooses them
extern "C" int eegldm_debug_emb_mlp_plan(int n, int mc, int te, int E, int* out12_host) {
  EEG_CHECK(out12_host && n > 0 && mc > 0 && te > 0 && E > 0, "bad argument");
  int splits, kper;
  emb_splitk_plan(emb_tiles(n) * emb_tiles(te), E, &splits, &kper);
  EmbMlpNet net = {}; net.mc = mc; net.te = te; net.E = E;
  const long wf = emb_mlp_bwd_work_floats(net, n);
  auto tiles = [](int M, int N, int T) { return emb_tiles(M, T) * emb_tiles(N, T); };
  auto picked = [&](int M, int N) { return tiles(M, N, emb_pick_tile(tiles(M, N, EMB_TILE))); };
  const int tp = emb_pick_tile((long)tiles(te, te, EMB_TILE) + tiles(te, mc, EMB_TILE));      // the two small weight gradients share a launch
  const int v[12] = {picked(n, te), picked(n, te), picked(n, E), picked(E, te), tiles(te, te, tp), tiles(te, mc, tp), tiles(n, te, EMB_TILE), splits, kper,
                     picked(n, te), (int)(wf & 0x7fffffff), (int)(wf >> 31)};
  for (int i = 0; i < 12; i++) out12_host[i] = v[i];
  return 0;
}
