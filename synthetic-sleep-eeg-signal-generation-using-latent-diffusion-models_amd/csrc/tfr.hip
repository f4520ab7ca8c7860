// Time-frequency primitives (eegldm.metrics: spectrograms, band courses, phase-amplitude coupling).
//   * stft_power_kernel: short-time multitaper power.  A 256-thread workgroup owns one row and a run of nf consecutive frames: it stages the
//     span of the extended row those frames cover into LDS once (zeros or whole-sample reflection past the ends), builds the n_fft / 2 roots
//     of unity e^{-2 pi i j / n_fft} with sincospif (j / n_fft is exact), then transforms frame by frame.  T = min(256, n_fft / 4) threads
//     form a group that owns one frame at a time (256 / T frames in flight): a thread takes four elements through two levels in registers,
//     so a transform costs ceil(log2(n_fft) / 2) barriers and LDS round trips, with the operations of the plain radix-2 scheme.  Per taper the
//     group writes v[n] = taper[n] (xe[n] - m) (0 behind n_win: set, never multiplied) as a complex sequence with zero imaginary part and
//     runs an in-place radix-2 decimation-in-frequency FFT in LDS; the result sits in bit-reversed order, which costs nothing because
//     only |X[k]|^2 is read back (at brev(k)).  A thread owns its bins of the frame's power row in LDS: acc = acc + w2[t] |X_t[k]|^2 in
//     ascending t from the first taper's term, then P = (scale c_k) acc, stored to `power` and left in LDS for the band sums (one thread per band, ascending k from
//     +0).  The operations on a frame, and their order, depend on n_fft, n_win, K and the frame's own samples only: not on the row, the
//     frame index, nf or the grid.  Every sequence is transformed as it is (no two-frame packing: the Hermitian split would tie a frame's
//     rounding to its partner).  No atomics, no memset, one writer per element.
//   * pac_intervals_kernel: one wave per interval, float64 terms from fp32 inputs, a lane's chain over samples start + lane, + 64, ... in
//     ascending order, then a fixed xor butterfly.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int TFR_MAX_K = 8, TFR_MAX_NB = 16, TFR_MIN_NFFT = 64, TFR_MAX_NFFT = 4096;
constexpr int TFR_SPAN_MAX = 8192;                                   // floats of the staged span (32 KiB)
constexpr int TFR_LDS_MAX = (TFR_MAX_NFFT / 2) * 8 + TFR_MAX_NFFT * 8 + (TFR_MAX_NFFT / 2 + 4) * 4 + TFR_SPAN_MAX * 4;

struct StftArgs {
  const float* x; long ldx; long L; long F;
  const float* tapers;
  float* power; float* bands;
  int n_win, hop, n_fft, log2n, K, centre, edge, detrend, onesided, k0, k1, NB, nf;
  long nchunk;
  float scale;
  float w2[TFR_MAX_K];
  int blo[TFR_MAX_NB], bhi[TFR_MAX_NB];
};

// one radix-2 decimation-in-frequency butterfly: u <- u + v, v <- (u - v) w
__device__ __forceinline__ void bfly(float2& u, float2& v, const float2 w) {
  const float dx = u.x - v.x, dy = u.y - v.y;
  u = make_float2(u.x + v.x, u.y + v.y);
  v = make_float2(dx * w.x - dy * w.y, dx * w.y + dy * w.x);
}

__global__ __launch_bounds__(NT) void stft_power_kernel(const StftArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float sRed[NT / 64], sW2[TFR_MAX_K];
  __shared__ int sBlo[TFR_MAX_NB], sBhi[TFR_MAX_NB];
  const int N = a.n_fft, H = N >> 1, NBIN = H + 1, PP = NBIN + 3;
  const int lt = a.log2n - 2 < 8 ? a.log2n - 2 : 8;                  // T = 2^lt = min(256, n_fft / 4) threads per transform
  const int T = 1 << lt, G = NT >> lt;
  float2* sTw = reinterpret_cast<float2*>(smem);                     // [H]
  float2* sZall = sTw + H;                                           // [G][N]
  float* sPall = reinterpret_cast<float*>(sZall + (size_t)G * N);    // [G][PP]
  float* sX = sPall + G * PP;                                        // [(nf - 1) hop + n_win]
  const int tid = threadIdx.x, g = tid >> lt, j = tid & (T - 1);
  const long b = (long)blockIdx.x / a.nchunk;
  const long f0 = ((long)blockIdx.x - b * a.nchunk) * a.nf;
  const int nf = (int)(a.F - f0 < a.nf ? a.F - f0 : a.nf);           // >= 1: the grid holds no empty chunk
  const int n_win = a.n_win, hop = a.hop;
  const long L = a.L;
  const long s0 = f0 * hop - (a.centre ? n_win / 2 : 0);
  const int span = (nf - 1) * hop + n_win;                           // <= TFR_SPAN_MAX (the host's choice of nf)
  const float* xr = a.x + b * a.ldx;
  for (int i = tid; i < span; i += NT) {
    long p = s0 + i;                                                 // in [-h, L - 1 + h] when centred, inside the row otherwise
    float v = 0.f;
    if (a.edge) {
      p = p < 0 ? -p : (p > L - 1 ? 2 * (L - 1) - p : p);            // h <= L - 1 (checked by the caller): back inside the row
      v = xr[p];
    } else if (p >= 0 && p < L) {
      v = xr[p];
    }
    sX[i] = v;
  }
  for (int i = tid; i < H; i += NT) {
    float s, c;
    sincospif(-2.0f * (float)i / (float)N, &s, &c);
    sTw[i] = make_float2(c, s);
  }
  if (tid == 0) {
#pragma unroll
    for (int t = 0; t < TFR_MAX_K; t++) sW2[t] = a.w2[t];
#pragma unroll
    for (int q = 0; q < TFR_MAX_NB; q++) { sBlo[q] = a.blo[q]; sBhi[q] = a.bhi[q]; }
  }
  __syncthreads();

  float2* z = sZall + (size_t)g * N;
  float* sP = sPall + g * PP;
  const int brs = 32 - a.log2n;
  for (int base = 0; base < nf; base += G) {                          // every thread runs every barrier: a group past the run computes and stores nothing
    const bool live = base + g < nf;
    const int fi = live ? base + g : base;
    const float* fx = sX + fi * hop;
    float m = 0.f;
    if (a.detrend) {                                                 // lane chains in ascending n, xor butterfly, then the group's waves in order
      float s = 0.f;
      for (int n = j; n < n_win; n += T) s = s + fx[n];
      for (int o = T >= 64 ? 32 : T >> 1; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
      if (T > 64) {
        if ((tid & 63) == 0) sRed[tid >> 6] = s;
        __syncthreads();
        const int w0 = g * (T >> 6);                                  // T == 128: two waves per group; T == 256: four
        s = sRed[w0];
        for (int w = 1; w < (T >> 6); w++) s = s + sRed[w0 + w];
      }
      m = s / (float)n_win;
    }
    for (int t = 0; t < a.K; t++) {
      const float* tp = a.tapers + (long)t * n_win;
      for (int n = j; n < N; n += T) {
        float v = 0.f;
        if (n < n_win) v = tp[n] * (fx[n] - m);
        z[n] = make_float2(v, 0.f);
      }
      __syncthreads();
      int s = 0;
      for (; s + 2 <= a.log2n; s += 2) {                             // levels s and s + 1 on four elements in registers: the operations of two radix-2 levels
        const int lh = a.log2n - 1 - s, h = 1 << lh, hh = h >> 1;
        for (int q = j; q < (N >> 2); q += T) {
          const int r = q & (hh - 1), i = ((q >> (lh - 1)) << (lh + 1)) | r;
          float2 e0 = z[i], e1 = z[i + hh], e2 = z[i + h], e3 = z[i + h + hh];
          bfly(e0, e2, sTw[r << s]); bfly(e1, e3, sTw[(r + hh) << s]);
          const float2 w = sTw[r << (s + 1)];
          bfly(e0, e1, w); bfly(e2, e3, w);
          z[i] = e0; z[i + hh] = e1; z[i + h] = e2; z[i + h + hh] = e3;
        }
        __syncthreads();
      }
      if (s < a.log2n) {                                             // an odd number of levels: the last one (h = 1, root 1) alone
        for (int q = j; q < H; q += T) {
          float2 e0 = z[2 * q], e1 = z[2 * q + 1];
          bfly(e0, e1, sTw[0]);
          z[2 * q] = e0; z[2 * q + 1] = e1;
        }
        __syncthreads();
      }
      const float wt = sW2[t];
      for (int k = j; k < NBIN; k += T) {
        const float2 X = z[__brev((unsigned)k) >> brs];
        const float p = wt * (X.x * X.x + X.y * X.y);
        sP[k] = t == 0 ? p : sP[k] + p;
      }
      __syncthreads();
    }
    const long fr = b * a.F + f0 + fi;
    for (int k = j; k < NBIN; k += T) {
      const float ck = (a.onesided && k > 0 && k < H) ? 2.0f : 1.0f;
      const float P = (a.scale * ck) * sP[k];
      sP[k] = P;
      if (a.power && live && k >= a.k0 && k < a.k1) a.power[fr * (a.k1 - a.k0) + (k - a.k0)] = P;
    }
    if (a.bands) {
      __syncthreads();
      if (live && j < a.NB) {
        float s = 0.f;
        for (int k = sBlo[j]; k < sBhi[j]; k++) s = s + sP[k];
        a.bands[fr * a.NB + j] = s;
      }
    }
  }
}

__global__ __launch_bounds__(NT) void pac_intervals_kernel(const float* __restrict__ pr, long ldr, const float* __restrict__ pi, long ldi,
                                                           const float* __restrict__ amp, long lda, const int* __restrict__ iv, long NI, long B,
                                                           long L, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long q = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (q >= NI) return;
  long row = q, start = 0, len = L;
  if (iv) { row = iv[3 * q]; start = iv[3 * q + 1]; len = iv[3 * q + 2]; }
  if (!(row >= 0 && row < B && start >= 0 && len >= 1 && start + len <= L)) {       // out of range: not a fault
    if (lane < 4) out[4 * q + lane] = lane == 0 ? -1.0 : 0.0;
    return;
  }
  const float* rr = pr + row * ldr; const float* ri = pi + row * ldi; const float* ra = amp + row * lda;
  double n = 0.0, sa = 0.0, sc = 0.0, ss = 0.0;
  for (long i = start + lane; i < start + len; i += 64) {
    const float af = ra[i], xf = rr[i], yf = ri[i];
    if (!(__builtin_isfinite(af) && __builtin_isfinite(xf) && __builtin_isfinite(yf))) continue;
    const double A = af, X = xf, Y = yf;
    const double h = sqrt(X * X + Y * Y);
    if (!(h > 0.0)) continue;
    n = n + 1.0; sa = sa + A; sc = sc + A * X / h; ss = ss + A * Y / h;
  }
  n = wave_sum_d(n); sa = wave_sum_d(sa); sc = wave_sum_d(sc); ss = wave_sum_d(ss);
  if (lane == 0) { double* o = out + 4 * q; o[0] = n; o[1] = sa; o[2] = sc; o[3] = ss; }
}

int tfr_log2(int n) { int l = 0; while ((1 << l) < n) l++; return l; }
}  // namespace

extern "C" long eegldm_stft_num_frames(long L, int n_win, int hop, int centre) {
  if (L < 0 || n_win < 1 || hop < 1 || (centre != 0 && centre != 1)) return -1;
  if (centre) return L >= 1 ? (L - 1) / hop + 1 : 0;
  return L >= n_win ? (L - n_win) / hop + 1 : 0;
}

extern "C" int eegldm_stft_power(eegldm_ctx* ctx, const float* x, long ldx, long B, long L, const float* tapers, const float* w2_host, int K,
                                 int n_win, int n_fft, int hop, int centre, int edge, int detrend, int onesided, float scale, int k0, int k1,
                                 float* power, const int* bands_host, int NB, float* bands) {
  EEG_CHECK(ctx && x && tapers && w2_host, "null argument");
  EEG_CHECK(power || bands, "both outputs are NULL");
  EEG_CHECK(n_fft >= TFR_MIN_NFFT && n_fft <= TFR_MAX_NFFT && (n_fft & (n_fft - 1)) == 0, "n_fft %d is not one of 64, 128, ..., 4096", n_fft);
  EEG_CHECK(n_win >= 1 && n_win <= n_fft, "n_win %d outside [1, n_fft = %d]", n_win, n_fft);
  EEG_CHECK(hop >= 1, "hop %d < 1", hop);
  EEG_CHECK(K >= 1 && K <= TFR_MAX_K, "K %d outside [1, %d]", K, TFR_MAX_K);
  EEG_CHECK((centre == 0 || centre == 1) && (edge == 0 || edge == 1), "centre %d / edge %d must be 0 or 1", centre, edge);
  EEG_CHECK((detrend == 0 || detrend == 1) && (onesided == 0 || onesided == 1), "detrend %d / onesided %d must be 0 or 1", detrend, onesided);
  EEG_CHECK(B >= 0 && L >= 0 && L <= (1L << 40), "B %ld / L %ld out of range", B, L);
  EEG_CHECK(ldx >= L, "row stride %ld shorter than L %ld", ldx, L);
  for (int t = 0; t < K; t++) EEG_CHECK(w2_host[t] >= 0.f && w2_host[t] <= 3.402823466e38f, "w2[%d] = %g is not a finite non-negative weight", t, (double)w2_host[t]);
  const int nbin = n_fft / 2 + 1;
  if (power) EEG_CHECK(k0 >= 0 && k0 < k1 && k1 <= nbin, "bin range [%d, %d) outside [0, %d)", k0, k1, nbin);
  if (bands) {
    EEG_CHECK(bands_host, "bands without bin ranges");
    EEG_CHECK(NB >= 1 && NB <= TFR_MAX_NB, "NB %d outside [1, %d]", NB, TFR_MAX_NB);
    for (int q = 0; q < NB; q++)
      EEG_CHECK(bands_host[2 * q] >= 0 && bands_host[2 * q] < bands_host[2 * q + 1] && bands_host[2 * q + 1] <= nbin,
                "band %d = [%d, %d) outside [0, %d)", q, bands_host[2 * q], bands_host[2 * q + 1], nbin);
  }
  EEG_CHECK(!(centre == 1 && edge == 1 && L >= 1 && n_win / 2 > L - 1), "reflect needs n_win / 2 <= L - 1, got n_win %d L %ld", n_win, L);
  EEG_CHECK((((uintptr_t)x | (uintptr_t)tapers | (uintptr_t)power | (uintptr_t)bands) & 3u) == 0, "float pointers must be 4-byte aligned");
  const long F = eegldm_stft_num_frames(L, n_win, hop, centre);
  if (F == 0 || B == 0) return 0;

  StftArgs a = {};
  a.x = x; a.ldx = ldx; a.L = L; a.F = F; a.tapers = tapers; a.power = power; a.bands = bands;
  a.n_win = n_win; a.hop = hop; a.n_fft = n_fft; a.log2n = tfr_log2(n_fft); a.K = K; a.centre = centre; a.edge = centre ? edge : 0;
  a.detrend = detrend; a.onesided = onesided; a.k0 = power ? k0 : 0; a.k1 = power ? k1 : 0; a.NB = bands ? NB : 0; a.scale = scale;
  for (int t = 0; t < K; t++) a.w2[t] = w2_host[t];
  for (int q = 0; q < a.NB; q++) { a.blo[q] = bands_host[2 * q]; a.bhi[q] = bands_host[2 * q + 1]; }
  // frames per workgroup: as many as the staged span holds, fewer while the grid is smaller than two workgroups per CU (never fewer than the
  // 256 / T frames in flight).  The choice changes no bit.
  const int T = n_fft / 4 < NT ? n_fft / 4 : NT, G = NT / T;
  long nf = 1 + (TFR_SPAN_MAX - n_win) / hop;
  if (nf > F) nf = F;
  while (nf > G && B * ((F + nf - 1) / nf) < 2L * ctx->num_cu) nf = (nf + 1) / 2 > G ? (nf + 1) / 2 : G;
  a.nf = (int)nf;
  a.nchunk = (F + nf - 1) / nf;
  EEG_CHECK(a.nchunk <= 0x7fffffffL / (B > 0 ? B : 1), "B %ld x %ld frame chunks exceed the grid", B, a.nchunk);
  const size_t lds = (size_t)(n_fft / 2) * 8 + (size_t)G * n_fft * 8 + (size_t)G * (nbin + 3) * 4 + ((size_t)(nf - 1) * hop + n_win) * 4;
  static DevOnce attr;
  if (attr.need(ctx->device))
    HIP_TRY(hipFuncSetAttribute((const void*)stft_power_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TFR_LDS_MAX));
  hipLaunchKernelGGL(stft_power_kernel, dim3((unsigned)(B * a.nchunk)), dim3(NT), lds, ctx->stream, a);
  LAUNCH_CHECK();
  return 0;
}

extern "C" int eegldm_pac_intervals(eegldm_ctx* ctx, const float* pr, long ldr, const float* pi, long ldi, const float* amp, long lda, long B,
                                    long L, const int* iv, long NI, double* out) {
  EEG_CHECK(ctx && pr && pi && amp && out, "null argument");
  EEG_CHECK(B >= 0 && B <= 0x7fffffffL && L >= 1 && L <= 0x7fffffffL, "B %ld / L %ld out of range", B, L);
  EEG_CHECK(NI >= 0 && NI <= 0x7fffffffL, "NI %ld outside [0, 2^31)", NI);
  EEG_CHECK(iv || NI == B, "iv == NULL needs NI == B, got NI %ld B %ld", NI, B);
  EEG_CHECK(ldr >= L && ldi >= L && lda >= L, "row strides %ld / %ld / %ld shorter than L %ld", ldr, ldi, lda, L);
  EEG_CHECK((((uintptr_t)pr | (uintptr_t)pi | (uintptr_t)amp | (uintptr_t)iv) & 3u) == 0, "float and int pointers must be 4-byte aligned");
  EEG_CHECK(((uintptr_t)out & 7u) == 0, "out must be 8-byte aligned");
  if (NI == 0) return 0;
  hipLaunchKernelGGL(pac_intervals_kernel, dim3((unsigned)((NI + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, ctx->stream, pr, ldr, pi, ldi, amp, lda,
                     iv, NI, B, L, out);
  LAUNCH_CHECK();
  return 0;
}
