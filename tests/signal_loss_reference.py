"""Float64 references, first-order rounding bounds, fp32 CPU models and the shared cases of the signal-domain losses and metrics:
csrc/spectral.hip (eegldm_spectral_loss), csrc/losses.hip (eegldm_l1_loss, eegldm_lsgan_loss), csrc/metrics.hip (eegldm_ms_ssim_1d,
eegldm_psd_multitaper).  Imported by tests/test_signal_loss_numerics_cpu.py and tests/test_gpu_signal_loss_rounding.py; not a conftest.

Every input is an fp32 value handed to float64 unchanged.  Each `*_reference` restates the operation from its definition in numpy float64
and returns, beside the value, an absolute bound built from float64 quantities only: u = 2^-24, numerics.gamma(n) = (n + 4) u with the
chain lengths n read off the kernel (stated in each docstring), propagated to first order and doubled (SAFETY) for the higher orders, as
tests/test_gpu_usleep_train.py does.  Second-order terms are kept where the first order vanishes (a loss of exactly 0, a PSD bin far
from a spectral line).

Each `*_model` is the kernel's arithmetic in numpy float32 at the kernel's chain lengths (numpy's sums and matrix products add in another
order; the bounds hold for every order).  `defect=` plants one mistake at a time; the CPU test demands that each one is caught."""
import math

import numpy as np

import numerics

U = 2.0 ** -24
SAFETY = 2.0
NT = 256                                      # threads of every kernel here
gamma = numerics.gamma
f32, f64 = np.float32, np.float64

FFT_SPLIT = {3072: (48, 64), 768: (24, 32), 256: (16, 16), 96: (8, 12)}      # spectral.hip: N = N1 x N2
GATE = 1e-10                                  # G_k = 0 where A_k^2 <= GATE x recon's mean bin power
GATE_MARGIN = 16.0


def _rng(*key):
    return np.random.default_rng([20260, *key])


def l2_err(got, ref):
    """L2 norm of got - ref (the callers divide by the norm of the reference gradient)"""
    d = np.asarray(got, f64) - np.asarray(ref, f64)
    return float(np.sqrt((d * d).sum()))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 = 0; anything outside a zero bound, or a non-finite value, = inf)"""
    got, ref, bound = np.asarray(got, f64), np.asarray(ref, f64), np.broadcast_to(np.asarray(bound, f64), np.shape(ref))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(got), r, np.inf)
    return float(np.max(r)) if r.size else 0.0


def report(case, n, worst, extra=""):
    print(f"[numerics] {case:<52s} n={n:>7d} worst={worst:.2e}xbound{extra}")


# ==================================================================================================== spectral loss
def spectral_chains(L):
    """(m, m2).  spectral.hip transforms each window by a four-step DFT: N1-point DFTs of the REAL samples (each output a chain of N1
    products), a twiddle, N2-point DFTs of complex values (2 N2 real products per output, two per complex MAC; |v.x w.x| + |v.y w.y| <= |v|).
    Roundings beside the chains: the sin/cos table (2u per stage), the twiddle (table 2u, product and sum 2), rsqrt(N) (2u) and the product
    by it (1): 11.  Per bin and to first order |dR_k| <= gamma(m) ||recon||_1 / sqrt(N) <= gamma(m) ||recon||_2 with m = N1 + 2 N2 + 12:
    e_R has no term in the target, because the target is not in the transform.  The backward transform has a complex input, 2 N1 + 2 N2
    and the same tables: m2 = 2 (N1 + N2) + 12."""
    N1, N2 = FFT_SPLIT[L]
    return N1 + 2 * N2 + 12, 2 * (N1 + N2) + 12


def spectral_reference(recon, target, acc=None, gw=1.0):
    """recon, target (B, L) -> dict.  R = FFT_ortho(recon), T = FFT_ortho(target), A = |R|, B = |T|, d = A - B, loss = sum d^2 over bins
    and windows; G_k = 2 d_k conj(R_k) / A_k, 0 where A_k^2 <= 1e-10 x recon's mean bin power (sum recon^2 / N by Parseval);
    out = acc + gw Re FFT_ortho(G).
    Bounds (first order, x SAFETY):
      e_R = gamma(m) ||recon||_2, e_T = gamma(m) ||target||_2 per bin (spectral_chains);  e_A = e_R + 4u A (two squares, sum, sqrt), e_B alike
      e_d = e_A + e_B + u |d|
      loss  sum_k (2 |d| e_d + e_d^2) + gamma(N / 256 + 10) sum d^2 per window (per-thread chain N / 256, 6 wave levels, 3 partials, the
            square), + gamma(B) loss for the B atomic additions (or the ordered fold of the deterministic mode)
      e_G = 2 e_d + 2 |d| (e_A + e_R) / A + 12u |d|  (g = 2 d / A: e_d / A and |d| e_A / A^2, three roundings; G = g conj R: |g| e_R --
            the |d| e_R / A term that grows at weak bins)
      grad  (sum_k e_G + gamma(m2) sum_k |G_k|) / sqrt(N): the exact transform of the input errors plus the transform's own rounding
      out   |gw| e_grad + 6u |gw grad| (gw * rsqrt(N), the product) + 2u |out| (the accumulation)
    `margin` = min over bins of max(A^2 / thr, thr / A^2): the condition on the inputs (>= GATE_MARGIN)."""
    r, t = np.asarray(recon, f64), np.asarray(target, f64)
    B, L = r.shape
    m, m2 = spectral_chains(L)
    R, T = np.fft.fft(r, axis=-1, norm="ortho"), np.fft.fft(t, axis=-1, norm="ortho")
    A, Bm = np.abs(R), np.abs(T)
    d = A - Bm
    en = (r * r).sum(-1)
    thr = (GATE * en / L)[:, None]
    opn = A * A > thr
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(thr > 0, A * A / thr, np.where(A > 0, np.inf, 0.0))
        margin = np.where(ratio > 1, ratio, np.where(ratio > 0, 1.0 / ratio, np.inf))
    eR = gamma(m) * np.sqrt(en)[:, None]; eT = gamma(m) * np.sqrt((t * t).sum(-1))[:, None]
    eA, eB = eR + 4 * U * A, eT + 4 * U * Bm
    ed = eA + eB + U * np.abs(d)
    loss_w = (d * d).sum(-1)
    e_loss_w = (2 * np.abs(d) * ed + ed * ed).sum(-1) + gamma(math.ceil(L / NT) + 10) * loss_w
    loss = float(loss_w.sum())
    As = np.where(opn, A, 1.0)
    G = np.where(opn, 2 * d * np.conj(R) / As, 0.0)
    eG = np.where(opn, 2 * ed + 2 * np.abs(d) * (eA + eR) / As + 12 * U * np.abs(d), 0.0)
    grad = np.fft.fft(G, axis=-1, norm="ortho").real
    e_grad = ((eG.sum(-1) + gamma(m2) * np.abs(G).sum(-1)) / math.sqrt(L))[:, None]
    a0 = np.zeros_like(r) if acc is None else np.asarray(acc, f64)
    out = a0 + gw * grad
    e_out = SAFETY * (abs(gw) * e_grad + 6 * U * np.abs(gw * grad) + 2 * U * np.abs(out))
    return dict(loss=loss, e_loss=SAFETY * (float(e_loss_w.sum()) + gamma(B) * loss), loss_w=loss_w, grad=grad, out=out, e_out=e_out,
                open=opn, margin=float(margin.min()), gnorm=abs(gw) * float(np.sqrt((grad * grad).sum())))


def _roots(L):
    j = np.arange(L, dtype=f64)
    return (np.cos(-2 * np.pi * j / L) + 1j * np.sin(-2 * np.pi * j / L)).astype(np.complex64)


def fft4(a, twiddle_off=0):
    """(B, L) complex64 -> (unnormalised forward DFT in natural order, the intermediate Y (B, N1, N2)): the kernel's four steps in fp32"""
    B, L = a.shape
    N1, N2 = FFT_SPLIT[L]
    tw = _roots(L)
    i1, i2 = np.arange(N1), np.arange(N2)
    F1 = tw[(N2 * np.outer(i1, i1)) % L]                      # [k1][n1] W_N1^(n1 k1)
    Y = np.matmul(F1, a.reshape(B, N1, N2))                    # a[N2 n1 + n2] -> [k1][n2]
    Y = Y * tw[np.outer(i1, i2 + twiddle_off) % L]             # W_N^(n2 k1)
    F2 = tw[(N1 * np.outer(i2, i2)) % L]                       # [n2][k2] W_N2^(n2 k2)
    X = np.matmul(Y, F2)                                       # [k1][k2] -> index k1 + N1 k2
    assert X.dtype == np.complex64
    return np.ascontiguousarray(X.transpose(0, 2, 1)).reshape(B, L), Y


def spectral_model(recon, target, acc=None, gw=1.0, variant="decoupled", defect=None):
    """fp32 model -> (loss, out (B, L)).  variant "decoupled": the kernel -- one transform per window, gate on recon's own power -- and,
    its sums in another order, the yardstick of check B (what a plain fp32 evaluation achieves); "packed": the kernel before the repair
    (one transform of recon + i target, the spectra separated by the Hermitian identities, gate on the combined power).
    defect: "sign" (-g ri loses its sign), "twiddle" (n2 off by one in the twiddle's index; an offset of the
    whole index would be a phase common to all bins, which the amplitudes and the backward transform cancel), "noscale" (rsqrt(N) missing on the backward transform),
    "overwrite" (the gradient replaces the accumulator), "herm0" ("packed" only: the Hermitian partner of bin 0 read at index N, one past the
    spectrum, where the kernel's scratch began -- the first element of the intermediate Y; the repair removed the separation, so the
    kernel has no place left where this mistake could occur, and the defect is kept for the arithmetic it belonged to)."""
    r, t = np.asarray(recon, f32), np.asarray(target, f32)
    B, L = r.shape
    off = 1 if defect == "twiddle" else 0
    scale = f32(1.0 / math.sqrt(L))
    en_r, en_t = (r * r).sum(-1, dtype=f32), (t * t).sum(-1, dtype=f32)
    partner = (-np.arange(L)) % L

    def c64(re, im=None):
        z = np.zeros(re.shape, np.complex64); z.real = re
        if im is not None:
            z.imag = im
        return z

    if variant == "decoupled":
        assert defect != "herm0", "the Hermitian separation exists in the packed variant only"
        R, T = fft4(c64(r), off)[0] * scale, fft4(c64(t), off)[0] * scale
        thr = f32(GATE) * en_r / f32(L)
    else:
        thr = f32(GATE) * (en_r + en_t) / f32(L)
        Z, Y = fft4(c64(r, t), off)
        Zm = np.conj(Z[:, partner])
        if defect == "herm0":
            Zm[:, 0] = np.conj(Y[:, 0, 0])
        R = (f32(0.5) * scale) * (Z + Zm)
        T = (f32(0.5) * scale) * ((Z - Zm) * np.complex64(-1j))
    A, Bm = np.abs(R), np.abs(T)
    d = A - Bm
    loss = float((d * d).sum(-1, dtype=f32).sum(dtype=f32))
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(A * A > thr[:, None], f32(2) * d / A, f32(0)).astype(f32)
    G = g * (R if defect == "sign" else np.conj(R))
    X = fft4(G.astype(np.complex64), off)[0].real
    grad = (f32(gw) * X) if defect == "noscale" else (f32(gw) * scale) * X
    a0 = np.zeros_like(r) if acc is None else np.asarray(acc, f32)
    out = grad if defect == "overwrite" else a0 + grad
    assert out.dtype == f32 and A.dtype == f32
    return loss, out


def _smooth(rng, B, L):
    w = min(31, max(3, L // 8))
    x = rng.standard_normal((B, L + w - 1))
    s = np.stack([np.convolve(x[b], np.ones(w) / w, mode="valid") for b in range(B)])
    return s / np.sqrt((s * s).mean(-1, keepdims=True))


def spectral_cases(L, B=3):
    """name -> (recon, target) fp32 (B, L), the same cases at every L.  The unit target is a 10-cycles-per-128-samples sinusoid plus
    0.5 white noise; `smooth` is a moving average of white noise at unit rms."""
    rng = _rng(1, L)
    n = np.arange(L)
    unit = (np.sin(2 * np.pi * 10 * n / 128.0 + rng.uniform(0, 6.28, (B, 1))) + 0.5 * rng.standard_normal((B, L))).astype(f32)
    cases = {"matched": ((unit + 0.05 * rng.standard_normal((B, L))).astype(f32), unit)}
    for s in (1e-1, 1e-2, 1e-3, 1e-5):
        cases[f"small_{s:.0e}"] = ((s * (_smooth(rng, B, L) + 0.05 * rng.standard_normal((B, L)))).astype(f32), unit)
    cases["swap"] = (unit, (1e-3 * (_smooth(rng, B, L) + 0.05 * rng.standard_normal((B, L)))).astype(f32))
    cases["identical"] = (unit.copy(), unit)
    cases["offset"] = ((unit + 0.05 * rng.standard_normal((B, L)) + 30.0).astype(f32), (unit + 30.0).astype(f32))
    bins = [k for k in (3, 7, 11, 20, 29, 41) if k < L // 2]
    band = sum(rng.uniform(0.5, 1.0, (B, 1)) * np.cos(2 * np.pi * k * n / L + rng.uniform(0, 6.28, (B, 1))) for k in bins).astype(f32)
    band[1] = 0.0
    cases["bandlimited"] = (band, unit)
    return cases


SPECTRAL_CHECK_B = ("matched", "small_1e-01", "small_1e-02", "small_1e-03", "small_1e-05", "swap", "offset", "bandlimited")
SPECTRAL_UNGATED = ("matched", "small_1e-01", "small_1e-02", "small_1e-03", "small_1e-05", "swap", "identical", "offset")


# ==================================================================================================== L1 and least-squares GAN
LOSS_N = (1, 255, 257, 3 * 3072 + 1)
SLOPE = 0.05


def loss_blocks(n, kind):
    """grid of losses.hip for the sizes of these tests (far below the cap of 16 blocks per CU): L1 walks four elements per thread"""
    return max(1, math.ceil((n // 4 + 1 if kind == "l1" else n) / NT))


def _sum_chain(n, kind):
    """per-thread chain n / (blocks x 256), 6 wave levels, 3 partials, one atomic addition (or fold step) per block, 1 / (float) n and the
    product by it (2), the element's own roundings (L1: the difference; LSGAN: counted per term)"""
    nb = loss_blocks(n, kind)
    return math.ceil(n / (nb * NT)) + 9 + nb + 3


def l1_reference(a, b, da0=None, gw=1.0):
    """loss = mean |a - b|, out = da0 + gw sign(a - b) / n with sign(0) = 0 -> (loss, e_loss, out, e_out).
    loss: gamma(_sum_chain) sum |a - b| / n.  Gradient: 1 / (float) n and gw * (1 / n) are two roundings, the sign is exact, the
    accumulation one more: 2u |g| + u |out|."""
    a, b = np.asarray(a, f64).reshape(-1), np.asarray(b, f64).reshape(-1)
    n = a.size
    d = a - b
    loss = float(np.abs(d).sum() / n)
    g = gw * np.sign(d) / n
    out = g if da0 is None else np.asarray(da0, f64).reshape(-1) + g
    return loss, SAFETY * gamma(_sum_chain(n, "l1")) * loss, out, SAFETY * (2 * U * np.abs(g) + U * np.abs(out))


def l1_model(a, b, da0=None, gw=1.0, defect=None):
    """defect: "sign0" (sign(0) = 1), "inv_n" (1 / (n + 1))"""
    a, b = np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1)
    n = a.size
    inv_n = f32(1) / f32(n + 1 if defect == "inv_n" else n)
    d = a - b
    loss = float(np.abs(d).sum(dtype=f32) * inv_n)
    s = np.where(d > 0, f32(1), np.where(d < 0, f32(-1), f32(1 if defect == "sign0" else 0))).astype(f32)
    g = (f32(gw) * inv_n) * s
    return loss, (g if da0 is None else np.asarray(da0, f32).reshape(-1) + g)


def lsgan_reference(x, real, gw=1.0):
    """a = x (x > 0) or 0.05 x; loss = mean (a - target)^2; dlogit = gw 2 (a - target) / n x (1 if x > 0 else 0.05): at a logit of exactly 0
    the derivative is the negative slope -> (loss, e_loss, dl, e_dl).
    e_a = 2u |a| on the negative branch (fp32(0.05) and the product), e_d = e_a + u |d|; a term d^2 carries 2 |d| e_d + e_d^2 + u d^2;
    the sum gamma(_sum_chain) sum d^2 / n.  Gradient: |gw| 2 slope e_d / n + 5u |dl| (three products, 1 / (float) n, fp32(0.05))."""
    x = np.asarray(x, f64).reshape(-1)
    n = x.size
    tgt = 1.0 if real else 0.0
    pos = x > 0
    a = np.where(pos, x, SLOPE * x)
    d = a - tgt
    ed = np.where(pos, 0.0, 2 * U * np.abs(a)) + U * np.abs(d)
    loss = float((d * d).sum() / n)
    e_loss = SAFETY * (float((2 * np.abs(d) * ed + ed * ed + U * d * d).sum() / n) + gamma(_sum_chain(n, "lsgan")) * loss)
    sl = np.where(pos, 1.0, SLOPE)
    dl = gw * 2 * d / n * sl
    return loss, e_loss, dl, SAFETY * (abs(gw) * 2 * sl * ed / n + 5 * U * np.abs(dl))


def lsgan_model(x, real, gw=1.0, defect=None):
    """defect: "slope0" (slope 1 at a logit of 0), "inv_n" (1 / (n + 1))"""
    x = np.asarray(x, f32).reshape(-1)
    n = x.size
    inv_n = f32(1) / f32(n + 1 if defect == "inv_n" else n)
    a = np.where(x > 0, x, f32(SLOPE) * x).astype(f32)
    d = a - f32(1.0 if real else 0.0)
    loss = float((d * d).sum(dtype=f32) * inv_n)
    one = (x >= 0) if defect == "slope0" else (x > 0)
    dl = f32(gw) * f32(2) * d * inv_n * np.where(one, f32(1), f32(SLOPE)).astype(f32)
    assert dl.dtype == f32
    return loss, dl


def loss_case(n, seed=0):
    """(a, b, logits): unit normal values; elements with a == b, among them +0 against -0, and logits of exactly +0 and -0 (n = 1: the
    single element is one of them)"""
    rng = _rng(2, n, seed)
    a, b, x = (rng.standard_normal(n).astype(f32) for _ in range(3))
    eq = np.arange(0, n, 5)
    b[eq] = a[eq]
    a[0], b[0] = f32(0.0), f32(-0.0)
    x[0] = f32(0.0)
    if n > 7:
        x[7] = f32(-0.0)
    return a, b, x


# ==================================================================================================== multi-scale SSIM
SSIM_CASES = ((3, 48, 1), (7, 375, 2), (11, 3000, 1), (17, 4096, 1))
SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gaussian_1d(ks, sigma=1.5):
    dist = np.arange((1 - ks) / 2, (1 + ks) / 2, 1.0, dtype=f32)
    g = np.exp(-np.power(dist / f32(sigma), 2) / 2).astype(f32)
    return (g / g.sum()).astype(f32)


def _windows(x, ks):
    return np.lib.stride_tricks.sliding_window_view(x, ks, axis=-1)


def _pool(x):
    Ln = x.shape[-1] // 2
    return 0.5 * (x[..., 0:2 * Ln:2] + x[..., 1:2 * Ln:2])


def ms_ssim_reference(a, b, kernel, weights, data_range=1.0, k1=0.01, k2=0.03):
    """a, b (B, C, L) -> (value (B,), bound (B,)).  The reference's definition (compute_mmds' 1-D MultiScaleSSIMMetric): per scale the windowed
    moments m_x = sum_t k_t x_(p+t), m_xx, m_yy, m_xy over the valid positions, s_x = m_xx - m_x^2, s_xy = m_xy - m_x m_y,
    cs = (2 s_xy + c2) / (s_x + s_y + c2), ssim = (2 m_x m_y + c1) / (m_x^2 + m_y^2 + c1) cs; v_s = relu(mean over positions and channels)
    of cs, of ssim at the last scale; avg_pool1d(2) between scales (a trailing odd sample is dropped); value = prod v_s^w_s.
    Bound.  n_s = ks + 2 + 2 s: a chain of ks products, two roundings of a term k x y, and the s poolings (one rounding each, on x and on
    y) that produced the scale's samples.
      e_mx = gamma(n_s) sum |k x|, e_mxx = gamma(n_s) m_xx, e_mxy = gamma(n_s) sum |k x y|
      e_sx = e_mxx + 2 |m_x| e_mx + 2u m_x^2 + u |s_x|: the one-pass cancellation, gamma(ks + 2) (m_xx + m_x^2) and its kin; e_sxy alike
      c1, c2 are (k data_range)^2 in fp32: 3u each
      a ratio num / den: (e_num + |ratio| e_den) / (den - e_den) + u |ratio|  (den >= c > 0; infinite when e_den reaches den)
      means: the mean of the element bounds + gamma(Lo / 256 + 10) mean |.| over the positions, + gamma(C + 1) over the channels
    and, all x SAFETY, through the monotone prod relu(v_s)^w_s: the value lies between prod relu(v_s -+ e_s)^w_s, each power within 8u
    (powf) and each product within u.  Where v_s + e_s < 0 for some scale the bound is 0: the result must be exactly 0."""
    x, y = np.asarray(a, f64), np.asarray(b, f64)
    k = np.asarray(kernel, f32).astype(f64); w = np.asarray(weights, f32).astype(f64)
    ks, ns = len(k), len(w)
    B, C, _L = x.shape
    c1, c2 = (float(f32(k1)) * float(f32(data_range))) ** 2, (float(f32(k2)) * float(f32(data_range))) ** 2
    ak = np.abs(k)
    v, e = np.zeros((ns, B)), np.zeros((ns, B))

    def ratio(num, e_num, den, e_den):
        r = num / den
        room = den - e_den
        return r, np.where(room > 0, (e_num + np.abs(r) * e_den) / np.where(room > 0, room, 1.0), np.inf) + U * np.abs(r)

    for s in range(ns):
        g = gamma(ks + 2 + 2 * s)
        Wx, Wy = _windows(x, ks), _windows(y, ks)
        Lo = Wx.shape[-2]
        mx, my = Wx @ k, Wy @ k
        mxx, myy, mxy = (Wx * Wx) @ k, (Wy * Wy) @ k, (Wx * Wy) @ k
        e_mx, e_my = g * (np.abs(Wx) @ ak), g * (np.abs(Wy) @ ak)
        e_mxx, e_myy, e_mxy = g * ((Wx * Wx) @ ak), g * ((Wy * Wy) @ ak), g * (np.abs(Wx * Wy) @ ak)
        sx, sy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
        e_sx = e_mxx + 2 * np.abs(mx) * e_mx + 2 * U * mx * mx + U * np.abs(sx)
        e_sy = e_myy + 2 * np.abs(my) * e_my + 2 * U * my * my + U * np.abs(sy)
        e_sxy = e_mxy + np.abs(mx) * e_my + np.abs(my) * e_mx + 2 * U * np.abs(mx * my) + U * np.abs(sxy)
        num, den = 2 * sxy + c2, sx + sy + c2
        cs, e_cs = ratio(num, 2 * e_sxy + 3 * U * c2 + 2 * U * np.abs(num), den, e_sx + e_sy + 3 * U * c2 + 2 * U * den)
        if s == ns - 1:
            lnum, lden = 2 * mx * my + c1, mx * mx + my * my + c1
            lum, e_lum = ratio(lnum, 2 * (np.abs(mx) * e_my + np.abs(my) * e_mx) + 3 * U * c1 + 3 * U * np.abs(lnum),
                               lden, 2 * np.abs(mx) * e_mx + 2 * np.abs(my) * e_my + 3 * U * c1 + 3 * U * lden)
            q, e_q = lum * cs, np.abs(lum) * e_cs + np.abs(cs) * e_lum + U * np.abs(lum * cs)
        else:
            q, e_q = cs, e_cs
        mean_c = q.mean(-1); e_mean_c = e_q.mean(-1) + gamma(math.ceil(Lo / NT) + 10) * np.abs(q).mean(-1)        # (B, C)
        v[s] = mean_c.mean(-1)
        e[s] = SAFETY * (e_mean_c.mean(-1) + gamma(C + 1) * np.abs(mean_c).mean(-1))
        x, y = _pool(x), _pool(y)
    wv = w[:, None]
    val = np.prod(np.maximum(v, 0.0) ** wv, axis=0)
    hi = np.prod(np.maximum(v + e, 0.0) ** wv, axis=0) * (1 + 9 * ns * U)
    lo = np.prod(np.maximum(v - e, 0.0) ** wv, axis=0) * (1 - 9 * ns * U)
    return val, np.maximum(hi - val, val - lo)


def ms_ssim_model(a, b, kernel, weights, data_range=1.0, k1=0.01, k2=0.03, defect=None):
    """fp32 model of ms_ssim_kernel.  defect: "odd" (a trailing odd sample becomes an output of its own instead of being dropped), "ssim"
    (ssim in place of cs at the second scale, whose weight is 0.29), "nochan" (the channel mean missing), "c1c2" (the constants swapped)"""
    x, y = np.asarray(a, f32), np.asarray(b, f32)
    k = np.asarray(kernel, f32); w = np.asarray(weights, f32)
    ks, ns = len(k), len(w)
    B, C, _L = x.shape
    c1, c2 = (f32(k1) * f32(data_range)) ** 2, (f32(k2) * f32(data_range)) ** 2
    if defect == "c1c2":
        c1, c2 = c2, c1
    r = np.ones(B, f32)
    for s in range(ns):
        Wx, Wy = _windows(x, ks), _windows(y, ks)
        mx, my, mxx, myy, mxy = Wx @ k, Wy @ k, (Wx * Wx) @ k, (Wy * Wy) @ k, (Wx * Wy) @ k
        sx, sy, sxy = mxx - mx * mx, myy - my * my, mxy - mx * my
        cs = (f32(2) * sxy + c2) / (sx + sy + c2)
        ss = (f32(2) * mx * my + c1) / (mx * mx + my * my + c1) * cs
        q = ss if (s == ns - 1 or (defect == "ssim" and s == 1)) else cs
        m = q.mean(-1, dtype=f32)
        vs = m.sum(-1, dtype=f32) if defect == "nochan" else m.sum(-1, dtype=f32) / f32(C)
        r = r * np.power(np.maximum(vs, f32(0)), w[s]).astype(f32)
        if defect == "odd" and x.shape[-1] % 2:
            x = np.concatenate([f32(0.5) * (x[..., 0:-1:2] + x[..., 1::2]), x[..., -1:]], -1)
            y = np.concatenate([f32(0.5) * (y[..., 0:-1:2] + y[..., 1::2]), y[..., -1:]], -1)
        else:
            x, y = f32(0.5) * (x[..., 0:2 * (x.shape[-1] // 2):2] + x[..., 1:2 * (x.shape[-1] // 2):2]), \
                   f32(0.5) * (y[..., 0:2 * (y.shape[-1] // 2):2] + y[..., 1:2 * (y.shape[-1] // 2):2])
    assert r.dtype == f32
    return r


def ssim_case(ks, L, C, B=5):
    """[0, 1] windows as the workload's: a slow oscillation plus noise, clipped; y = x + 0.03 noise, clipped.  Pair 0 identical, pair 1
    anti-correlated (y = 1 - x), pair 2 offset by 10 data ranges (both windows + 10), pair 3 plain, pair 4 darker and flatter
    (y = 0.8 x + 0.05 + noise: the luminance term is 2 % below 1, so ssim and cs differ) and with last samples that disagree
    (1 against 0: whether a trailing odd sample is dropped shows in a share ks / Lo of the positions)."""
    rng = _rng(3, ks, L, C)
    n = np.arange(L)
    x = 0.5 + 0.25 * np.sin(2 * np.pi * n / 37.0 + rng.uniform(0, 6.28, (B, C, 1))) + 0.1 * rng.standard_normal((B, C, L))
    x = np.clip(x, 0, 1).astype(f32)
    y = np.clip(x + 0.03 * rng.standard_normal((B, C, L)), 0, 1).astype(f32)
    y[0] = x[0]
    y[1] = f32(1.0) - x[1]
    x[2] += f32(10.0); y[2] += f32(10.0)
    y[4] = np.clip(0.8 * x[4] + 0.05 + 0.03 * rng.standard_normal((C, L)), 0, 1).astype(f32)
    x[4, :, -1], y[4, :, -1] = f32(1.0), f32(0.0)
    return x, y


def ssim_refused(L, ks, n_scales):
    """the reference's guard, and every scale at least as long as the kernel"""
    div = max(1, n_scales - 1) ** 2
    return not (L // div > ks - 1) or (L >> (n_scales - 1)) < ks


# ==================================================================================================== multitaper PSD
PSD_CASES = ((2, 1), (255, 3), (256, 16), (3000, 7), (4096, 7))


def psd_reference(x, tapers, weights, sfreq, n_bins):
    """x (B, L), tapers (K, L), weights (K,) -> (psd (B, n_bins), bound).  De-mean, taper, one-sided DFT S_(t,k) = sum_n v_n e^(-2 pi i n k / L)
    with v = (x - mean) taper_t, psd_k = f_k sum_t w_t^2 |S_(t,k)|^2 / (sum_t w_t^2 sfreq), f_k = 2 except DC and (even L) Nyquist.
    Bound: the fp32 mean carries e_mean = gamma(L / 256 + 10) mean |x| (per-thread chain, 6 wave levels, 3 partials, the division), the
    same in every sample, so it reaches a bin as e_mean |sum_n taper e^(..)| <= e_mean sum |taper|; a chain of L products with the
    difference, the product by the taper, the table (2u) and the product by it: gamma(L + 6) sum |v_n|.  Real and imaginary part each:
    e_S = sqrt(2) (gamma(L + 6) sum |v| + e_mean sum |taper|); |S|^2: 2 |S| e_S + e_S^2 + 4u |S|^2 (the second order is what holds the
    bins far from a line, relative to the window's energy); the K weighted terms gamma(K + 2); w^2 in fp32, fp32(1 / (den sfreq)) and two
    products: 5u."""
    x, tp, w = np.asarray(x, f64), np.asarray(tapers, f64), np.asarray(weights, f64)
    B, L = x.shape
    K = tp.shape[0]
    mean = x.mean(-1, keepdims=True)
    xs = x - mean
    v = xs[:, None, :] * tp[None]
    S = np.abs(np.fft.rfft(v, axis=-1)[..., :n_bins])                                # (B, K, n_bins)
    e_mean = gamma(math.ceil(L / NT) + 10) * np.abs(x).mean(-1)                        # (B,)
    e_S = math.sqrt(2) * (gamma(L + 6) * np.abs(v).sum(-1) + e_mean[:, None] * np.abs(tp).sum(-1)[None])[..., None]      # (B, K, 1)
    P = S * S
    e_P = 2 * S * e_S + e_S * e_S + 4 * U * P
    w2 = (w * w)[None, :, None]
    fac = np.full(n_bins, 2.0); fac[0] = 1.0
    if L % 2 == 0 and n_bins == L // 2 + 1:
        fac[-1] = 1.0
    norm = fac / (float((w * w).sum()) * float(sfreq))
    acc = (w2 * P).sum(1)
    psd = acc * norm
    return psd, SAFETY * (((w2 * e_P).sum(1) + gamma(K + 2) * acc) * norm + 5 * U * psd)


def psd_model(x, tapers, weights, sfreq, n_bins, defect=None):
    """fp32 model of psd_kernel.  defect: "nyq" (the Nyquist bin of an even L doubled), "last" (the last bin of an odd L not doubled),
    "mean" (the de-mean skipped), "w" (the weights used unsquared)"""
    x, tp, w = np.asarray(x, f32), np.asarray(tapers, f32), np.asarray(weights, f32)
    B, L = x.shape
    K = tp.shape[0]
    xs = x if defect == "mean" else x - (x.sum(-1, dtype=f32, keepdims=True) / f32(L))
    v = (xs[:, None, :] * tp[None]).reshape(B * K, L)
    idx = (np.arange(L, dtype=np.int64)[:, None] * np.arange(n_bins, dtype=np.int64)[None]) % L
    ang = -2 * np.pi * np.arange(L, dtype=f64) / L
    ct, st = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
    re, im = v @ ct[idx], v @ st[idx]
    P = (re * re + im * im).reshape(B, K, n_bins)
    w2 = w if defect == "w" else w * w
    acc = (w2[None, :, None] * P).sum(1, dtype=f32)
    inv_norm = f32(1.0 / (float(w2.astype(f64).sum()) * float(sfreq)))
    fac = np.full(n_bins, 2.0, f32); fac[0] = 1.0
    if L % 2 == 0 and n_bins == L // 2 + 1 and defect != "nyq":
        fac[-1] = 1.0
    if L % 2 == 1 and defect == "last":
        fac[-1] = 1.0
    out = acc * inv_norm * fac
    assert out.dtype == f32
    return out


def psd_case(L, K, B=3):
    """(x (B, L), tapers (K, L), weights (K,), n_bins = the whole one-sided spectrum).  Window 0: unit noise; window 1: the same kind with a
    mean of 100 sigma; window 2: a pure sinusoid (at a bin centre near L / 5 when there is one).  Tapers: scipy's DPSS as the wrapper builds
    them when that yields K of them (L = 3000, 4096: half-bandwidth 4, the 7 low-bias tapers), otherwise orthonormal columns from a QR
    factorisation, with weights in [0.5, 1]."""
    rng = _rng(4, L, K)
    tapers = weights = None
    if K == 7:
        from scipy.signal.windows import dpss
        tp, ratios = dpss(L, 4.0, 8, sym=False, norm=2, return_ratios=True)
        keep = ratios > 0.9
        if int(keep.sum()) == K:
            tapers, weights = np.ascontiguousarray(tp[keep], f32), np.sqrt(ratios[keep]).astype(f32)
    if tapers is None:
        q, _ = np.linalg.qr(rng.standard_normal((L, K)))
        tapers, weights = np.ascontiguousarray(q.T, f32), rng.uniform(0.5, 1.0, K).astype(f32)
    x = rng.standard_normal((B, L))
    x[1] += 100.0
    kk = max(1, L // 5) if L > 2 else 1
    x[2] = np.sin(2 * np.pi * kk * np.arange(L) / L + 0.3)
    return x.astype(f32), tapers, weights, L // 2 + 1
