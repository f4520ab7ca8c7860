"""float64 numpy references of the two primitives of csrc/tfr.hip and the error bounds they are held to.  Shared by tests/test_tfr_cpu.py and
tests/test_gpu_tfr.py.  Every reference evaluates the definition in float64 FROM THE fp32 INPUTS (x, tapers, w2 and scale are the fp32 values
handed to the call).

eegldm_stft_power.

    frames   centre 0: s_f = f hop, F = (L - n_win) / hop + 1 (0 when L < n_win);   centre 1: s_f = f hop - n_win / 2, F = (L - 1) / hop + 1
             xe: zero outside [0, L) (edge 0) or xe[-i] = x[i], xe[L-1+i] = x[L-1-i] (edge 1)
    value    v_t[n] = taper_t[n] (xe[s_f + n] - m), m = mean of the frame's n_win samples (detrend) or 0;  X_t = DFT_n_fft(v_t, zero-padded)
             P[k] = scale c_k sum_t w2[t] |X_t[k]|^2,   c_k = 2 when onesided and 0 < k < n_fft / 2, else 1
             bands[j] = sum_{k in [lo_j, hi_j)} P[k]

Error bound (`stft_error_bound`), u = 2^-24, g(n) = n u / (1 - n u), TINY = 2^-126 per sum for results that leave the normal range, every term in
float64 on the reference's values.  The kernel's operations, in order:

 1. m^ : a sum of the n_win fp32 samples (lane chains, an xor butterfly, the group's waves in order: every sample passes through fewer than
    n_win additions) and one correctly rounded division: |m^ - m| <= g(n_win) mean|xe| =: dm               (0 without detrend)
 2. v^[n] = fl(taper fl(xe - m^)): |v^ - v| <= |taper| ((2 u + u^2) |xe - m| + (1 + u)^2 dm).  Through the exact DFT that moves a bin by at
    most sum_n |v^ - v| <= (2 u + u^2) sqrt(n_fft) ||v||_2 + (1 + u)^2 dm sum|taper|                        (Cauchy-Schwarz, n_win <= n_fft)
 3. the FFT: radix-2 decimation in frequency, t = log2 n_fft levels, roots of unity from sincospif (SINCOSPI_ULPS = 1 ulp in HIP's table of
    device functions; an ulp is at most 2 u of the value, so |w^ - w| <= mu = 2 u SINCOSPI_ULPS).  Higham, Accuracy and Stability of
    Numerical Algorithms, theorem 24.2: ||X^ - X||_2 <= t eta / (1 - t eta) ||X||_2 with eta = mu + g(4) (sqrt 2 + mu) per level and
    ||X||_2 = sqrt(n_fft) ||v^||_2; a bin's error is at most the vector's.  eta = 7.66 u < 8 u (`fft_level_eta`, asserted in the CPU tests).
    Together with 2.:  E_X = C u sqrt(n_fft) ||v||_2 + 1.001 dm sum|taper| + n_fft TINY,   C = 8 log2(n_fft) + 8
    (8 t covers t eta / (1 - t eta) with 0.34 t to spare; the + 8 covers the 2 u of step 2, the second-order terms and the roundings of the
    magnitude and the weights below where they are folded into it; 1.001 covers (1 + u)^2 (1 + t eta sqrt(n_fft)) <= 1.0004.)
 4. p^ = fl(Xr^2 + Xi^2): two roundings on either path (fused or not):  e_p = (1 + g(2)) (2 |X| E_X + E_X^2) + g(2) |X|^2
 5. acc = sum_t fl(w2[t] p^_t), K products and K - 1 additions, then P^ = fl(fl(scale c_k) acc), scale c_k exact:
    E_P = |scale| c_k ((1 + g(K + 4)) sum_t w2[t] (2 |X_t| E_X,t + E_X,t^2) + g(K + 4) sum_t w2[t] |X_t|^2) + (K + 2) TINY
 6. bands: nb = hi - lo additions from +0 of the stored P^:  E_band = sum_k E_P[k] + g(nb) sum_k (|P[k]| + E_P[k]) + nb TINY

The bound is rigorous and loose (C is 56 to 104; a single-precision FFT sits near 1).  `yardstick_errors` holds the kernel to numpy's
complex64 rfft as well: through a K = 1, scale = 1, two-sided, undetrended call, the RMS over a frame's bins of |P_device - P_64| against the
same RMS for p_y = fl32(Yr^2 + Yi^2), Y = np.fft.rfft(fl32(taper xe)) (single precision), the magnitude taken in fp32 as the kernel takes it.

eegldm_pac_intervals.  out = (n, sum a, sum a pr / h, sum a pi / h), h = sqrt(pr^2 + pi^2), over the samples with finite a, pr, pi and h > 0.
Bound (`pac_error_bound`), v = 2^-53: a term (a pr) / h is one product, one quotient and h's three roundings and square root: relative error
below 6 v (|pr / h| <= 1); a lane's chain holds ceil(len / 64) additions and the butterfly 6 more, so with q = ceil(len / 64) + 6:
    |c^ - c|, |s^ - s| <= (6 v + q v / (1 - q v) (1 + 6 v)) sum |a|;     |sum_a^ - sum_a| <= q v / (1 - q v) sum |a|;    n is exact.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
V = 2.0 ** -53
SINCOSPI_ULPS = 1.0
NFFT = (64, 128, 256, 512, 1024, 2048, 4096)
YARDSTICK_FACTOR = 8.0


def g(n):
    return n * U / (1.0 - n * U)


def fft_level_eta():
    mu = 2.0 * U * SINCOSPI_ULPS
    return mu + g(4) * (np.sqrt(2.0) + mu)


def fft_constant(n_fft):
    """C of E_X = C u sqrt(n_fft) ||v||_2: the issue's cap, 8 log2(n_fft) + 8."""
    return 8.0 * np.log2(n_fft) + 8.0


# ---------------------------------------------------------------------------------------------------- frames
def num_frames(L, n_win, hop, centre):
    if L < 0 or n_win < 1 or hop < 1 or centre not in (0, 1):
        return -1
    if centre:
        return (L - 1) // hop + 1 if L >= 1 else 0
    return (L - n_win) // hop + 1 if L >= n_win else 0


def frame_sources(L, n_win, hop, centre, edge):
    """(F, n_win) int64: the row index every frame element comes from, -1 for a zero."""
    F = num_frames(L, n_win, hop, centre)
    pos = np.arange(F)[:, None] * hop - (n_win // 2 if centre else 0) + np.arange(n_win)[None, :]
    if centre and edge:
        assert n_win // 2 <= L - 1
        return np.where(pos < 0, -pos, np.where(pos > L - 1, 2 * (L - 1) - pos, pos))
    return np.where((pos >= 0) & (pos < L), pos, -1)


def frames64(x, n_win, hop, centre, edge):
    """(B, L) fp32 -> (B, F, n_win) float64 frames of the extended rows."""
    x = np.asarray(x, np.float32).astype(np.float64)
    src = frame_sources(x.shape[1], n_win, hop, centre, edge)
    return np.where(src[None] >= 0, x[:, np.maximum(src, 0)], 0.0)


def poisoned_frames(L, n_win, hop, centre, edge, idx):
    """(F,) bool: the frames whose support holds sample idx (reflected copies included)."""
    return np.any(frame_sources(L, n_win, hop, centre, edge) == idx, axis=1)


# ---------------------------------------------------------------------------------------------------- STFT power
def _ck(n_fft, onesided):
    c = np.ones(n_fft // 2 + 1)
    if onesided:
        c[1:n_fft // 2] = 2.0
    return c


def stft64(x, tapers, w2, n_fft, hop, centre=1, edge=1, detrend=1, scale=1.0, onesided=1, with_parts=False):
    """P (B, F, n_fft / 2 + 1) float64; with_parts also returns (absX (K, B, F, nbin), vnorm (K, B, F), dm (B, F))."""
    tp = np.asarray(tapers, np.float32).astype(np.float64).reshape(-1, np.asarray(tapers).shape[-1])
    w2 = np.asarray(w2, np.float32).astype(np.float64).reshape(-1)
    sc = float(np.float32(scale))
    fr = frames64(x, tp.shape[1], hop, centre, edge)
    with np.errstate(all="ignore"):
        m = fr.mean(axis=2, keepdims=True) if detrend else 0.0
        v = tp[:, None, None, :] * (fr - m)[None]                                      # (K, B, F, n_win)
        X = np.fft.rfft(v, n_fft, axis=-1)
        absX = np.abs(X)
        P = sc * _ck(n_fft, onesided) * np.einsum("t,tbfk->bfk", w2, absX * absX)
    if not with_parts:
        return P
    dm = g(tp.shape[1]) * np.mean(np.abs(fr), axis=2) if detrend else np.zeros(fr.shape[:2])
    return P, absX, np.sqrt(np.sum(v * v, axis=-1)), dm


def stft_error_bound(x, tapers, w2, n_fft, hop, centre=1, edge=1, detrend=1, scale=1.0, onesided=1):
    """(P, E_P): |P_device - P| <= E_P elementwise for finite inputs (steps 1 to 5 above)."""
    tp = np.asarray(tapers, np.float32).astype(np.float64).reshape(-1, np.asarray(tapers).shape[-1])
    w2 = np.asarray(w2, np.float32).astype(np.float64).reshape(-1)
    K = tp.shape[0]
    P, absX, vnorm, dm = stft64(x, tapers, w2, n_fft, hop, centre, edge, detrend, scale, onesided, with_parts=True)
    e_x = fft_constant(n_fft) * U * np.sqrt(n_fft) * vnorm + 1.001 * dm[None] * np.sum(np.abs(tp), axis=1)[:, None, None] + n_fft * TINY   # (K, B, F)
    e_x = e_x[..., None]
    first = np.einsum("t,tbfk->bfk", w2, 2.0 * absX * e_x + e_x * e_x)
    second = np.einsum("t,tbfk->bfk", w2, absX * absX)
    sc = abs(float(np.float32(scale))) * _ck(n_fft, onesided)
    return P, sc * ((1.0 + g(K + 4)) * first + g(K + 4) * second) + (K + 2) * TINY


def bands64(P, ranges):
    """(B, F, nbin) -> (B, F, NB): float64 sums over the bin ranges [lo, hi)."""
    return np.stack([P[:, :, lo:hi].sum(axis=2) for lo, hi in ranges], axis=2)


def bands_error_bound(P, E_P, ranges):
    return np.stack([E_P[:, :, lo:hi].sum(axis=2) + g(hi - lo) * (np.abs(P[:, :, lo:hi]) + E_P[:, :, lo:hi]).sum(axis=2) + (hi - lo) * TINY
                     for lo, hi in ranges], axis=2)


def fold_bands32(power32, ranges):
    """The ascending fp32 fold from +0 of a full call's stored values: what a bands call must equal bit for bit."""
    p = np.asarray(power32, np.float32)
    out = np.zeros(p.shape[:2] + (len(ranges),), np.float32)
    for j, (lo, hi) in enumerate(ranges):
        s = np.zeros(p.shape[:2], np.float32)
        with np.errstate(all="ignore"):
            for k in range(lo, hi):
                s = (s + p[:, :, k]).astype(np.float32)
        out[:, :, j] = s
    return out


def yardstick_errors(P_dev, x, taper, n_fft, hop, centre, edge):
    """(rms_device, rms_yardstick), each (B, F): RMS over the bins of |P - P_64| for the device's K = 1, scale = 1, two-sided, undetrended power
    and for numpy's single-precision rfft of the same float32 frame fl32(taper xe), magnitude in fp32."""
    tp = np.asarray(taper, np.float32).reshape(-1)
    fr = frames64(x, tp.size, hop, centre, edge).astype(np.float32)
    v32 = (fr * tp).astype(np.float32)                                               # one fp32 rounding, as in the kernel
    X64 = np.fft.rfft(v32.astype(np.float64), n_fft, axis=-1)
    P64 = X64.real ** 2 + X64.imag ** 2
    Y = np.fft.rfft(v32, n_fft, axis=-1)
    assert Y.dtype == np.complex64, "numpy's rfft of float32 no longer computes in single precision"
    p_y = (Y.real * Y.real + Y.imag * Y.imag).astype(np.float32)
    rms = lambda d: np.sqrt(np.mean(d * d, axis=-1))
    return rms(np.asarray(P_dev, np.float64) - P64), rms(p_y.astype(np.float64) - P64)


# ---------------------------------------------------------------------------------------------------- phase-amplitude sums
def pac64(pr, pi, amp, iv=None):
    """out (NI, 4) float64 by the definition; (-1, 0, 0, 0) for an interval outside its row."""
    pr, pi, amp = (np.asarray(t, np.float32).astype(np.float64) for t in (pr, pi, amp))
    B, L = pr.shape
    if iv is None:
        iv = np.stack([np.arange(B), np.zeros(B, np.int64), np.full(B, L)], axis=1)
    out = np.zeros((len(iv), 4))
    for q, (row, start, length) in enumerate(np.asarray(iv, np.int64)):
        if not (0 <= row < B and start >= 0 and length >= 1 and start + length <= L):
            out[q] = (-1.0, 0.0, 0.0, 0.0)
            continue
        a, x, y = amp[row, start:start + length], pr[row, start:start + length], pi[row, start:start + length]
        with np.errstate(all="ignore"):
            h = np.sqrt(x * x + y * y)
            ok = np.isfinite(a) & np.isfinite(x) & np.isfinite(y) & (h > 0)
        a, x, y, h = a[ok], x[ok], y[ok], h[ok]
        out[q] = (ok.sum(), a.sum(), np.sum(a * x / h), np.sum(a * y / h))
    return out


def pac_error_bound(pr, pi, amp, iv=None):
    """(NI, 4): column 0 (n) is exact, 1 the bound on sum a, 2 and 3 on the two phase sums."""
    pr, pi, amp = (np.asarray(t, np.float32).astype(np.float64) for t in (pr, pi, amp))
    B, L = pr.shape
    if iv is None:
        iv = np.stack([np.arange(B), np.zeros(B, np.int64), np.full(B, L)], axis=1)
    E = np.zeros((len(iv), 4))
    for q, (row, start, length) in enumerate(np.asarray(iv, np.int64)):
        if not (0 <= row < B and start >= 0 and length >= 1 and start + length <= L):
            continue
        a = amp[row, start:start + length]
        with np.errstate(all="ignore"):
            ok = np.isfinite(a) & np.isfinite(pr[row, start:start + length]) & np.isfinite(pi[row, start:start + length])
        sa = np.abs(a[ok]).sum()
        qn = -(-int(length) // 64) + 6
        gq = qn * V / (1.0 - qn * V)
        E[q] = (0.0, gq * sa, (6.0 * V + gq * (1.0 + 6.0 * V)) * sa, (6.0 * V + gq * (1.0 + 6.0 * V)) * sa)
    return E


# ---------------------------------------------------------------------------------------------------- planted coupling (float64)
def fir_reflect64(x, taps):
    """`eegldm_fir_same` with reflected edges in float64: y[n] = sum_k taps[k] xe[n + k - c]."""
    x = np.asarray(x, np.float64)
    t = np.asarray(taps, np.float64)
    c = (len(t) - 1) // 2
    xe = np.concatenate([x[:, 1:c + 1][:, ::-1], x, x[:, x.shape[1] - 1 - c:x.shape[1] - 1][:, ::-1]], axis=1)
    return np.stack([np.correlate(r, t, "valid") for r in xe])


def planted_windows(seed, theta, n_windows=16, length=3000, sfreq=100.0):
    """The planted-coupling recording: 0.3 N(0, 1) noise plus 2 cos(2 pi 0.8 t + phi_i) per window, and three 13-Hz bursts (Gaussian envelope,
    sd 0.25 s, amplitude 1), burst j centred at the sample in [6 + 6 j, 6 + 6 j + 1.25) s where the slow oscillation's phase equals the
    planted phase theta (None: a uniformly random phase per burst).  Returns (windows float32 (n, length), centres int64 (n, 3))."""
    rng = np.random.default_rng(seed)
    t = np.arange(length) / sfreq
    phi = rng.uniform(0.0, 2.0 * np.pi, n_windows)
    x = 0.3 * rng.standard_normal((n_windows, length)) + 2.0 * np.cos(2.0 * np.pi * 0.8 * t[None] + phi[:, None])
    centres = np.zeros((n_windows, 3), np.int64)
    for i in range(n_windows):
        for j in range(3):
            th = rng.uniform(-np.pi, np.pi) if theta is None else theta
            t0 = 6.0 + 6.0 * j
            # phase 2 pi 0.8 t + phi_i = th (mod 2 pi) at t = (th - phi_i + 2 pi k) / (2 pi 0.8): the first such t at or after t0
            k = np.ceil((2.0 * np.pi * 0.8 * t0 - th + phi[i]) / (2.0 * np.pi))
            tc = (th - phi[i] + 2.0 * np.pi * k) / (2.0 * np.pi * 0.8)
            c = int(round(tc * sfreq))
            centres[i, j] = c
            x[i] += np.exp(-0.5 * ((t - c / sfreq) / 0.25) ** 2) * np.cos(2.0 * np.pi * 13.0 * (t - c / sfreq))
    return x.astype(np.float32), centres


def circ_mean_r(a):
    a = np.asarray(a, np.float64)
    c, s = np.mean(np.cos(a)), np.mean(np.sin(a))
    return float(np.arctan2(s, c)), float(np.hypot(c, s))


def circ_dist(a, b):
    return float(abs(np.angle(np.exp(1j * (a - b)))))
