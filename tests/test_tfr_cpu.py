"""CPU: everything of the time-frequency layer that needs no device -- eegldm_stft_num_frames at its edges, every refusal of the two exports
(code and message, before any device call) and of the Python layer (ValueError), the float64 reference of tests/tfr_reference.py against
scipy.signal.spectrogram and Parseval, the analytic filter design, the statistics that take tables as input against their definitions and
scipy.stats, the planted-coupling experiment in float64, and the header."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tfr_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1


# ------------------------------------------------------------------------------------------------ the exports, without a device
def test_num_frames_rule_at_the_edges():
    from eegldm._lib import lib
    nf = lib.eegldm_stft_num_frames
    for n_win, hop in ((200, 50), (64, 64), (7, 3), (1, 1), (256, 300)):
        for L, want in ((n_win - 1, 0), (n_win, 1), (n_win + hop - 1, 1), (n_win + hop, 2), (n_win + 5 * hop + hop // 2, 6)):
            assert nf(L, n_win, hop, 0) == want == R.num_frames(L, n_win, hop, 0), (L, n_win, hop)
        for L in (1, 2, hop, hop + 1, 2 * hop, 2 * hop + 1, 3000):
            assert nf(L, n_win, hop, 1) == (L - 1) // hop + 1 == R.num_frames(L, n_win, hop, 1), (L, n_win, hop)
    assert nf(1, 200, 50, 1) == 1 and nf(0, 200, 50, 1) == 0 and nf(0, 200, 50, 0) == 0
    assert nf(1 << 24, 200, 1, 1) == 1 << 24 and nf((1 << 33) + 7, 4096, 1, 0) == (1 << 33) + 7 - 4096 + 1          # a long, not an int
    for bad in ((-1, 200, 50, 1), (100, 0, 50, 1), (100, 200, 0, 0), (100, 200, 50, 2), (100, 200, 50, -1)):
        assert nf(*bad) == -1 == R.num_frames(*bad)


def _raw_stft(**kw):
    """The export with placeholder pointers: a refusal must come before anything is dereferenced."""
    from eegldm._lib import lib
    a = dict(ctx=C.c_void_p(64), x=C.c_void_p(64), ldx=3000, B=2, L=3000, tapers=C.c_void_p(64), w2=(C.c_float * 8)(*([1.0] * 8)), K=3, n_win=200,
             n_fft=256, hop=50, centre=1, edge=1, detrend=1, onesided=1, scale=1.0, k0=0, k1=129, power=C.c_void_p(64),
             bands_host=(C.c_int * 32)(*([0, 1] * 16)), NB=2, bands=C.c_void_p(64))
    a.update(kw)
    rc = lib.eegldm_stft_power(a["ctx"], a["x"], a["ldx"], a["B"], a["L"], a["tapers"], a["w2"], a["K"], a["n_win"], a["n_fft"], a["hop"], a["centre"],
                               a["edge"], a["detrend"], a["onesided"], a["scale"], a["k0"], a["k1"], a["power"], a["bands_host"], a["NB"], a["bands"])
    return rc, lib.eegldm_last_error().decode()


def test_stft_export_refuses_before_the_device():
    bad_band = lambda lo, hi: (C.c_int * 32)(*([0, 1, lo, hi] + [0, 1] * 14))
    cases = [
        (dict(ctx=None), "null argument"), (dict(x=None), "null argument"), (dict(tapers=None), "null argument"), (dict(w2=None), "null argument"),
        (dict(power=None, bands=None), "both outputs are NULL"),
        (dict(n_fft=0), "not one of"), (dict(n_fft=32), "not one of"), (dict(n_fft=192), "not one of"), (dict(n_fft=8192), "not one of"), (dict(n_fft=255), "not one of"),
        (dict(n_win=0), "n_win"), (dict(n_win=257), "n_win"), (dict(hop=0), "hop"), (dict(hop=-3), "hop"),
        (dict(K=0), "K 0"), (dict(K=9), "K 9"),
        (dict(centre=2), "centre"), (dict(edge=2), "edge"), (dict(detrend=2), "detrend"), (dict(onesided=-1), "onesided"),
        (dict(B=-1), "out of range"), (dict(L=-1, ldx=0), "out of range"),
        (dict(ldx=2999), "row stride"),
        (dict(w2=(C.c_float * 8)(1.0, -1.0, 1.0)), "w2\\[1\\]"), (dict(w2=(C.c_float * 8)(1.0, 1.0, float("nan"))), "w2\\[2\\]"),
        (dict(k0=-1), "bin range"), (dict(k0=5, k1=5), "bin range"), (dict(k1=130), "bin range"), (dict(k0=7, k1=3), "bin range"),
        (dict(bands_host=None), "without bin ranges"), (dict(NB=0), "NB 0"), (dict(NB=17), "NB 17"),
        (dict(bands_host=bad_band(-1, 4)), "band 1"), (dict(bands_host=bad_band(4, 4)), "band 1"), (dict(bands_host=bad_band(100, 130)), "band 1"),
        (dict(L=100, ldx=100), "reflect needs"),                                                      # h = 100 > L - 1 = 99
        (dict(x=C.c_void_p(66)), "4-byte aligned"), (dict(power=C.c_void_p(65)), "4-byte aligned"), (dict(bands=C.c_void_p(67)), "4-byte aligned"),
        (dict(tapers=C.c_void_p(62)), "4-byte aligned"),
    ]
    import re
    for kw, msg in cases:
        rc, err = _raw_stft(**kw)
        assert rc == ERR_INVALID and "eegldm_stft_power" in err and re.search(msg, err), (kw, rc, err)
    # what a refusal is not: the ignored arguments of an output that is not asked for, and the two no-ops (no device call either)
    assert _raw_stft(power=None, k0=-5, k1=9999, B=0)[0] == 0
    assert _raw_stft(bands=None, NB=99, bands_host=None, B=0)[0] == 0
    assert _raw_stft(L=199, ldx=199, centre=0)[0] == 0                                               # F == 0
    assert _raw_stft(L=0, ldx=0)[0] == 0
    assert _raw_stft(L=100, ldx=100, edge=0, B=0)[0] == 0 and _raw_stft(L=100, ldx=100, centre=0, B=0)[0] == 0      # no reflection asked for


def test_pac_export_refuses_before_the_device():
    from eegldm._lib import lib
    p = C.c_void_p(64)

    def call(ctx=p, pr=p, ldr=100, pi=p, ldi=100, amp=p, lda=100, B=4, L=100, iv=p, NI=3, out=p):
        return lib.eegldm_pac_intervals(ctx, pr, ldr, pi, ldi, amp, lda, B, L, iv, NI, out), lib.eegldm_last_error().decode()

    for kw, msg in ((dict(ctx=None), "null"), (dict(pr=None), "null"), (dict(pi=None), "null"), (dict(amp=None), "null"), (dict(out=None), "null"),
                    (dict(B=-1), "out of range"), (dict(L=0), "out of range"), (dict(NI=-1), "NI"), (dict(iv=None, NI=3), "NI == B"),
                    (dict(ldr=99), "row strides"), (dict(ldi=99), "row strides"), (dict(lda=99), "row strides"),
                    (dict(pr=C.c_void_p(66)), "4-byte"), (dict(iv=C.c_void_p(65)), "4-byte"), (dict(out=C.c_void_p(68)), "8-byte")):
        rc, err = call(**kw)
        assert rc == ERR_INVALID and "eegldm_pac_intervals" in err and msg in err, (kw, rc, err)
    assert call(NI=0)[0] == 0 and call(iv=None, B=0, NI=0)[0] == 0


def test_python_layer_refuses_with_value_errors():
    """Without a GPU any touch of the device raises RuntimeError: a ValueError proves the refusal came first."""
    from eegldm import metrics as M
    x = torch.zeros(3, 3000)
    tp = np.ones((3, 200), np.float32)
    for bad in (torch.zeros(3000), torch.zeros(2, 2, 3000)):
        with pytest.raises(ValueError, match=r"\(N, L\) or \(N, 1, L\)"):
            M.stft_power(bad, tp)
        with pytest.raises(ValueError, match=r"\(N, L\) or \(N, 1, L\)"):
            M.spectrogram(bad)
    for kw, msg in ((dict(tapers=np.ones((9, 200))), "tapers"), (dict(tapers=np.ones((1, 2, 3))), "tapers"), (dict(tapers=np.full((1, 8), np.nan)), "non-finite"),
                    (dict(n_fft=200), "n_fft must be"), (dict(n_fft=128), "exceeds"), (dict(tapers=np.ones(5000)), "1..4096"), (dict(hop=0), "hop"), (dict(hop=2.5), "hop"),
                    (dict(edge="wrap"), "edge must be"), (dict(weights=[1.0, 2.0]), "weights"), (dict(weights=[1.0, np.inf, 1.0]), "weights"),
                    (dict(weights=[1.0, 1e30, 1.0]), "weights"), (dict(scale=np.nan), "scale"), (dict(scale=1e39), "scale"),
                    (dict(bins=(0, 130)), "bins"), (dict(bins=(4, 4)), "bins"), (dict(bins=(-1, 4)), "bins"), (dict(bins=(0.5, 4)), "integers"),
                    (dict(bands=[(0, 130)]), "bands"), (dict(bands=[(3, 3)]), "bands"), (dict(bands=[]), "1..16 bands"), (dict(bands=[(0, 1)] * 17), "1..16 bands"),
                    (dict(bins=False), "nothing to compute")):
        a = dict(x=x, tapers=tp)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            M.stft_power(**a)
    with pytest.raises(ValueError, match="reflect needs"):
        M.stft_power(torch.zeros(2, 100), tp)
    for kw, msg in ((dict(sfreq=0.0), "positive"), (dict(win_s=0.001), "shorter than a sample"), (dict(step_s=0.001), "shorter than a sample"),
                    (dict(win_s=50.0), "1..4096"), (dict(window="kaiser"), "window must be"), (dict(window="hann", n_tapers=2), "one taper"),
                    (dict(n_tapers=9), "tapers"), (dict(n_tapers=0), "tapers"), (dict(fmin=60.0), "no bin"), (dict(bands={"x": (3.0, 3.1)}), "holds no bin"),
                    (dict(bands={str(i): (1.0, 4.0) for i in range(17)}), "1..16 bands")):
        with pytest.raises(ValueError, match=msg):
            M.spectrogram(x, **kw)
    for bad in (np.zeros((3, 4)), np.zeros(5)):
        with pytest.raises(ValueError, match=r"\(B, F, NB\)"):
            M.band_course_stats(bad)
    for lo, hi in ((1.25, 0.4), (0.4, 0.4), (-0.1, 1.0), (11.0, 50.0), (None, 4.0)):
        with pytest.raises(ValueError, match="Hz"):
            M.fir_design_analytic(100.0, lo, hi, 0.6)
        with pytest.raises(ValueError, match="Hz"):
            M.analytic_band(x, lo, hi)
    with pytest.raises(ValueError, match="at most 2049"):
        M.analytic_band(x, 0.5, 1.25, trans_hz=0.1)
    with pytest.raises(ValueError, match="reflect needs"):
        M.analytic_band(torch.zeros(2, 200), 0.4, 1.25, trans_hz=0.6)
    z = torch.zeros(2, 50)
    with pytest.raises(ValueError, match="shapes differ"):
        M.phase_amplitude_coupling(z, z, torch.zeros(2, 51))
    for iv in (np.zeros((2, 2), np.int32), np.zeros((2, 3)), np.zeros(3, np.int32), np.array([[0, 0, 1 << 40]])):
        with pytest.raises(ValueError, match="intervals"):
            M.phase_amplitude_coupling(z, z, z, iv)
    table = {"window": np.array([0, 5]), "argmax": np.array([10, 20])}
    with pytest.raises(ValueError, match="does not belong"):
        M.spindle_so_coupling(x, table)
    with pytest.raises(ValueError, match="bands must be"):
        M.spindle_so_coupling(x, table, so_band=(0.5,))
    with pytest.raises(ValueError, match="non-negative"):
        M.spindle_so_coupling(x, table, half_s=-1.0)


# ------------------------------------------------------------------------------------------------ the float64 reference
def test_fft_level_eta_is_below_eight_u():
    assert R.fft_level_eta() < 8.0 * R.U
    for n in R.NFFT:
        t = np.log2(n)
        assert t * R.fft_level_eta() / (1.0 - t * R.fft_level_eta()) + 2.0 * R.U + R.U ** 2 < (8.0 * t + 8.0) * R.U == R.fft_constant(n) * R.U


@pytest.mark.parametrize("n_win,hop,n_fft", [(200, 50, 256), (64, 64, 64), (255, 7, 1024)])
def test_reference_equals_scipy_spectrogram(n_win, hop, n_fft):
    from scipy.signal import get_window, spectrogram
    rng = np.random.default_rng(n_win)
    sfreq = 100.0
    x = (rng.standard_normal((3, 2000)) + 5.0).astype(np.float32)
    win = get_window("hann", n_win)
    _f, _t, S = spectrogram(x.astype(np.float64), fs=sfreq, window=win, nperseg=n_win, noverlap=n_win - hop, nfft=n_fft, detrend="constant",
                            scaling="density", mode="psd")
    # the reference takes fp32 tapers: hand it the window as the float64 it would be, through a float64-exact route
    fr = R.frames64(x, n_win, hop, 0, 0)
    v = win * (fr - fr.mean(axis=2, keepdims=True))
    P = np.abs(np.fft.rfft(v, n_fft, axis=-1)) ** 2 * R._ck(n_fft, 1) / (sfreq * np.sum(win * win))
    assert S.shape == (3, n_fft // 2 + 1, P.shape[1])
    assert np.max(np.abs(P - S.transpose(0, 2, 1))) <= 1e-10 * np.max(np.abs(S))
    # and stft64 itself, with the window rounded to fp32 on both sides
    w32 = win.astype(np.float32)
    _f, _t, S32 = spectrogram(x.astype(np.float64), fs=sfreq, window=w32.astype(np.float64), nperseg=n_win, noverlap=n_win - hop, nfft=n_fft,
                              detrend="constant", scaling="density", mode="psd")
    scale = np.float32(1.0 / (sfreq * np.sum(w32.astype(np.float64) ** 2)))
    P32 = R.stft64(x, w32[None], [1.0], n_fft, hop, 0, 0, 1, scale, 1)
    ratio = float(scale) * sfreq * np.sum(w32.astype(np.float64) ** 2)                       # the fp32 rounding of scale, taken out exactly
    assert np.max(np.abs(P32 / ratio - S32.transpose(0, 2, 1))) <= 1e-10 * np.max(np.abs(S32))


def test_reference_parseval():
    """sum_k P[k] df = the tapered frame's mean power / sfreq x the taper energy normalisation: with scale = 1 / (sfreq sum taper^2) and a
    one-sided spectrum, sum_k P df = sum_n v^2 / sum_n taper^2 (per-sample power of the tapered frame over the taper's energy)."""
    rng = np.random.default_rng(1)
    sfreq = 100.0
    for n_win, n_fft, K in ((200, 256, 3), (64, 64, 1), (100, 4096, 2)):
        tp = rng.standard_normal((K, n_win)).astype(np.float32)
        w2 = rng.uniform(0.5, 1.5, K).astype(np.float32)
        x = rng.standard_normal((2, 1000)).astype(np.float32)
        P = R.stft64(x, tp, w2, n_fft, 50, 1, 1, 1, 1.0, 1)
        fr = R.frames64(x, n_win, 50, 1, 1)
        v = tp.astype(np.float64)[:, None, None, :] * (fr - fr.mean(axis=2, keepdims=True))[None]
        want = n_fft * np.einsum("t,tbf->bf", w2.astype(np.float64), np.sum(v * v, axis=-1))          # sum over the full circle = n_fft sum_n v^2
        assert np.max(np.abs(P.sum(axis=2) - want)) <= 1e-12 * np.max(want)
        df = sfreq / n_fft
        scale = 1.0 / (sfreq * float(np.sum(tp[0].astype(np.float64) ** 2)))
        P1 = R.stft64(x, tp[:1], [1.0], n_fft, 50, 1, 1, 1, 1.0, 1) * scale                           # scale applied in float64
        mean_power = np.sum(v[0] * v[0], axis=-1) / np.sum(tp[0].astype(np.float64) ** 2)
        assert np.max(np.abs(P1.sum(axis=2) * df - mean_power)) <= 1e-12 * np.max(mean_power)


def test_frame_sources_and_poisoned_frames():
    src = R.frame_sources(10, 4, 3, 1, 1)
    assert src.shape == (4, 4) and src[0].tolist() == [2, 1, 0, 1] and src[3].tolist() == [7, 8, 9, 8]
    assert R.frame_sources(10, 4, 3, 1, 0)[0].tolist() == [-1, -1, 0, 1] and R.frame_sources(10, 4, 3, 0, 1)[2].tolist() == [6, 7, 8, 9]
    assert R.poisoned_frames(10, 4, 3, 1, 1, 0).tolist() == [True, False, False, False]
    assert R.poisoned_frames(10, 4, 3, 1, 1, 7).tolist() == [False, False, True, True]
    assert R.poisoned_frames(10, 4, 3, 1, 0, 9).tolist() == [False, False, False, True]
    assert np.array_equal(R.fold_bands32(np.ones((1, 2, 5), np.float32), [(0, 5), (2, 3)]), np.array([[[5, 1], [5, 1]]], np.float32))


# ------------------------------------------------------------------------------------------------ the analytic filter
@pytest.mark.parametrize("lo,hi,trans", [(0.4, 1.25, 0.6), (11.0, 16.0, 2.0), (0.5, 1.25, 0.5)])
def test_fir_design_analytic(lo, hi, trans):
    from eegldm import metrics as M
    sfreq = 100.0
    re, im = M.fir_design_analytic(sfreq, lo, hi, trans)
    assert re.dtype == np.float64 and re.size == im.size == M.fir_length(sfreq, trans) and re.size % 2 == 1
    assert np.array_equal(re, re[::-1]) or np.max(np.abs(re - re[::-1])) <= 1e-15 * np.max(np.abs(re))
    assert np.max(np.abs(im + im[::-1])) <= 1e-15 * np.max(np.abs(im)) and im[(im.size - 1) // 2] == 0.0
    m = np.arange(re.size) - (re.size - 1) / 2
    resp = lambda f: np.sum((re + 1j * im) * np.exp(2j * np.pi * f / sfreq * m))          # y / e^{i w n} under y[n] = sum_m g[m] x[n + m]
    fc = 0.5 * (lo + hi)
    # a real cosine at the band centre, (e^{+} + e^{-}) / 2, comes out as e^{+i w0 n}: unit gain (its mirror adds the image, > 50 dB down)
    assert abs(resp(fc) / 2.0 - 1.0) <= 1e-12
    floor = 10.0 ** (-50.0 / 20.0)
    half = 0.5 * (hi - lo)
    freqs = np.linspace(-50.0, 50.0, 4001)
    gain = np.abs(np.array([resp(f) for f in freqs])) / 2.0
    stop = np.abs(freqs - fc) >= half + 0.5 * trans
    assert np.all(freqs[freqs <= 0] - fc <= -(half + 0.5 * trans)) and gain[stop].max() < floor, gain[stop].max()
    assert abs(resp(-fc)) / 2.0 < floor
    inside = np.abs(freqs - fc) <= half - 0.5 * trans
    if inside.any():
        assert np.all(np.abs(gain[inside] - 1.0) < 0.01)
    # the real part alone is the band-pass `fir_design` would give at the half-amplitude points, up to its own normalisation
    if lo - 0.5 * trans > 0:
        assert np.max(np.abs(re / np.sum(re * np.cos(2 * np.pi * fc / sfreq * m)) - M.fir_design(sfreq, lo, hi, trans))) < 1e-12


# ------------------------------------------------------------------------------------------------ statistics from tables
def test_pac_from_out_and_circular_statistics():
    from eegldm import metrics as M
    from scipy import stats
    rng = np.random.default_rng(3)
    out = np.array([[10, 5.0, 3.0, 4.0], [-1, 0, 0, 0], [0, 0, 0, 0], [4, 2.0, -2.0, 0.0], [3, 0.0, 0.0, 0.0]])
    r = M.pac_from_out(out)
    assert r["n"].tolist() == [10, -1, 0, 4, 3] and r["n"].dtype == np.int64
    assert abs(r["mvl"][0] - 1.0) <= 1e-12 and abs(r["phase"][0] - np.arctan2(4.0, 3.0)) <= 1e-12
    assert abs(r["mvl"][3] - 1.0) <= 1e-12 and abs(r["phase"][3] - np.pi) <= 1e-12
    assert np.all(np.isnan(r["mvl"][[1, 2, 4]])) and np.all(np.isnan(r["phase"][[1, 2, 4]]))
    # the reference of the sums against a direct restatement
    pr, pi, am = (rng.standard_normal((3, 70)).astype(np.float32) for _ in range(3))
    am = np.abs(am); pr[1, 5] = np.nan; am[1, 6] = np.inf; pr[2, 7] = 0.0; pi[2, 7] = 0.0
    o = R.pac64(pr, pi, am, [(0, 0, 70), (1, 0, 70), (2, 3, 10), (3, 0, 1), (0, 69, 2), (0, -1, 5), (0, 0, 0)])
    assert o[:, 0].tolist() == [70, 68, 9, -1, -1, -1, -1]
    ph = np.arctan2(pi[0].astype(np.float64), pr[0].astype(np.float64))
    assert abs(o[0, 2] - np.sum(am[0].astype(np.float64) * np.cos(ph))) <= 1e-12 * o[0, 1] and abs(o[0, 3] - np.sum(am[0].astype(np.float64) * np.sin(ph))) <= 1e-12 * o[0, 1]
    for kappa in (0.0, 0.5, 4.0):
        a = rng.vonmises(1.0, kappa, 200) if kappa else rng.uniform(-np.pi, np.pi, 200)
        s = M.circular_summary(np.concatenate([a, [np.nan]]))
        ds = stats.directional_stats(np.stack([np.cos(a), np.sin(a)], axis=1))
        assert s["n"] == 200 and abs(s["R"] - ds.mean_resultant_length) <= 1e-12
        assert M.circular_distance(s["mean"], stats.circmean(a, high=np.pi, low=-np.pi)) <= 1e-12
        assert abs(s["z"] - 200 * s["R"] ** 2) <= 1e-12 * max(s["z"], 1.0) and 0.0 <= s["p"] <= 1.0
        z = s["z"]
        want = np.exp(-z) * (1 + (2 * z - z * z) / 800.0 - (24 * z - 132 * z ** 2 + 76 * z ** 3 - 9 * z ** 4) / (288 * 200.0 ** 2))
        assert abs(s["p"] - min(max(want, 0.0), 1.0)) <= 1e-12
    assert M.circular_summary(rng.vonmises(0.0, 4.0, 100))["p"] < 1e-6 and M.circular_summary(rng.uniform(-np.pi, np.pi, 5000))["p"] > 1e-3
    assert M.circular_summary([])["n"] == 0 and M.circular_summary([np.nan])["mean"] is None
    assert abs(M.circular_distance(3.0, -3.0) - (2 * np.pi - 6.0)) <= 1e-12 and M.circular_distance(None, 1.0) is None


def test_band_course_stats_and_comparisons():
    from eegldm import metrics as M
    rng = np.random.default_rng(4)
    p = rng.lognormal(0.0, 0.7, (6, 40, 3))
    s = M.band_course_stats(torch.from_numpy(p))
    for b in range(6):
        for j in range(3):
            v = p[b, :, j]
            y = np.log(v) - np.log(v).mean()
            assert abs(s["mean"][b, j] - v.mean()) <= 1e-12 * v.mean() and abs(s["cv"][b, j] - v.std() / v.mean()) <= 1e-12
            assert abs(s["lag1"][b, j] - np.sum(y[:-1] * y[1:]) / np.sum(y * y)) <= 1e-12
    # a steady course and a bursting one with the same mean: the mean cannot tell them apart, cv and lag1 can
    t = np.arange(60)
    steady = np.full(60, 2.0) * (1.0 + 0.01 * np.sin(t))
    burst = np.where((t // 10) % 2 == 0, 3.8, 0.2)
    two = M.band_course_stats(np.stack([steady, burst * steady.mean() / burst.mean()])[:, :, None])
    assert abs(two["mean"][0, 0] - two["mean"][1, 0]) <= 1e-12 and two["cv"][1, 0] > 20 * two["cv"][0, 0] and two["lag1"][1, 0] > 0.7
    one = M.band_course_stats(np.ones((2, 1, 2)))
    assert np.all(one["mean"] == 1.0) and np.all(np.isnan(one["lag1"]))
    assert np.all(np.isnan(M.band_course_stats(np.ones((2, 5, 1)))["lag1"])) and np.all(np.isnan(M.band_course_stats(np.zeros((1, 5, 1)))["cv"]))
    assert M.band_course_stats(np.zeros((2, 0, 3)))["mean"].shape == (2, 3)
    a, c = M.band_course_stats(p[:3]), M.band_course_stats(p[3:] * 2.0)
    cmp_ = M.compare_band_courses(a, c, ["d", "t", "s"])
    assert sorted(cmp_) == ["d", "s", "t"] and sorted(cmp_["d"]) == ["cv", "lag1", "mean"]
    assert cmp_["d"]["mean"]["ks"] == M.ks_statistic(a["mean"][:, 0], c["mean"][:, 0]) and cmp_["s"]["cv"]["n_real"] == 3
    names, ranges = M.band_bin_ranges(M.BANDS, 100.0, 256)
    df = 100.0 / 256
    assert names == list(M.BANDS)
    for (lo, hi), (k_lo, k_hi) in zip(M.BANDS.values(), ranges):
        assert (k_lo - 1) * df < lo <= k_lo * df and (k_hi - 1) * df < hi <= k_hi * df
    tp, w = M.spectrogram_tapers(200)
    assert tp.shape == (3, 200) and np.all(w == 1.0) and np.max(np.abs(np.sum(tp * tp, axis=1) - 1.0)) <= 1e-12
    assert np.max(np.abs(tp @ tp.T - np.eye(3))) < 1e-3                                                  # DPSS tapers: orthonormal (the periodic form nearly so)
    hp, _w = M.spectrogram_tapers(200, "hann")
    from scipy.signal import get_window
    assert hp.shape == (1, 200) and np.max(np.abs(hp[0] - get_window("hann", 200) / np.linalg.norm(get_window("hann", 200)))) <= 1e-14
    assert M.stft_n_fft(200) == 256 and M.stft_n_fft(64) == 64 and M.stft_n_fft(1) == 64 and M.stft_n_fft(4096) == 4096
    real = {"n_events": 2, "n_dropped": 1, "mvl": np.array([0.5, 0.7]), "peak_phase_stats": M.circular_summary([0.1, 0.2]),
            "preferred_phase_stats": M.circular_summary([0.0, 0.1])}
    fake = {"n_events": 0, "n_dropped": 0, "mvl": np.zeros(0), "peak_phase_stats": M.circular_summary([]), "preferred_phase_stats": M.circular_summary([])}
    cc = M.compare_coupling(real, fake)
    assert cc["peak_phase_distance"] is None and cc["mvl"]["ks"] is None and cc["real"]["n_dropped"] == 1
    cc = M.compare_coupling(real, real)
    assert cc["peak_phase_distance"] == 0.0 and cc["mvl"]["ks"] == 0.0 and cc["mvl"]["wasserstein"] == 0.0


# ------------------------------------------------------------------------------------------------ planted coupling in float64
def planted_coupling64(seed, theta):
    """(peak phases, preferred phases) of the 48 planted bursts through the float64 filters."""
    from eegldm import metrics as M
    x, centres = R.planted_windows(seed, theta)
    so = [R.fir_reflect64(x, t) for t in M.fir_design_analytic(100.0, 0.4, 1.25, 0.6)]
    sg = [R.fir_reflect64(x, t) for t in M.fir_design_analytic(100.0, 11.0, 16.0, 2.0)]
    amp = np.hypot(sg[0], sg[1])
    phase = np.arctan2(so[1], so[0])
    peak, pref = [], []
    for i in range(x.shape[0]):
        for c in centres[i]:
            sl = slice(c - 50, c + 51)
            peak.append(phase[i, c])
            pref.append(np.arctan2(np.sum(amp[i, sl] * np.sin(phase[i, sl])), np.sum(amp[i, sl] * np.cos(phase[i, sl]))))
    return np.array(peak), np.array(pref)


@pytest.mark.parametrize("seed", range(5))
def test_planted_coupling_float64(seed):
    from eegldm import metrics as M
    assert M.fir_length(100.0, 0.6) == 551
    _x, centres = R.planted_windows(seed, 0.0)
    for j in range(3):
        assert np.all((centres[:, j] >= 100 * (6 + 6 * j)) & (centres[:, j] < 100 * (6 + 6 * j + 1.25) + 1))
    for theta in (0.0, 2.0):
        for name, ph in zip(("peak", "preferred"), planted_coupling64(seed, theta)):
            mean, r = R.circ_mean_r(ph)
            assert ph.size == 48 and R.circ_dist(mean, theta) <= 0.1 and r >= 0.95, (seed, theta, name, mean, r)
    for name, ph in zip(("peak", "preferred"), planted_coupling64(seed, None)):
        assert R.circ_mean_r(ph)[1] <= 0.5, (seed, name, R.circ_mean_r(ph))


# ------------------------------------------------------------------------------------------------ header and documents
def test_header_and_documents_name_the_exports():
    src = open(os.path.join(ROOT, "include", "eegldm.h")).read()
    for name in ("eegldm_stft_num_frames", "eegldm_stft_power", "eegldm_pac_intervals"):
        assert src.count(name) >= 2, name
    assert "#define EEGLDM_ABI_VERSION 8" in src
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "eegldm_stft_power" in readme and "have not been validated" in readme and "not evidence of realism" in readme
    from eegldm.entry import time_frequency as T
    assert "not been validated" in T.CAVEAT and "not evidence of realism" in T.CAVEAT
