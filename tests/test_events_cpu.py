"""CPU: everything of the sleep micro-structure layer that needs no device -- the refusals, the filter design (symmetry, gain, attenuation,
scipy.signal.firwin where scipy is there), the references of tests/events_reference.py held against independent restatements, the table
algebra (event_summary, compare_events, pair_half_waves), the planted-event construction the GPU pipeline test relies on, and the header."""
import os
import re

import numpy as np
import pytest
import torch

import events_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_come_before_the_device():
    """Without a GPU any touch of the device raises RuntimeError: a ValueError proves the refusal came first."""
    from eegldm import metrics as M
    w = torch.zeros(4, 1, 3000)
    for bad in (torch.zeros(3000), torch.zeros(2, 2, 3000), torch.zeros(1, 2, 1, 3000)):
        for fn in (lambda x: M.fir_filter(x, [1.0]), lambda x: M.band_envelope(x, 11.0, 16.0), lambda x: M.detect_spindles(x, 1.0),
                   lambda x: M.detect_half_waves(x), lambda x: M.envelope_threshold(x), lambda x: M.threshold_events(x, 0.0)):
            with pytest.raises(ValueError, match=r"\(N, L\) or \(N, 1, L\)"):
                fn(bad)
    for lo, hi in ((16.0, 11.0), (11.0, 11.0), (11.0, 50.0), (11.0, 60.0), (0.0, 16.0), (-1.0, 16.0)):
        with pytest.raises(ValueError, match="Hz"):
            M.fir_design(100.0, lo, hi)
        with pytest.raises(ValueError, match="Hz"):
            M.band_envelope(w, lo, hi)
        with pytest.raises(ValueError, match="Hz"):
            M.detect_spindles(w, 1.0, band=(lo, hi))
    with pytest.raises(ValueError, match="lo .* hi|give"):
        M.fir_design(100.0)
    with pytest.raises(ValueError, match="positive"):
        M.fir_design(100.0, hi=4.0, trans_hz=0.0)
    with pytest.raises(ValueError, match="at most 2049"):                 # 3.3 * 100 / 0.16 = 2063 taps
        M.fir_design(100.0, hi=4.0, trans_hz=0.16)
    with pytest.raises(ValueError, match="at most 2049"):
        M.detect_half_waves(w, trans_hz=0.16)
    assert len(M.fir_design(100.0, hi=4.0, trans_hz=3.3 * 100 / 2049)) == 2049
    with pytest.raises(ValueError, match="odd number of taps"):
        M.fir_filter(w, np.ones(2051))
    with pytest.raises(ValueError, match="odd number of taps"):
        M.fir_filter(w, np.ones(4))
    with pytest.raises(ValueError, match="odd number of taps"):
        M.fir_filter(w, [])
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="non-finite taps"):
            M.fir_filter(w, [0.5, bad, 0.5])
    for bad in (1e39, -3.5e38):                                          # finite in float64, inf as the fp32 that is uploaded
        with pytest.raises(ValueError, match="non-finite taps"):
            M.fir_filter(w, [0.5, bad, 0.5])
    with pytest.raises(ValueError, match="edge must be"):
        M.fir_filter(w, [1.0], edge="wrap")
    for band in ((16.0, 11.0), (11.0, 50.0)):
        with pytest.raises(ValueError, match="Hz"):
            M.envelope_threshold(w, band=band)
    with pytest.raises(ValueError, match="band must be"):
        M.envelope_threshold(w, band=(11.0,))
    with pytest.raises(ValueError, match="reflect needs"):
        M.fir_filter(torch.zeros(3, 82), np.ones(165) / 165, edge="reflect")          # c = 82 > L - 1 = 81
    with pytest.raises(ValueError, match="reflect needs"):
        M.band_envelope(torch.zeros(3, 82), 11.0, 16.0)
    with pytest.raises(ValueError, match="reflect needs"):
        M.detect_spindles(torch.zeros(3, 82), 1.0)
    with pytest.raises(ValueError, match="1..4096 samples"):
        M.fir_filter(torch.zeros(2, 4097), [1.0])
    with pytest.raises(ValueError, match="1..4096 samples"):
        M.threshold_events(torch.zeros(2, 4097), 0.0)
    for e in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="max_events"):
            M.threshold_events(w, 0.0, max_events=e)
        with pytest.raises(ValueError, match="max_events"):
            M.detect_spindles(w, 1.0, max_events=e)
        with pytest.raises(ValueError, match="max_events"):
            M.detect_half_waves(w, max_events=e)
    for kw in (dict(min_len=0), dict(min_len=5, max_len=4), dict(merge_gap=-1)):
        with pytest.raises(ValueError, match="min_len"):
            M.threshold_events(w, 0.0, **kw)
    with pytest.raises(ValueError, match="aux"):
        M.threshold_events(w, 0.0, aux=torch.zeros(4, 2999))
    with pytest.raises(ValueError, match="thr must be"):
        M.threshold_events(w, np.zeros(3))
    with pytest.raises(ValueError, match="polarity"):
        M.detect_half_waves(w, polarity=0)
    with pytest.raises(ValueError, match="rms_s"):
        M.band_envelope(w, 11.0, 16.0, rms_s=0.001)
    tab = {"window": np.array([0, 2]), "duration_s": np.array([1.0, 2.0])}
    for lab in (np.zeros(2), np.zeros(4)):
        with pytest.raises(ValueError, match="labels"):
            M.event_summary(tab, 3, 30.0, labels=lab)
    with pytest.raises(ValueError, match="n_windows"):
        M.event_summary(tab, 2, 30.0)


def test_envelope_threshold_passes_the_detectors_band(monkeypatch):
    """envelope_threshold(real, factor) as the issue writes it: the band defaults to detect_spindles' (11, 16) Hz, `band=` and band_envelope's own
    keywords reach the filter.  band_envelope is replaced by a recorder, so no device is needed."""
    import inspect
    from eegldm import metrics as M
    calls = []

    def fake(windows, lo, hi, **kw):
        calls.append((tuple(windows.shape), lo, hi, kw))
        e = torch.arange(windows.numel(), dtype=torch.float32).reshape(windows.shape)
        return e, e
    monkeypatch.setattr(M, "band_envelope", fake)
    w = torch.zeros(5, 1, 3000)
    thr = M.envelope_threshold(w, factor=1.5)
    v = np.arange(15000.0)
    assert abs(thr - (v.mean() + 1.5 * v.std())) < 1e-6 * thr                         # the fake's fp32 ramp rounds above 2^24: not the point here
    assert calls == [((5, 3000), 11.0, 16.0, {})]
    assert inspect.signature(M.envelope_threshold).parameters["band"].default == inspect.signature(M.detect_spindles).parameters["band"].default
    del calls[:]
    M.envelope_threshold(w, 3.0, band=(9.0, 12.0), batch_size=2, sfreq=128.0, rms_s=0.3, trans_hz=1.0)
    assert [c[0] for c in calls] == [(2, 3000), (2, 3000), (1, 3000)] and all(c[1:] == (9.0, 12.0, {"sfreq": 128.0, "rms_s": 0.3, "trans_hz": 1.0}) for c in calls)
    del calls[:]
    M.envelope_threshold(w, lo=12.0, hi=15.0)
    assert calls == [((5, 3000), 12.0, 15.0, {})]


# ------------------------------------------------------------------------------------------------ filter design
DESIGNS = [dict(hi=18.0, trans_hz=4.0), dict(hi=4.0), dict(lo=11.0, hi=16.0), dict(lo=0.5), dict(lo=0.5, hi=4.0, trans_hz=0.5), dict(hi=4.0, trans_hz=0.3),
           dict(lo=9.0, hi=12.0, trans_hz=1.0)]


def _gain(t, f, sfreq=100.0):
    k = np.arange(len(t)) - (len(t) - 1) / 2
    return np.abs(np.sum(t[None, :] * np.exp(-2j * np.pi * np.atleast_1d(f)[:, None] * k[None, :] / sfreq), 1))


@pytest.mark.parametrize("kw", DESIGNS)
def test_fir_design(kw):
    """Odd, symmetric, the smallest odd length >= 3.3 sfreq / trans_hz, gain 1 at DC / the band centre / Nyquist to 1e-12, and more than 50 dB down
    beyond the transition bands (the Hamming window's side lobes stay below -53 dB).  The transition band is [cut-off - trans_hz / 2, cut-off +
    trans_hz / 2], ends included: the gain AT its end is the -49.5 dB of the main lobe's foot, so the stop band is sampled on a 0.05-Hz grid
    that starts one step beyond it."""
    from eegldm import metrics as M
    t = M.fir_design(100.0, **kw)
    trans = kw.get("trans_hz", 2.0)
    need = 3.3 * 100.0 / trans
    assert t.dtype == np.float64 and len(t) % 2 == 1 and need - 1e-9 <= len(t) < need + 2 and np.array_equal(t, t[::-1])
    lo, hi = kw.get("lo"), kw.get("hi")
    centre = 0.0 if lo is None else (50.0 if hi is None else 0.5 * (lo + hi))
    assert abs(_gain(t, centre)[0] - 1.0) <= 1e-12
    stop = []
    if hi is not None:
        stop.append(np.arange(hi + 0.5 * trans + 0.05, 50.0 + 1e-9, 0.05))
    if lo is not None and lo - 0.5 * trans > 0:
        stop.append(np.arange(0.0, lo - 0.5 * trans - 0.05 + 1e-9, 0.05))
    for f in stop:
        assert 20.0 * np.log10(_gain(t, f).max()) < -50.0, kw
    if lo is None:                                  # pass band of a low-pass: flat to the ripple of the window (0.02 dB)
        inside = np.arange(0.0, max(hi - 0.5 * trans, 0.0) + 1e-9, 0.05)
        assert np.all(np.abs(_gain(t, inside) - 1.0) < 5e-3)


@pytest.mark.parametrize("kw", DESIGNS)
def test_fir_design_equals_firwin(kw):
    signal = pytest.importorskip("scipy.signal")
    from eegldm import metrics as M
    t = M.fir_design(100.0, **kw)
    lo, hi = kw.get("lo"), kw.get("hi")
    cut = hi if lo is None else (lo if hi is None else [lo, hi])
    want = signal.firwin(len(t), cut, window="hamming", pass_zero=lo is None, fs=100.0)
    assert np.abs(t - want).max() <= 1e-12


def test_rms_box():
    from eegldm import metrics as M
    for rms_s, w in ((0.2, 21), (0.21, 21), (0.25, 25), (0.01, 1), (0.3, 31)):
        b = M.rms_box(rms_s, 100.0)
        assert len(b) == w and np.all(b == 1.0 / w)


# ------------------------------------------------------------------------------------------------ the references
def test_fir_reference_against_a_direct_loop():
    """fir64 (np.correlate on the extended rows) against the definition written out index by index, both edges and both modes; the support masks."""
    rng = np.random.default_rng(0)
    for L, M_, edge, mode in ((7, 5, 1, 0), (7, 13, 1, 1), (5, 9, 0, 0), (1, 3, 0, 1), (9, 1, 1, 0), (12, 7, 0, 1)):
        x = rng.standard_normal((2, L)).astype(np.float32); t = rng.standard_normal(M_).astype(np.float32)
        c = (M_ - 1) // 2
        want = np.zeros((2, L))
        for b in range(2):
            for n in range(L):
                for k in range(M_):
                    j = n + k - c
                    if edge:
                        j = -j if j < 0 else (2 * (L - 1) - j if j > L - 1 else j)
                    elif not 0 <= j < L:
                        continue
                    v = np.float32(x[b, j] * x[b, j]) if mode else x[b, j]
                    want[b, n] += float(t[k]) * float(v)
        if mode:
            want = np.sqrt(np.maximum(want, 0.0))
        assert np.abs(R.fir64(x, t, edge, mode) - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
        assert np.all(R.fir_error_bound(x, t, edge, mode) > 0)
    assert R.support_mask(10, 5, 0).tolist() == [True] * 3 + [False] * 7 and R.support_mask(10, 5, 9).tolist() == [False] * 7 + [True] * 3
    assert R.support_mask_reflect(10, 5, 1).tolist() == [True] * 4 + [False] * 6          # x[1] is also xe[-1]: output 0 sees it twice, output 3 once
    assert R.support_mask_reflect(10, 5, 0).tolist() == [True] * 3 + [False] * 7          # the end sample is not repeated


def test_closing_equals_the_sequential_merge():
    rng = np.random.default_rng(1)
    for trial in range(300):
        L = int(rng.integers(1, 200)); rate = (0.05, 0.3, 0.7)[trial % 3]; gap = int(rng.integers(0, 6))
        a = rng.random(L) < rate
        closed = R.close_mask(a, gap)
        runs = R.sequential_merge(a, gap)
        want = np.zeros(L, bool)
        for s, e, _n in runs:
            want[s:e] = True
        assert np.array_equal(closed, want)
        assert sum(r[2] for r in runs) == len(R.sequential_merge(a, -1))
        assert R.runs_of(a) == [(r[0], r[1]) for r in R.sequential_merge(a, -1)]
        # stretches that touch a row end are never filled
        if not a[0]:
            first = np.argmax(a) if a.any() else L
            assert not closed[:first].any()


def test_run_features_forms_agree():
    """The array form of the per-run features against the sample-by-sample definition, bit for bit, with NaNs, signed zeros and plateaus."""
    rng = np.random.default_rng(2)
    for trial in range(200):
        n = int(rng.integers(1, 40))
        s = rng.integers(-2, 3, n).astype(np.float32); aux = rng.integers(-2, 3, n).astype(np.float32)
        if trial % 2:
            s += rng.standard_normal(n).astype(np.float32); aux += rng.standard_normal(n).astype(np.float32)
        for arr in (s, aux):
            arr[rng.random(n) < 0.1] = np.nan
            arr[rng.random(n) < 0.1] = -0.0
        s[0] = 1.0 if np.isnan(s[0]) else s[0]                  # a run starts on an active sample
        for ax in (aux, None):
            a, b = R.run_features_loop(s, ax, 0, n), R.run_features(s, ax, 0, n)
            assert a[1] == b[1]
            for u, v in zip((a[0], a[2], a[3], a[4]), (b[0], b[2], b[3], b[4])):
                assert np.float32(u).view(np.int32) == np.float32(v).view(np.int32) or (np.isnan(u) and np.isnan(v))


def test_events_reference_hand_cases():
    s = np.array([[0, 2, 2, 0, 0, 3, 0, 0, 0, 1, 1]], np.float32)
    aux = np.array([[-1, 0, -1, 1, -1, -1, 0, 0, -1, 2, -3]], np.float32)
    c, i, f = R.threshold_events(s, [0.5], aux=aux, merge_gap=2, max_events=4)
    assert c.tolist() == [[2, 3]]
    assert i[0, 0].tolist() == [1, 5, 5, 1, 2, 0] and f[0, 0].tolist() == [3.0, 7.0, 1.0, -1.0]
    assert i[0, 1].tolist() == [9, 2, 9, 0, 1, 2] and f[0, 1].tolist() == [1.0, 2.0, 2.0, -3.0]
    assert not i[0, 2:].any()
    c, i, f = R.threshold_events(s, [0.5], merge_gap=3, drop_edge=True, max_events=1)
    assert c.tolist() == [[0, 3]] and not i.any()
    c, i, f = R.threshold_events(s, [0.5], merge_gap=1, min_len=2, max_len=2, max_events=1)
    assert c.tolist() == [[2, 3]] and i[0, 0].tolist() == [1, 2, 1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ table algebra
def test_event_summary_equals_its_definition():
    from eegldm import metrics as M
    rng = np.random.default_rng(3)
    win = np.sort(rng.integers(0, 10, 37))
    tab = {"window": win, "duration_s": rng.uniform(0.5, 3, 37), "amplitude": rng.uniform(1, 9, 37), "freq_hz": rng.uniform(11, 16, 37)}
    lab = rng.integers(0, 3, 10)
    got = M.event_summary(tab, 10, 30.0, labels=lab)
    assert got["n_events"] == 37 and got["n_windows"] == 10 and abs(got["density_per_min"] - 37 / 5.0) < 1e-15
    for f in ("duration_s", "amplitude", "freq_hz"):
        v = tab[f]
        st = got[f]
        assert st["n"] == 37 and abs(st["mean"] - v.sum() / 37) < 1e-12 and abs(st["sd"] - np.sqrt(((v - v.mean()) ** 2).mean())) < 1e-12
        assert [st["q25"], st["median"], st["q75"]] == [float(np.percentile(v, p)) for p in (25, 50, 75)]
    assert sorted(got["per_stage"]) == sorted(str(int(c)) for c in np.unique(lab))
    for c in np.unique(lab):
        blk = got["per_stage"][str(int(c))]
        nw = int((lab == c).sum()); pick = lab[win] == c
        assert blk["n_windows"] == nw and blk["n_events"] == int(pick.sum()) and abs(blk["density_per_min"] - pick.sum() / (nw * 0.5)) < 1e-12
        if pick.any():
            assert abs(blk["amplitude"]["mean"] - tab["amplitude"][pick].mean()) < 1e-12
    empty = M.event_summary({"window": np.zeros(0, np.int64), "duration_s": np.zeros(0)}, 4, 30.0)
    assert empty["n_events"] == 0 and empty["density_per_min"] == 0.0 and empty["duration_s"]["mean"] is None and "freq_hz" not in empty


def test_compare_events_equals_its_definition():
    from eegldm import metrics as M
    rng = np.random.default_rng(4)
    real = {"duration_s": rng.uniform(0.5, 3, 41), "amplitude": np.round(rng.uniform(1, 9, 41), 1), "freq_hz": rng.uniform(11, 16, 41)}
    fake = {"duration_s": rng.uniform(0.7, 2, 30), "amplitude": np.round(rng.uniform(2, 7, 30), 1)}
    got = M.compare_events(real, fake)
    assert sorted(got) == ["amplitude", "duration_s"]
    for f in got:
        a, b = real[f], fake[f]
        grid = np.sort(np.concatenate([a, b]))
        fa = np.array([(a <= g).mean() for g in grid]); fb = np.array([(b <= g).mean() for g in grid])
        assert abs(got[f]["ks"] - np.abs(fa - fb).max()) < 1e-15
        assert abs(got[f]["wasserstein"] - np.sum(np.abs(fa - fb)[:-1] * np.diff(grid))) < 1e-12
        assert got[f]["n_real"] == 41 and got[f]["n_synthetic"] == 30
    none = M.compare_events(real, {"duration_s": np.zeros(0)})
    assert none["duration_s"]["ks"] is None and none["duration_s"]["wasserstein"] is None
    same = M.compare_events(real, real)
    assert same["freq_hz"]["ks"] == 0.0 and same["freq_hz"]["wasserstein"] == 0.0


def test_compare_events_equals_scipy():
    stats = pytest.importorskip("scipy.stats")
    from eegldm import metrics as M
    rng = np.random.default_rng(5)
    for n, m in ((1, 1), (7, 50), (200, 180)):
        a, b = rng.standard_normal(n), np.round(rng.standard_normal(m) * 1.5 + 0.3, 2)
        assert abs(M.ks_statistic(a, b) - stats.ks_2samp(a, b).statistic) <= 1e-12
        assert abs(M.wasserstein_1d(a, b) - stats.wasserstein_distance(a, b)) <= 1e-12


def _table(rows, sfreq=100.0, n_windows=3):
    a = np.asarray(rows, np.float64).reshape(-1, 4)
    return {"window": a[:, 0].astype(np.int64), "start": a[:, 1].astype(np.int32), "length": a[:, 2].astype(np.int32), "peak": a[:, 3].astype(np.float32),
            "sfreq": sfreq, "n_windows": n_windows}


def test_pair_half_waves_hand_tables():
    from eegldm import metrics as M
    neg = _table([(0, 10, 50, 4.0), (0, 200, 40, 2.0), (1, 10, 50, 3.0), (2, 5, 30, 1.0)])
    pos = _table([(0, 60, 45, 5.0), (0, 241, 40, 9.0), (1, 60, 70, 2.5), (1, 10, 50, 8.0), (0, 0, 10, 7.0)])
    p = M.pair_half_waves(neg, pos)
    assert p["window"].tolist() == [0, 1] and p["start"].tolist() == [10, 10]            # (0, 200): the positive one starts one sample late; (2, 5): none
    assert p["neg_length"].tolist() == [50, 50] and p["pos_length"].tolist() == [45, 70]
    assert p["amplitude"].tolist() == [9.0, 5.5] and p["duration_s"].tolist() == [0.95, 1.2] and p["mid_s"].tolist() == [0.6, 0.6]
    empty = M.pair_half_waves(neg, _table([]))
    assert len(empty["window"]) == 0 and len(empty["amplitude"]) == 0
    with pytest.raises(ValueError, match="different sets"):
        M.pair_half_waves(neg, _table([], n_windows=4))


def test_events_from_tables_and_event_table():
    from eegldm import metrics as M
    counts = np.array([[2, 5], [0, 0], [3, 3]], np.int32)
    ev_i = np.arange(3 * 2 * 6, dtype=np.int32).reshape(3, 2, 6); ev_f = np.arange(3 * 2 * 4, dtype=np.float32).reshape(3, 2, 4)
    ev = M.events_from_tables(counts, ev_i, ev_f)
    assert ev["stored"].tolist() == [[True, True], [False, False], [True, True]] and ev["n_events"].tolist() == [2, 0, 3]
    t = M.event_table(ev, 100.0)
    assert t["window"].tolist() == [0, 0, 2, 2] and t["truncated"] == 1 and t["n_windows"] == 3
    assert t["start"].tolist() == [0, 6, 24, 30] and t["length"].tolist() == [1, 7, 25, 31] and t["peak"].tolist() == [0.0, 4.0, 16.0, 20.0]
    assert t["mid_s"].tolist() == [0.005, 0.095, 0.365, 0.455]


# ------------------------------------------------------------------------------------------------ the planted construction
@pytest.mark.parametrize("seed", R.PLANT_SEEDS[:2])
def test_planted_spindles_on_the_reference(seed):
    """The construction of the GPU pipeline test, run through the float64 restatement (all five seeds were checked before they were committed;
    two run here): every burst found within 0.25 s, nothing else, nothing in the noise."""
    from eegldm import metrics as M
    lp18, band, box = M.fir_design(100.0, hi=18.0, trans_hz=4.0), M.fir_design(100.0, 11.0, 16.0), M.rms_box(0.2, 100.0)
    noise, x, bursts = R.planted_spindles(seed, lp18)
    env = R.spindles64(noise, np.inf, band, box, 50, 300, 10, False)[1].astype(np.float64)
    thr = env.mean() + R.SPINDLE_FACTOR * env.std()
    for data, want in ((x, 48), (noise, 0)):
        c, i, _f = R.spindles64(data, thr, band, box, 50, 300, 10, False)[2]
        win, slot = np.nonzero(np.arange(32)[None, :] < c[:, :1])
        found, extra = R.match_planted((i[win, slot, 0] + 0.5 * i[win, slot, 1]) / 100.0, win, bursts[:, :, 0], 0.25)
        assert c[:, 0].sum() == want and extra == 0 and (found.all() if want else True)


# ------------------------------------------------------------------------------------------------ the header
def test_header_declares_the_exports():
    src = open(os.path.join(ROOT, "include", "eegldm.h")).read()
    assert re.search(r"int eegldm_fir_same\(eegldm_ctx\*, const float\* x, long ldx, const float\* taps, int M, float\* y, long ldy, long B, int L,", src)
    assert re.search(r"int eegldm_threshold_events\(eegldm_ctx\*, const float\* s, long lds_, const float\* aux, long ldaux, const float\* thr, long B, int L,", src)
    assert re.search(r"#define EEGLDM_ABI_VERSION\s+8\b", src)
