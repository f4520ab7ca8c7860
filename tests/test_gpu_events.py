"""-m gpu: the two primitives of csrc/events.hip and the detectors built on them.  eegldm_fir_same against a float64 evaluation of its
definition within the operation-count bound of tests/events_reference.py, its bit-exact anchors (unit tap, integer data, repeat runs, row and
batch independence, shift invariance across every segment edge, launch geometries, non-finite samples, refusals) and the device sqrtf;
eegldm_threshold_events equal to the sequential reference in every integer and every float bit; the spindle and slow-wave detectors on planted
events; the entry script."""
import json
import os
import time

import numpy as np
import pytest
import torch

import events_reference as R

pytestmark = pytest.mark.gpu
FILL = 7.0e30


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.time()
    yield
    print(f"\nevents_numerics: wall time of tests/test_gpu_events.py {time.time() - t:.1f} s")


def _carve(a, ld, off, fill=FILL):
    """Rows of `a` on the device with row stride ld (>= L), starting `off` floats into an allocation filled with `fill`: a read outside the rows
    shows in every result."""
    n, d = a.shape
    buf = torch.full((off + max(n, 1) * ld + 4,), fill, device="cuda")
    view = buf[off:off + max(n, 1) * ld].view(max(n, 1), ld)[:n, :d]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    return buf, view


def _dev_vec(v, off=0):
    buf = torch.full((off + len(v) + 4,), FILL, device="cuda")
    out = buf[off:off + len(v)]
    out.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32)))
    return out


def _raw_fir(x, taps, y, B, L, M, edge, mode, ldx=None, ldy=None):
    import gpu_util as G
    return G.lib.eegldm_fir_same(G.ctx().h, G.ptr(x), x.stride(0) if ldx is None else ldx, G.ptr(taps), M, G.ptr(y), y.stride(0) if ldy is None else ldy,
                                 B, L, edge, mode)


def _fir(x, taps, edge=0, mode=0, ld=None, x_off=0, t_off=0, y_off=0, ldy=None, check_gutters=True):
    """y (B, L) fp32 numpy of host arrays x (B, L), taps (M,), through carved buffers."""
    import gpu_util as G
    x = np.asarray(x, np.float32); taps = np.asarray(taps, np.float32)
    B, L = x.shape
    ld = L if ld is None else ld
    ldy = L if ldy is None else ldy
    _xb, xv = _carve(x, ld, x_off)
    tv = _dev_vec(taps, t_off)
    ybuf = torch.full((y_off + B * ldy + 4,), FILL, device="cuda")
    yv = ybuf[y_off:y_off + B * ldy].view(B, ldy)[:, :L]
    G.check(_raw_fir(xv, tv, yv, B, L, len(taps), edge, mode, ldx=ld, ldy=ldy))
    torch.cuda.synchronize()
    if check_gutters:
        g = ybuf.cpu().numpy()
        assert np.all(g[:y_off] == np.float32(FILL)) and np.all(g[y_off + B * ldy:] == np.float32(FILL)), "a write outside y"
        assert np.all(g[y_off:y_off + B * ldy].reshape(B, ldy)[:, L:] == np.float32(FILL)), "a write into y's gutters"
    return yv.cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _taps(rng, M):
    """Decaying random taps with both signs (a windowed-sinc look-alike), fp32."""
    k = np.arange(M) - (M - 1) / 2
    return (rng.standard_normal(M) / (1.0 + np.abs(k) / 8.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. FIR against float64
LS = (1, 2, 63, 64, 65, 300, 3000, 3072, 4096)
BS = (1, 5, 130)
MAGS = (1e-3, 1.0, 1e3)
REF_BUDGET = 4.0e7          # multiply-adds of one float64 reference: the batch shrinks (130 -> 5 -> 1) where L * M is large


@pytest.mark.parametrize("M", [1, 3, 15, 17, 165, 1101, 2049])
def test_fir_against_float64(M):
    """|y - y64| <= E elementwise (events_reference.fir_error_bound) over L, B, both edges (reflect wherever c <= L - 1, so M > L runs with
    zeros), both modes, magnitudes 1e-3 .. 1e3, row strides above L, every pointer 0..3 floats off an allocation filled with 7e30, and
    nothing written outside y's rows."""
    rng = np.random.default_rng(100 + M)
    taps = _taps(rng, M)
    c = (M - 1) // 2
    n = 0
    worst = {0: 0.0, 1: 0.0}
    seen = set()
    for L in LS:
        for em in range(4):
            n += 1
            edge, mode = em & 1, em >> 1
            if edge and c > L - 1:
                edge = 0
            B = BS[n % 3]
            while B > 1 and B * L * M > REF_BUDGET:
                B = {130: 5, 5: 1}[B]
            mag = MAGS[(n // 3) % 3]
            x = (rng.standard_normal((B, L)) * mag).astype(np.float32)
            got = _fir(x, taps, edge, mode, ld=L + n % 3, x_off=n % 4, t_off=(n // 4) % 4, y_off=(n // 2) % 4, ldy=L + (n + 1) % 3)
            want, E = R.fir64(x, taps, edge, mode), R.fir_error_bound(x, taps, edge, mode)
            tag = f"M={M} L={L} B={B} edge={edge} mode={mode} mag={mag}"
            assert np.all(np.isfinite(got)), tag
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= E), f"{tag}: off by {err.max():.3e}, bound {E[np.unravel_index(np.argmax(err - E), E.shape)]:.3e}"
            worst[mode] = max(worst[mode], float((err / E).max()))
            seen.update({("B", B), ("mag", mag), ("edge", edge), ("mode", mode)})
    if M <= 165:
        assert all(("B", b) in seen for b in BS)
    assert all(("mag", m) in seen for m in MAGS) and {("edge", 0), ("mode", 0), ("mode", 1)} <= seen and (("edge", 1) in seen or c > max(LS) - 1)
    print(f"events_numerics: fir M={M}: {n} calls, worst error / bound: plain {worst[0]:.3f}, rms {worst[1]:.3f}")


def test_device_sqrtf():
    """M = 1, taps = [1], mode = 1 stores sqrtf(fl32(x * x)): the device sqrtf on its own, held to the SQRTF_ULPS the bound assumes."""
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((256, 4096)) * np.exp(rng.uniform(-40.0, 40.0, (256, 4096)))).astype(np.float32)
    x[0, :4] = (0.0, 1.0, 2.0, 3.0)
    got = _fir(x, [1.0], 0, 1).astype(np.float64)
    sq = (x * x).astype(np.float64)                       # fl32(x * x) exactly as staged
    want = np.sqrt(sq)
    ok = (sq >= 2.0 ** -126) & np.isfinite(sq)             # normal squares: an ulp of the root is well defined
    ulp = 2.0 ** (np.floor(np.log2(np.where(ok, want, 1.0))) - 23)
    err = np.where(ok, np.abs(got - want) / ulp, 0.0)
    print(f"events_numerics: device sqrtf over {int(ok.sum())} values: largest error {err.max():.4f} ulp (the bound assumes {R.SQRTF_ULPS})")
    assert err.max() <= R.SQRTF_ULPS
    assert got[0, 0] == 0.0 and got[0, 1] == 1.0 and got[0, 2] == 2.0 and got[0, 3] == 3.0


# ------------------------------------------------------------------------------------------------ 2. FIR bit-exact anchors
def test_fir_unit_tap_and_integers():
    rng = np.random.default_rng(8)
    for L in (1, 65, 3000, 4096):
        x = rng.standard_normal((3, L)).astype(np.float32)
        assert np.array_equal(_bits(_fir(x, [1.0])), _bits(x)), L
    for L, M, edge in ((300, 15, 1), (3000, 165, 0), (4096, 17, 1), (64, 165, 0)):
        x = rng.integers(-8, 9, (5, L)).astype(np.float32); t = rng.integers(-4, 5, M).astype(np.float32)
        got = _fir(x, t, edge, 0)
        assert np.array_equal(got.astype(np.float64), R.fir64(x, t, edge, 0)), (L, M, edge)          # every partial sum is a small integer: exact


def test_fir_repeats_and_row_independence():
    """Run == run; a row alone == the same row inside a batch of 130 (another grid: 16 segments against 4 at L = 4096)."""
    rng = np.random.default_rng(9)
    for L, M, edge, mode in ((4096, 165, 1, 0), (3000, 1101, 1, 1), (3072, 2049, 0, 0), (65, 17, 0, 1)):
        x = rng.standard_normal((130, L)).astype(np.float32); t = _taps(rng, M)
        a, b = _fir(x, t, edge, mode), _fir(x, t, edge, mode)
        assert np.array_equal(_bits(a), _bits(b))
        for r in (0, 77, 129):
            assert np.array_equal(_bits(_fir(x[r:r + 1], t, edge, mode)), _bits(a[r:r + 1])), (L, M, r)
        assert np.array_equal(_bits(_fir(x[40:45], t, edge, mode)), _bits(a[40:45]))


@pytest.mark.parametrize("mode", [0, 1])
def test_fir_shift_invariance(mode):
    """The same samples 1, 7 and 64 places further along the row give the same output bits, shifted: an output depends only on its support,
    not on the thread, the register slot or the segment that computed it.  B = 1 at L = 4096 runs 16 segments of 256 outputs, B = 130 four of
    1024: every segment edge is crossed by some shift."""
    rng = np.random.default_rng(10 + mode)
    L, M = 4096, 165
    c = (M - 1) // 2
    core = rng.standard_normal(L).astype(np.float32)
    t = _taps(rng, M)
    for B in (1, 130):
        base = None
        for s in (0, 1, 7, 64):
            x = rng.standard_normal((B, L)).astype(np.float32)
            x[B // 2, s:] = core[:L - s]
            y = _fir(x, t, 0, mode)[B // 2]
            inner = y[s + c:L - c]                         # outputs whose whole support lies inside the copied samples
            if base is None:
                base = inner
            else:
                assert np.array_equal(_bits(inner), _bits(base[:len(inner)])), (B, s)


def test_fir_launch_geometries():
    """The developer switches EEGLDM_FIR_R (outputs per thread: 4, 8, 12) and EEGLDM_FIR_SEGS (at least so many segments per row) change the
    launch, not one bit of the result."""
    import gpu_util as G
    rng = np.random.default_rng(12)
    try:
        for L, M, edge, mode, B in ((4096, 1101, 1, 0, 3), (3000, 165, 1, 1, 130), (300, 17, 0, 0, 5), (65, 2049, 0, 1, 2)):
            x = rng.standard_normal((B, L)).astype(np.float32); t = _taps(rng, M)
            os.environ.pop("EEGLDM_FIR_R", None); os.environ.pop("EEGLDM_FIR_SEGS", None); G.lib.eegldm_debug_reload_env()
            want = _fir(x, t, edge, mode)
            for r, segs in ((4, 0), (8, 0), (12, 7), (8, 33), (4, 1000), (12, 4096)):
                os.environ["EEGLDM_FIR_R"] = str(r); os.environ["EEGLDM_FIR_SEGS"] = str(segs); G.lib.eegldm_debug_reload_env()
                assert np.array_equal(_bits(_fir(x, t, edge, mode)), _bits(want)), (L, M, r, segs)
    finally:
        os.environ.pop("EEGLDM_FIR_R", None); os.environ.pop("EEGLDM_FIR_SEGS", None); G.lib.eegldm_debug_reload_env()


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_fir_non_finite_samples(bad):
    """An inf or a NaN at the first, the last and an interior sample: the non-finite outputs are exactly those whose support holds the sample
    (with reflection: a reflected copy of it too); every other output has the bits of the run with a zero there."""
    rng = np.random.default_rng(13)
    for L, M, edge, mode in ((300, 17, 0, 0), (300, 17, 1, 0), (3000, 165, 1, 1), (4096, 165, 0, 1), (3000, 1101, 0, 0), (65, 165, 0, 0), (64, 15, 1, 1)):
        t = _taps(rng, M)
        t[M // 3] = 0.0                                   # a stored zero tap must not hide the sample (inf * 0) nor spread it
        for idx in (0, L - 1, L // 2 + 3):
            x = rng.standard_normal((2, L)).astype(np.float32)
            x0 = x.copy(); x0[1, idx] = 0.0
            x[1, idx] = bad
            got, clean = _fir(x, t, edge, mode), _fir(x0, t, edge, mode)
            hit = R.support_mask_reflect(L, M, idx) if edge else R.support_mask(L, M, idx)
            assert np.array_equal(~np.isfinite(got[1]), hit), (L, M, edge, mode, idx)
            assert np.array_equal(_bits(got[1][~hit]), _bits(clean[1][~hit])) and np.array_equal(_bits(got[0]), _bits(clean[0]))


def test_fir_refusals():
    import gpu_util as G
    x = torch.zeros(4, 300, device="cuda"); t = torch.ones(2049, device="cuda")
    y = torch.full((4, 300), FILL, device="cuda")
    h = G.ctx().h
    cases = {
        "null x": lambda: G.lib.eegldm_fir_same(h, None, 300, G.ptr(t), 15, G.ptr(y), 300, 4, 300, 0, 0),
        "null taps": lambda: G.lib.eegldm_fir_same(h, G.ptr(x), 300, None, 15, G.ptr(y), 300, 4, 300, 0, 0),
        "null y": lambda: G.lib.eegldm_fir_same(h, G.ptr(x), 300, G.ptr(t), 15, None, 300, 4, 300, 0, 0),
        "null ctx": lambda: G.lib.eegldm_fir_same(None, G.ptr(x), 300, G.ptr(t), 15, G.ptr(y), 300, 4, 300, 0, 0),
        "M even": lambda: _raw_fir(x, t, y, 4, 300, 16, 0, 0),
        "M 0": lambda: _raw_fir(x, t, y, 4, 300, 0, 0, 0),
        "M -1": lambda: _raw_fir(x, t, y, 4, 300, -1, 0, 0),
        "M 2051": lambda: _raw_fir(x, t, y, 4, 300, 2051, 0, 0),
        "L 0": lambda: _raw_fir(x, t, y, 4, 0, 15, 0, 0),
        "L 4097": lambda: _raw_fir(x, t, y, 4, 4097, 15, 0, 0, ldx=5000, ldy=5000),
        "reflect too long": lambda: _raw_fir(x, t, y, 4, 300, 601, 1, 0),
        "ldx": lambda: _raw_fir(x, t, y, 4, 300, 15, 0, 0, ldx=299),
        "ldy": lambda: _raw_fir(x, t, y, 4, 300, 15, 0, 0, ldy=299),
        "edge 2": lambda: _raw_fir(x, t, y, 4, 300, 15, 2, 0),
        "edge -1": lambda: _raw_fir(x, t, y, 4, 300, 15, -1, 0),
        "mode 2": lambda: _raw_fir(x, t, y, 4, 300, 15, 0, 2),
        "in place": lambda: _raw_fir(y, t, y, 4, 300, 15, 0, 0),
        "B < 0": lambda: _raw_fir(x, t, y, -1, 300, 15, 0, 0),
    }
    for name, call in cases.items():
        assert call() != 0, name
        assert len(G.lib.eegldm_last_error()) > 0
    torch.cuda.synchronize()
    assert bool((y == FILL).all()), "a refused call wrote to y"
    assert _raw_fir(x, t, y, 0, 300, 15, 0, 0) == 0                   # B == 0: a successful no-op
    assert _raw_fir(x, t, y, 4, 300, 599, 1, 0) == 0                  # c = 299 = L - 1: the longest reflection
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())


# ------------------------------------------------------------------------------------------------ 3. events, equal to the reference
SENT_I, SENT_F = -77, -77.5


def _events(s, thr, aux=None, E=8, lds=None, off=0, **kw):
    """The export on host arrays -> (counts, ev_i, ev_f) numpy; the tables start out filled with sentinels."""
    import gpu_util as G
    s = np.asarray(s, np.float32)
    B, L = s.shape
    lds = L if lds is None else lds
    _sb, sv = _carve(s, lds, off)
    av = None
    if aux is not None:
        _ab, av = _carve(np.asarray(aux, np.float32), lds + 1, (off + 1) % 4)
    tv = _dev_vec(np.asarray(thr, np.float32), (off + 2) % 4)
    counts = torch.full((B, 2), SENT_I, dtype=torch.int32, device="cuda")
    ev_i = torch.full((B, E, 6), SENT_I, dtype=torch.int32, device="cuda")
    ev_f = torch.full((B, E, 4), SENT_F, dtype=torch.float32, device="cuda")
    G.check(G.lib.eegldm_threshold_events(G.ctx().h, G.ptr(sv), lds, G.ptr(av), lds + 1 if av is not None else 0, G.ptr(tv), B, L, kw.get("min_len", 1),
                                          kw.get("max_len", L), kw.get("merge_gap", 0), 1 if kw.get("drop_edge") else 0, E, G.ptr(counts), G.ptr(ev_i),
                                          G.ptr(ev_f)))
    torch.cuda.synchronize()
    return counts.cpu().numpy(), ev_i.cpu().numpy(), ev_f.cpu().numpy()


def _same_floats(a, b):
    """Bit-equal, except that any NaN equals any NaN (the payload of a NaN sum is not part of the definition)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.int32) == b.view(np.int32)) | nan))


def _check_events(s, thr, aux=None, E=8, tag="", **kw):
    s = np.asarray(s, np.float32)
    B, L = s.shape
    got = _events(s, thr, aux, E=E, **kw)
    want = R.threshold_events(s, thr, aux, min_len=kw.get("min_len", 1), max_len=kw.get("max_len", L), merge_gap=kw.get("merge_gap", 0),
                              drop_edge=kw.get("drop_edge", False), max_events=E, counts=np.full((B, 2), SENT_I, np.int32),
                              ev_i=np.full((B, E, 6), SENT_I, np.int32), ev_f=np.full((B, E, 4), SENT_F, np.float32))
    assert np.array_equal(got[0], want[0]), f"{tag}: counts {got[0].tolist()[:4]} want {want[0].tolist()[:4]}"
    bad = np.nonzero((got[1] != want[1]).any(2))
    assert np.array_equal(got[1], want[1]), f"{tag}: ev_i differs first at row {bad[0][:1]} slot {bad[1][:1]}: {got[1][bad][:1].tolist()} want {want[1][bad][:1].tolist()}"
    assert _same_floats(got[2], want[2]), f"{tag}: ev_f"
    return got


def _row(L, runs, lo=0.0):
    """A row that is `lo` outside the runs and 1 + a small ramp inside them."""
    s = np.full(L, lo, np.float32)
    for a, b in runs:
        a, b = max(a, 0), min(b, L)
        if b > a:
            s[a:b] = 1.0 + 0.001 * (np.arange(a, b) % 17)
    return s


@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 3000, 4096])
def test_events_crafted(L):
    rng = np.random.default_rng(20 + L)
    aux = rng.integers(-1, 2, (1, L)).astype(np.float32)                       # exact zeros in aux: n_up counts < 0 followed by >= 0
    thr = [0.5]
    n_cases = 0

    def go(runs, tag, s=None, a=aux, t=thr, **kw):
        nonlocal n_cases
        n_cases += 1
        row = _row(L, runs)[None, :] if s is None else np.asarray(s, np.float32).reshape(1, L)
        return _check_events(row, t, a, tag=f"L={L} {tag}", off=n_cases % 4, lds=L + n_cases % 3, **kw)

    for dg in (False, True):
        go([], f"nothing active drop_edge={dg}", drop_edge=dg)
        c = go([(0, L)], f"whole row active drop_edge={dg}", drop_edge=dg)
        assert c[0].tolist() == [[0 if dg else 1, 1]]
    go([(0, L)], "whole row active, longer than max_len", max_len=max(L - 1, 1), min_len=1) if L > 1 else None
    # runs that start or stop at 63 / 64 / 65 and at the row ends
    for a, b in ((0, 1), (0, 3), (60, 63), (60, 64), (60, 65), (63, 64), (63, 70), (64, 65), (64, 70), (65, 70), (L - 3, L), (L - 1, L), (1, L - 1), (1, L), (0, L - 1),
                 (127, 129), (128, 192), (3 * 64, 5 * 64), (L - 65, L - 1), (L - 64, L), (2000, 2900)):
        if 0 <= a < b <= L:
            for dg in (False, True):
                go([(a, b)], f"run [{a}, {b}) drop_edge={dg}", drop_edge=dg)
            go([(a, b)], f"run [{a}, {b}) no aux", a=None)
    if L >= 63:
        # merge_gap 0; a gap of exactly merge_gap and of merge_gap + 1, inside a lane and across lane boundaries
        for g in (1, 2, 5, 40, 70):
            for p in (10, 30, 60, 62):
                if p + g + 12 <= L:
                    runs = [(p - 8, p), (p + g, p + g + 12)]
                    go(runs, f"gap {g} at {p} merge_gap 0", merge_gap=0)
                    go(runs, f"gap {g} at {p} merge_gap == gap", merge_gap=g)
                    go(runs, f"gap {g} at {p} merge_gap == gap - 1", merge_gap=g - 1)
        # a gap that touches a row end is never filled
        go([(3, 10), (L - 9, L - 2)], "stretches at both row ends", merge_gap=5)
        go([(3, 10), (L - 9, L - 2)], "stretches at both row ends, drop_edge", merge_gap=5, drop_edge=True)
        # min_len / max_len at the boundary
        for n in (1, 7, 40):
            go([(5, 5 + n), (50, 50 + n - 1 if n > 1 else 51)], f"length {n} against min_len", min_len=n)
            go([(5, 5 + n), (50, 50 + n + 1)], f"length {n} against max_len", max_len=n)
        # more events than slots: the counts go on, the slots past the stored ones keep the sentinel
        runs = [(4 * k, 4 * k + 2) for k in range(L // 4)]
        c = go(runs, "more events than E", E=4)
        assert c[0][0, 0] == len(runs) and np.all(c[1][0, :4, 0] == [0, 4, 8, 12])
        c = go(runs[:3], "fewer events than E", E=8)
        assert np.all(c[1][0, 3:] == SENT_I) and np.all(c[2][0, 3:] == np.float32(SENT_F))
        go(runs, "E = 1", E=1); go(runs, "E = 64", E=64, merge_gap=1); go(runs, "E = 64, all merged", E=64, merge_gap=2)
        # NaN in s (inactive: it splits a run, and inside a closed gap it makes the sum NaN), NaN / inf thresholds, ties
        s = _row(L, [(10, 40)]); s[20] = np.nan; s[30] = np.nan
        go([], "NaN splits a run", s=s); c = go([], "NaN inside a closed gap", s=s, merge_gap=1)
        assert np.isnan(c[2][0, 0, 1]) and c[1][0, 0, :2].tolist() == [10, 30]
        an = aux.copy(); an[0, 10] = np.nan; an[0, 25] = np.nan
        go([(10, 40)], "NaN at aux[start] and inside", a=an); go([(8, 40)], "NaN inside aux", a=an)
        for t in (np.nan, np.inf, -np.inf):
            go([(10, 40)], f"thr {t}", t=[t])
        s = _row(L, [(10, 40)]); s[5] = -np.inf; s[6] = np.inf
        go([], "inf in s, thr -inf", s=s, t=[-np.inf]); go([], "inf in s", s=s)
        s = np.full(L, 0.5, np.float32); s[20:30] = np.nextafter(np.float32(0.5), np.float32(1))
        c = go([], "ties are inactive", s=s)
        assert c[1][0, 0, :2].tolist() == [20, 10]
        # the first argmax on a plateau
        s = _row(L, []); s[10:20] = (1, 3, 3, 2, 3, 1, 1, 1, 1, 1)
        c = go([], "plateau", s=s)
        assert c[1][0, 0, 2] == 11 and c[2][0, 0, 0] == 3.0 and c[2][0, 0, 1] == 17.0
        # n_up with exact zeros: -1 0 (up) 0 0 (not) -1 1 (up) 1 -0.0 (not: -0 is not < 0) -1 -0.0 (up: -0 >= 0)
        a0 = np.zeros((1, L), np.float32); a0[0, 10:22] = (-1, 0, 0, 0, -1, 1, 1, -0.0, 1, -1, -0.0, 5)
        c = go([(10, 22)], "n_up with zeros", a=a0)
        assert c[1][0, 0, 3] == 3 and c[2][0, 0, 2:].tolist() == [5.0, -1.0]
        c = go([(11, 22)], "n_up starts after the first crossing", a=a0)
        assert c[1][0, 0, 3] == 2
    if L >= 200:
        # a chain of four raw runs merged transitively across three lanes (gaps 4, 5, 3; the first gap crosses the lane boundary at 64)
        chain = [(50, 62), (66, 120), (125, 130), (133, 200)]
        c = go(chain, "chain of four", merge_gap=5)
        assert c[0].tolist() == [[1, 4]] and c[1][0, 0, [0, 1, 4]].tolist() == [50, 150, 4]
        c = go(chain, "chain broken at the widest gap", merge_gap=4)
        assert c[0].tolist() == [[2, 4]] and c[1][0, :2, 4].tolist() == [2, 2]
    if L >= 3000:
        # a closed run across many lanes; a gap wider than a lane; runs and gaps on every lane boundary
        go([(100, 1000), (1070, 2000), (2000 + 65, 2900)], "gaps wider than a lane", merge_gap=70)
        go([(100, 1000), (1070, 2000), (2000 + 65, 2900)], "gaps wider than a lane, one closed", merge_gap=65)
        go([(64 * k - 1, 64 * k + 1) for k in range(1, L // 64)], "a run on every lane boundary", E=64)
        go([(64 * k + 1, 64 * k + 63) for k in range(L // 64)], "a gap on every lane boundary", E=64, merge_gap=2)
        go([(64 * k + 1, 64 * k + 63) for k in range(L // 64)], "a gap on every lane boundary, open", E=64, merge_gap=1)
    print(f"events_numerics: events L={L}: {n_cases} crafted cases equal to the reference")


@pytest.mark.parametrize("B", [1, 5, 130])
def test_events_random_rows(B):
    """Smoothed noise at three activity rates, every gate in play, with and without aux; run == run."""
    rng = np.random.default_rng(30 + B)
    n = 0
    for L in (4096, 3000, 65):
        for rate in (0.1, 0.5, 0.9):
            n += 1
            w = rng.standard_normal((B, L + 8))
            s = np.stack([np.convolve(r, np.ones(9) / 3.0, "valid") for r in w]).astype(np.float32)
            aux = (rng.standard_normal((B, L)) * (rng.random((B, L)) < 0.8)).astype(np.float32)
            thr = np.quantile(s, 1.0 - rate, axis=1).astype(np.float32)
            thr[::7] = s[::7, L // 2]                                         # ties with a sample of the row
            kw = dict(min_len=(1, 3, 8)[n % 3], max_len=(L, 40, 400)[n % 3], merge_gap=(0, 2, 9)[(n // 3) % 3], drop_edge=bool(n % 2), E=(64, 8, 32)[n % 3])
            a = _check_events(s, thr, aux if n % 4 else None, tag=f"B={B} L={L} rate={rate}", lds=L + n % 3, off=n % 4, **kw)
            b = _events(s, thr, aux if n % 4 else None, lds=L + n % 3, off=n % 4, **kw)
            assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(a, b))


def test_events_refusals():
    import gpu_util as G
    h = G.ctx().h
    s = torch.zeros(4, 300, device="cuda"); thr = torch.zeros(4, device="cuda")
    counts = torch.full((4, 2), SENT_I, dtype=torch.int32, device="cuda"); ev_i = torch.full((4, 8, 6), SENT_I, dtype=torch.int32, device="cuda")
    ev_f = torch.full((4, 8, 4), SENT_F, device="cuda")
    P = G.ptr

    def call(s_=s, lds=300, aux=None, ldaux=0, thr_=thr, B=4, L=300, mn=1, mx=300, mg=0, E=8, c=counts, i=ev_i, f=ev_f, ctx=h):
        return G.lib.eegldm_threshold_events(ctx, P(s_), lds, P(aux), ldaux, P(thr_), B, L, mn, mx, mg, 0, E, P(c), P(i), P(f))

    cases = {"null ctx": dict(ctx=None), "null s": dict(s_=None), "null thr": dict(thr_=None), "null counts": dict(c=None), "null ev_i": dict(i=None),
             "null ev_f": dict(f=None), "L 0": dict(L=0), "L 4097": dict(L=4097, lds=5000), "min_len 0": dict(mn=0), "max_len < min_len": dict(mn=5, mx=4),
             "merge_gap -1": dict(mg=-1), "E 0": dict(E=0), "E 65": dict(E=65), "lds": dict(lds=299), "ldaux": dict(aux=s, ldaux=299), "B < 0": dict(B=-1)}
    for name, kw in cases.items():
        assert call(**kw) != 0, name
    torch.cuda.synchronize()
    assert bool((counts == SENT_I).all()) and bool((ev_i == SENT_I).all()) and bool((ev_f == SENT_F).all())
    assert call(B=0) == 0 and call() == 0
    torch.cuda.synchronize()
    assert bool((counts == 0).all()) and bool((ev_i == SENT_I).all())


# ------------------------------------------------------------------------------------------------ 4. the detectors on planted events
@pytest.fixture(scope="module")
def lp18():
    from eegldm import metrics as M
    return M.fir_design(100.0, hi=18.0, trans_hz=4.0)


@pytest.mark.parametrize("seed", R.PLANT_SEEDS)
def test_planted_spindles(seed, lp18):
    """16 windows of 18-Hz-low-passed unit noise with three planted bursts each (events_reference.planted_spindles), threshold = envelope_threshold of
    the noise-only set at factor 3.0 (1.5 leaves 1 to 5 noise events per seed in the float64 restatement): every burst has an event whose
    midpoint lies within 0.25 s of its centre, no other event exists, the noise-only set has none.

    freq_hz = n_up * sfreq / length counts upward crossings over the run, so it is quantised to 1 / duration (1.7 Hz for a 0.6-s run); the
    float64 restatement puts it within 1.05 .. 1.27 Hz of the planted frequency over the five seeds (within 1.3 crossings).  Held here to two
    crossings over the run's duration: one for the count's truncation at the run's two ends, one for a crossing the noise adds or removes in
    the margins, where the burst has fallen to the noise's own amplitude at the threshold.  Beside it an absolute cap of 1.5 Hz, so that a wrong
    n_up cannot hide on short runs: one systematic extra crossing on the shortest kept run (0.5 s) would be 2 Hz, above the cap."""
    from eegldm import metrics as M
    noise, x, bursts = R.planted_spindles(seed, lp18)
    thr = M.envelope_threshold(torch.from_numpy(noise), factor=R.SPINDLE_FACTOR)
    got = M.detect_spindles(torch.from_numpy(x)[:, None, :], thr, merge_s=0.1, drop_edge=False)
    found, extra = R.match_planted(got["mid_s"], got["window"], bursts[:, :, 0], 0.25)
    err_hz = err_cross = 0.0
    for w, m, f, d in zip(got["window"], got["mid_s"], got["freq_hz"], got["duration_s"]):
        k = int(np.argmin(np.abs(bursts[w, :, 0] - m)))
        err_hz = max(err_hz, abs(f - bursts[w, k, 2])); err_cross = max(err_cross, abs(f - bursts[w, k, 2]) * d)
    quiet = M.detect_spindles(torch.from_numpy(noise), thr, merge_s=0.1, drop_edge=False)
    print(f"events_numerics: planted spindles seed {seed}: threshold {thr:.4f}, {int(found.sum())} of {found.size} bursts found, {extra} other events, "
          f"{len(quiet['window'])} events in the noise, freq_hz within {err_hz:.2f} Hz = {err_cross:.2f} crossings, amplitude {got['amplitude'].min():.2f} .. "
          f"{got['amplitude'].max():.2f}")
    assert found.all() and extra == 0 and len(got["window"]) == found.size and got["truncated"] == 0
    assert len(quiet["window"]) == 0
    assert err_cross <= 2.0 and err_hz <= 1.5
    assert np.all((got["duration_s"] >= 0.5) & (got["duration_s"] <= 3.0)) and np.all(got["amplitude"] > 1.5) and np.all(got["amplitude"] < 9.0)
    # the device tables against the float64 restatement of the same pipeline: the same events wherever no sample sits within the filters' error of the threshold
    band, box = M.fir_design(100.0, 11.0, 16.0), M.rms_box(0.2, 100.0)
    c, i, _f = R.spindles64(x, thr, band, box, 50, 300, 10, False)[2]
    assert int(c[:, 0].sum()) == len(got["window"])
    win, slot = np.nonzero(np.arange(32)[None, :] < c[:, :1])
    assert np.array_equal(win, got["window"]) and np.all(np.abs(i[win, slot, 0] - got["start"]) <= 1) and np.all(np.abs(i[win, slot, 1] - got["length"]) <= 2)


def test_envelope_threshold_default_band(lp18):
    """envelope_threshold(real, factor) as the README writes it uses detect_spindles' band (11, 16) Hz; `band=` and band_envelope's lo / hi reach
    the filter; the value is mean + factor * sd of the envelope in float64; chunking only re-associates the float64 sums."""
    from eegldm import metrics as M
    noise = torch.from_numpy(R.lowpass_noise(3, lp18)[0])
    thr = M.envelope_threshold(noise, factor=3.0)
    assert thr == M.envelope_threshold(noise, factor=3.0, band=(11.0, 16.0)) == M.envelope_threshold(noise[:, None, :], 3.0, lo=11.0, hi=16.0)
    env = M.band_envelope(noise, 11.0, 16.0)[1].double().cpu().numpy()
    assert abs(thr - (env.mean() + 3.0 * env.std())) <= 1e-12 * thr
    assert abs(M.envelope_threshold(noise, factor=3.0, batch_size=5) - thr) <= 1e-12 * thr
    other = M.envelope_threshold(noise, factor=3.0, band=(2.0, 6.0))
    env2 = M.band_envelope(noise, 2.0, 6.0)[1].double().cpu().numpy()
    assert abs(other - (env2.mean() + 3.0 * env2.std())) <= 1e-12 * other and abs(other - thr) > 0.01 * thr
    assert M.envelope_threshold(noise, factor=0.0, rms_s=0.5) != M.envelope_threshold(noise, factor=0.0)


SW_MIN_AMP, SW_MAX_S = 2.5, 2.0


@pytest.mark.parametrize("seed", R.PLANT_SEEDS)
def test_planted_slow_waves(seed, lp18):
    """Three planted slow waves per window (a negative half-sine of 0.6 s, then a positive one of 0.5 s, amplitude 5) on the same noise, low-passed
    at 4 Hz: detect_half_waves of both polarities + pair_half_waves finds every one (zero crossing within 0.1 s) and nothing else; the
    noise-only set yields no pair.

    min_amp = 2.5: the 4-Hz-low-passed noise has a standard deviation of 0.28, so its largest half-wave peak over 16 x 3000 samples is about
    4.5 sd = 1.3 (0.73 .. 0.95 in the float64 restatement, five seeds) while a planted peak keeps at least 5 - 5 sd = 3.6 (4.6 at the least
    there).  max_s = 2.0, not the literature's 1.0: a half-wave lasts until the SUM changes sign, and once the planted wave
    has ended that is up to the noise, which keeps its sign for up to 1.2 s here; with max_s = 1.0 the restatement loses 2 to 6 of the 48
    waves per seed to the duration gate, with 2.0 none."""
    from eegldm import metrics as M
    noise, x, t0 = R.planted_slow_waves(seed, lp18)
    pairs = {}
    for name, data in (("noise", noise), ("planted", x)):
        neg = M.detect_half_waves(torch.from_numpy(data), polarity=-1, max_s=SW_MAX_S, min_amp=SW_MIN_AMP)
        pos = M.detect_half_waves(torch.from_numpy(data), polarity=1, max_s=SW_MAX_S, min_amp=SW_MIN_AMP)
        pairs[name] = M.pair_half_waves(neg, pos)
    p = pairs["planted"]
    found, extra = R.match_planted(p["mid_s"], p["window"], t0 + R.SW_NEG_S, 0.1)
    print(f"events_numerics: planted slow waves seed {seed}: {int(found.sum())} of {found.size} found, {extra} other pairs, {len(pairs['noise']['window'])} pairs in "
          f"the noise, peak to peak {p['amplitude'].min():.2f} .. {p['amplitude'].max():.2f}, duration {p['duration_s'].min():.2f} .. {p['duration_s'].max():.2f} s")
    assert found.all() and extra == 0 and len(p["window"]) == found.size
    assert len(pairs["noise"]["window"]) == 0
    assert np.all(p["amplitude"] > 2 * 3.6) and np.all(p["amplitude"] < 2 * 6.4) and np.all(p["duration_s"] >= R.SW_NEG_S + R.SW_POS_S - 0.1)


def test_micro_structure_script_round_trip(tmp_path, lp18):
    from eegldm.entry import micro_structure as S
    _n, real, _b = R.planted_spindles(0, lp18)
    _n, syn, _b = R.planted_spindles(1, lp18)
    _n, sw, _t = R.planted_slow_waves(2, lp18)
    real = np.concatenate([real, sw[:8]])[:, None, :]                       # (24, 1, 3000)
    syn = np.concatenate([syn[:6], sw[8:12]])[:, None, :]                    # (10, 1, 3000)
    os.makedirs(tmp_path / "syn")
    np.save(tmp_path / "syn" / "sample_0.npy", syn[:4]); np.save(tmp_path / "syn" / "sample_1.npy", syn[4:])
    np.save(tmp_path / "syn" / "sample_0_label.npy", np.array([2, 2, 2, 2])); np.save(tmp_path / "syn" / "sample_1_label.npy", np.array([2, 2, 3, 3, 3, 3]))
    np.save(tmp_path / "hold.npy", real)
    out = str(tmp_path / "micro_structure.json")
    res = S.main(S.parse_args(["--samples", str(tmp_path / "syn" / "sample_*.npy"), "--holdout_npy", str(tmp_path / "hold.npy"), "--labels_from_samples",
                               "--thr_factor", "1.0", "--min_amp", "2.5", "--chunk", "7", "--seed", "1", "--output", out]))
    with open(out) as f:
        back = json.load(f)
    assert back == json.loads(json.dumps(res))
    assert back["n_real"] == 24 and back["n_synthetic"] == 10 and back["window_s"] == 30.0 and len(back["files"]) == 2
    assert back["args"]["thr_factor"] == 1.0 and back["thresholds"]["half_wave_min_amp"] == 2.5 and back["thresholds"]["spindle_envelope"] > 0
    for side, n in (("real", 24), ("synthetic", 10)):
        for kind in ("spindles", "slow_waves"):
            b = back[side][kind]
            assert b["n_windows"] == n and b["n_events"] >= 6 and abs(b["density_per_min"] - b["n_events"] / (n * 0.5)) < 1e-12
            assert b["duration_s"]["n"] == b["n_events"] and b["amplitude"]["mean"] > 0
        assert 11.0 < back[side]["spindles"]["freq_hz"]["mean"] < 16.0 and "freq_hz" not in back[side]["slow_waves"]
    assert "per_stage" not in back["real"]["spindles"]
    st = back["synthetic"]["spindles"]["per_stage"]
    assert sorted(st) == ["2", "3"] and st["2"]["n_windows"] == 6 and st["3"]["n_windows"] == 4 and st["2"]["n_events"] >= 9 and st["2"]["n_events"] + st["3"]["n_events"] == back["synthetic"]["spindles"]["n_events"]
    # planted: 12 and 24; the literature's 1-s gate on a half-wave loses some of them to the noise's tail (see test_planted_slow_waves)
    assert 6 <= back["synthetic"]["slow_waves"]["per_stage"]["3"]["n_events"] <= 12 and 12 <= back["real"]["slow_waves"]["n_events"] <= 24
    assert back["synthetic"]["slow_waves"]["per_stage"]["2"]["n_events"] == 0
    for block in ("real_vs_synthetic", "real_vs_real"):
        for kind, feats in (("spindles", ("duration_s", "amplitude", "freq_hz")), ("slow_waves", ("duration_s", "amplitude"))):
            assert sorted(back[block][kind]) == sorted(feats)
            for f in feats:
                v = back[block][kind][f]
                assert 0.0 <= v["ks"] <= 1.0 and v["wasserstein"] >= 0.0 and v["n_real"] > 0 and v["n_synthetic"] > 0
    assert back["real_vs_real"]["n"] == [12, 12]
    assert "nobody has validated" in back["caveat"] and "not evidence of realism" in back["caveat"]
    # chunking changes nothing, and the default min_amp comes from the real set
    res2 = S.main(S.parse_args(["--samples", str(tmp_path / "syn" / "sample_*.npy"), "--holdout_npy", str(tmp_path / "hold.npy"), "--thr_factor", "1.0",
                                "--seed", "1", "--output", out]))
    assert res2["real"]["spindles"] == {k: v for k, v in res["real"]["spindles"].items() if k != "per_stage"} and res2["thresholds"]["half_wave_min_amp"] > 0
