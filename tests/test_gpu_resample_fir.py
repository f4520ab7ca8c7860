"""-m gpu: the two primitives of csrc/resample.hip and the preparation pipeline built on them.  eegldm_resample_fir against the float64
definition within the operation-count bound of tests/recordings_reference.py (every element; both edges; fp32 and int16 rows; strides,
gutters and alignments), its bit-exact anchors (eegldm_fir_same at U = D = 1, launch geometries, shifted sub-rows, repeat runs), non-finite
samples, every refusal; eegldm_epoch_stats against float64; python -m eegldm.entry.prepare_recordings end to end on written files."""
import csv
import json
import os
import time

import numpy as np
import pytest
import torch

import recordings_reference as R

pytestmark = pytest.mark.gpu
FILL = 7.0e30


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.time()
    yield
    print(f"\nresample_numerics: wall time of tests/test_gpu_resample_fir.py {time.time() - t:.1f} s")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _carve(a, ld, off, dtype):
    """Rows of `a` on the device with row stride ld, `off` elements into an allocation filled with a loud value."""
    n, d = a.shape
    fill = FILL if dtype == torch.float32 else 32000
    buf = torch.full((off + n * ld + 8,), fill, device="cuda", dtype=dtype)
    view = buf[off:off + n * ld].view(n, ld)[:, :d]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, view


def _dev_vec(v, off=0):
    buf = torch.full((off + len(v) + 4,), FILL, device="cuda")
    out = buf[off:off + len(v)]
    out.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32)))
    return out


def _resample(x, taps, U, D, edge=0, gain=None, offset=None, ldx=None, ldy=None, x_off=0, t_off=0, y_off=0):
    """(B, Lout) fp32 numpy through carved buffers; y's gutters and surroundings start as NaN and must stay NaN."""
    import gpu_util as G
    x = np.asarray(x)
    is16 = x.dtype == np.int16
    if not is16:
        x = x.astype(np.float32)
    taps = np.asarray(taps, np.float32)
    B, L = x.shape
    lout = R.out_len(L, U, D)
    ldx = L if ldx is None else ldx
    ldy = lout if ldy is None else ldy
    _xb, xv = _carve(x, ldx, x_off, torch.int16 if is16 else torch.float32)
    tv = _dev_vec(taps, t_off)
    gv = _dev_vec(gain) if is16 else None
    ov = _dev_vec(offset) if is16 else None
    ybuf = torch.full((y_off + B * ldy + 4,), float("nan"), device="cuda")
    yv = ybuf[y_off:y_off + B * ldy].view(B, ldy)[:, :lout]
    G.check(G.lib.eegldm_resample_fir(G.ctx().h, G.ptr(xv), ldx, 1 if is16 else 0, G.ptr(gv), G.ptr(ov), G.ptr(tv), len(taps), U, D, G.ptr(yv), ldy, B, L,
                                      edge))
    torch.cuda.synchronize()
    g = ybuf.cpu().numpy()
    assert np.all(np.isnan(g[:y_off])) and np.all(np.isnan(g[y_off + B * ldy:])), "a write outside y"
    assert np.all(np.isnan(g[y_off:y_off + B * ldy].reshape(B, ldy)[:, lout:])), "a write into y's gutters"
    return yv.cpu().numpy().copy()


def _taps(rng, M):
    k = np.arange(M) - (M - 1) / 2
    return (rng.standard_normal(M) / (1.0 + np.abs(k) / 8.0)).astype(np.float32)


def _design(fin):
    from eegldm.recordings import lowpass_resample_design
    u, d, t = lowpass_resample_design(fin, 100)
    return u, d, t.astype(np.float32)


_COUNTER = [0]


def _held_to_float64(tag, U, D, taps, L, B=2, edges=(0, 1), kinds=("f32", "i16"), seed=0):
    """Every element within the bound, for every edge and input type asked for; strides and offsets change from call to call."""
    rng = np.random.default_rng(seed)
    c = (len(taps) - 1) // 2
    worst = 0.0
    for edge in edges:
        if edge and -(-c // U) > L - 1:
            continue
        for kind in kinds:
            n = _COUNTER[0] = _COUNTER[0] + 1
            if kind == "f32":
                x = (rng.standard_normal((B, L)) * (1e-3, 1.0, 1e3)[n % 3]).astype(np.float32)
                gain = offset = None
            else:                                                    # rows of different gain and offset
                x = rng.integers(-32768, 32768, (B, L)).astype(np.int16)
                gain = np.resize(np.array([400.0 / 4095, 1e-7, 3.0], np.float32), B)
                offset = np.resize(np.array([0.0488, -3.1e-5, 12.5], np.float32), B)
            kw = dict(ldx=L + n % 3, ldy=R.out_len(L, U, D) + (n + 1) % 3, x_off=n % (4 if kind == "f32" else 8), t_off=(n // 4) % 4, y_off=(n // 2) % 4)
            got = _resample(x, taps, U, D, edge, gain, offset, **kw)
            want, E = R.resample64(x, taps, U, D, edge, gain, offset), R.resample_error_bound(x, taps, U, D, edge, gain, offset)
            t = f"{tag} U={U} D={D} M={len(taps)} L={L} B={B} edge={edge} {kind} {kw}"
            assert got.shape == want.shape and np.all(np.isfinite(got)), t
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= E), f"{t}: off by {err.max():.3e}, bound {E[np.unravel_index(np.argmax(err - E), E.shape)]:.3e}"
            worst = max(worst, float((err / E).max()))
    print(f"resample_numerics: {tag}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("L", [1, 2, 38, 74, 75, 1000, 4096])
def test_case1_plain_lowpass(L):
    u, d, t = _design(100)
    assert (u, d, t.size) == (1, 1, 75)
    _held_to_float64("case 1", 1, 1, t, L, seed=L)


@pytest.mark.parametrize("L, B", [(93, 1), (93, 3), (1000, 1), (1000, 3), (100003, 1), (100003, 3)])
def test_case2_125_hz(L, B):
    u, d, t = _design(125)
    assert (u, d, t.size) == (4, 5, 367)
    _held_to_float64("case 2", u, d, t, L, B=B, seed=L + B)


@pytest.mark.parametrize("fin, ud, n_taps, L", [(128, (25, 32), 2347, 5000), (256, (25, 64), 4695, 20011), (512, (25, 128), 9387, 60013)])
def test_cases3_to_5_long_filters(fin, ud, n_taps, L):
    u, d, t = _design(fin)
    assert ((u, d), t.size) == (ud, n_taps)
    _held_to_float64(f"case {fin} Hz", u, d, t, L, seed=fin)


def test_case6_decimation_only():
    u, d, t = _design(200)
    assert (u, d) == (1, 2)
    _held_to_float64("case 6 (1, 2)", 1, 2, t, 3001, seed=6)
    _held_to_float64("case 6 (1, 5)", 1, 5, _taps(np.random.default_rng(65), 61), 2503, seed=65)


def test_case7_upsampling():
    _held_to_float64("case 7", 3, 2, _taps(np.random.default_rng(7), 31), 1001, seed=7)
    _held_to_float64("case 7 short", 3, 2, _taps(np.random.default_rng(7), 31), 7, seed=77)


def test_case8_fewer_taps_than_phases():
    taps = _taps(np.random.default_rng(8), 33)
    _held_to_float64("case 8", 64, 1, taps, 50, seed=8)
    x = np.random.default_rng(88).standard_normal((2, 50)).astype(np.float32)
    got = _resample(x, taps, 64, 1, 0)
    m = np.arange(got.shape[1])
    empty = ((16 - m) % 64) >= 33                                        # k0 = (c - m D) mod U is past the last tap
    assert empty.any() and not empty.all() and np.all(_bits(got[:, empty]) == 0), "an output without a term must be +0"
    assert np.all(_bits(_resample(x, taps, 64, 1, 1)[:, empty]) == 0)
    j0 = (m - 16 + (16 - m) % 64) // 64
    assert np.all(got[:, ~empty & (j0 < 50)] != 0) and np.all(_bits(got[:, ~empty & (j0 >= 50)]) == 0)      # the one term, inside the row or skipped


def test_case9_single_tap():
    _held_to_float64("case 9", 1, 1, np.array([0.75], np.float32), 1000, seed=9)
    x = np.random.default_rng(9).standard_normal((2, 300)).astype(np.float32)
    assert np.array_equal(_bits(_resample(x, np.ones(1, np.float32), 1, 1, 0)), _bits(x))


def test_case10_one_long_row():
    u, d, t = _design(125)
    _held_to_float64("case 10", u, d, t, 1000003, B=1, seed=10)


# The terms of an output are taken in chunks of TC = min(10240 / U - 1, 3072): a second pass over the re-staged taps and samples runs only for
# ceil(M / U) > TC.  U = 1: 3073 taps (the last chunk holds one term), 16383 taps (six chunks; under zero edges the first term of the outputs
# near the row's start lies anywhere in [0, 8191], so chunk boundaries fall before, inside and behind [lo, hi)); U = 64: 10241 taps, 161
# terms against TC = 159.
CHUNKED = {"U1_M3073": (1, 1, 3073, 4000), "U1_M16383": (1, 1, 16383, 8200), "U1_D3_M6145": (1, 3, 6145, 7001), "U64_D3_M10241": (64, 3, 10241, 500)}


@pytest.mark.parametrize("name", list(CHUNKED))
def test_chunked_terms(name):
    U, D, M, L = CHUNKED[name]
    assert -(-M // U) > min(10240 // U - 1, 3072)
    _held_to_float64(f"chunked {name}", U, D, _taps(np.random.default_rng(M), M), L, seed=M)


def test_chunked_terms_geometry_changes_no_bit():
    import gpu_util as G
    rng = np.random.default_rng(51)
    cases = [CHUNKED["U1_M16383"], CHUNKED["U64_D3_M10241"]]
    data = [(_taps(rng, M), rng.standard_normal((2, L)).astype(np.float32), rng.integers(-2048, 2048, (2, L)).astype(np.int16)) for _, _, M, L in cases]
    gn, of = np.array([0.1, 0.2], np.float32), np.array([1.0, -1.0], np.float32)

    def run():
        return [(_resample(x, t, U, D, 0), _resample(xi, t, U, D, 1, gn, of)) for (U, D, _, _), (t, x, xi) in zip(cases, data)]
    try:
        os.environ.pop("EEGLDM_RS_SEG", None); os.environ.pop("EEGLDM_RS_R", None); G.lib.eegldm_debug_reload_env()
        want = run()
        for seg, r in ((64, 1), (257, 8), (4096, 4)):
            os.environ["EEGLDM_RS_SEG"] = str(seg); os.environ["EEGLDM_RS_R"] = str(r); G.lib.eegldm_debug_reload_env()
            for (a, b), (wa, wb) in zip(run(), want):
                assert np.array_equal(_bits(a), _bits(wa)) and np.array_equal(_bits(b), _bits(wb)), (seg, r)
    finally:
        os.environ.pop("EEGLDM_RS_SEG", None); os.environ.pop("EEGLDM_RS_R", None); G.lib.eegldm_debug_reload_env()


def test_more_workgroups_than_one_grid_row():
    """Past 2^20 workgroups the grid grows a second dimension: one output per workgroup (EEGLDM_RS_SEG=1) on a row of 1 100 003 samples, and
    eegldm_epoch_stats with E = 1 on 2^21 + 5 samples."""
    import gpu_util as G
    rng = np.random.default_rng(61)
    x = rng.standard_normal((1, 1100003)).astype(np.float32)
    taps = np.array([0.25, 0.5, -0.125], np.float32)
    try:
        os.environ["EEGLDM_RS_SEG"] = "1"; G.lib.eegldm_debug_reload_env()
        got = _resample(x, taps, 1, 1, 1)
    finally:
        os.environ.pop("EEGLDM_RS_SEG", None); G.lib.eegldm_debug_reload_env()
    assert np.all(np.abs(got - R.resample64(x, taps, 1, 1, 1)) <= R.resample_error_bound(x, taps, 1, 1, 1))
    assert np.array_equal(_bits(got), _bits(_resample(x, taps, 1, 1, 1)))
    y = rng.standard_normal((1, (1 << 21) + 5)).astype(np.float32)
    st = _stats(y, 1)
    assert st.shape == (1, (1 << 21) + 5, 4)
    assert np.array_equal(_bits(st[0, :, 0]), _bits(y[0])) and np.array_equal(_bits(st[0, :, 1]), _bits(y[0])) and np.array_equal(_bits(st[0, :, 2]), _bits(y[0]))
    assert np.all(st[0, :, 3] == 0.0)


def test_every_alignment():
    """x, taps and y each 0..3 floats off a 16-byte boundary (so the 16-byte loads start at every position), int16 x at 0..7 shorts."""
    u, d, t = _design(125)
    rng = np.random.default_rng(11)
    L = 2000
    x = rng.standard_normal((2, L)).astype(np.float32)
    want = _resample(x, t, u, d, 1)
    for off in range(4):
        assert np.array_equal(_bits(_resample(x, t, u, d, 1, x_off=off, ldx=L + off)), _bits(want))
        assert np.array_equal(_bits(_resample(x, t, u, d, 1, t_off=off)), _bits(want))
        assert np.array_equal(_bits(_resample(x, t, u, d, 1, y_off=off, ldy=want.shape[1] + off)), _bits(want))
    xi = rng.integers(-2048, 2048, (2, L)).astype(np.int16)
    gn, of = np.array([0.1, 0.2], np.float32), np.array([1.0, -1.0], np.float32)
    want = _resample(xi, t, u, d, 1, gn, of)
    E = R.resample_error_bound(xi, t, u, d, 1, gn, of)
    assert np.all(np.abs(want - R.resample64(xi, t, u, d, 1, gn, of)) <= E)
    for off in range(8):
        assert np.array_equal(_bits(_resample(xi, t, u, d, 1, gn, of, x_off=off, ldx=L + off)), _bits(want)), off


# ------------------------------------------------------------------------------------------------ 2. bit-exact anchors
@pytest.mark.parametrize("M", [1, 75, 2049])
def test_equals_fir_same_bit_for_bit(M):
    import gpu_util as G
    rng = np.random.default_rng(M)
    taps = _taps(rng, M)
    for L in (75, 3072, 4096):
        for edge in (0, 1):
            if edge and (M - 1) // 2 > L - 1:
                continue
            x = rng.standard_normal((3, L)).astype(np.float32)
            xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(taps).cuda()
            y = torch.full((3, L), float("nan"), device="cuda")
            G.check(G.lib.eegldm_fir_same(G.ctx().h, G.ptr(xd), L, G.ptr(td), M, G.ptr(y), L, 3, L, edge, 0))
            assert np.array_equal(_bits(_resample(x, taps, 1, 1, edge)), _bits(y.cpu().numpy())), (M, L, edge)


def test_geometry_changes_no_bit():
    import gpu_util as G
    rng = np.random.default_rng(21)
    cases = [(_design(125), 5003), (_design(512), 30011), ((1, 1, _taps(rng, 75)), 4096), ((3, 2, _taps(rng, 31)), 700)]
    data = [(rng.standard_normal((2, L)).astype(np.float32), rng.integers(-2048, 2048, (2, L)).astype(np.int16)) for _, L in cases]
    gn, of = np.array([0.1, 0.2], np.float32), np.array([1.0, -1.0], np.float32)

    def run():
        return [(_resample(x, t, u, d, 1), _resample(xi, t, u, d, 0, gn, of)) for ((u, d, t), L), (x, xi) in zip(cases, data)]
    try:
        os.environ.pop("EEGLDM_RS_SEG", None); os.environ.pop("EEGLDM_RS_R", None); G.lib.eegldm_debug_reload_env()
        want = run()
        for seg in (64, 257, 4096):
            for r in (1, 4, 8):
                os.environ["EEGLDM_RS_SEG"] = str(seg); os.environ["EEGLDM_RS_R"] = str(r); G.lib.eegldm_debug_reload_env()
                for (a, b), (wa, wb) in zip(run(), want):
                    assert np.array_equal(_bits(a), _bits(wa)) and np.array_equal(_bits(b), _bits(wb)), (seg, r)
    finally:
        os.environ.pop("EEGLDM_RS_SEG", None); os.environ.pop("EEGLDM_RS_R", None); G.lib.eegldm_debug_reload_env()


def test_shifted_sub_row_and_repeat_runs():
    """A sub-row cut from inside a longer row n D samples in: its virtual index is shifted by n D U, so output m of the sub-row is output
    m + n U of the row.  Under edge 0 the outputs whose whole support lies inside the sub-row see the same samples under the same taps and must
    carry the same bits.  Two runs are bit-equal."""
    u, d, t = _design(125)
    c = (t.size - 1) // 2
    rng = np.random.default_rng(31)
    x = rng.standard_normal((1, 9000)).astype(np.float32)
    full = _resample(x, t, u, d, 0)
    assert np.array_equal(_bits(full), _bits(_resample(x, t, u, d, 0)))
    for n in (1, 7, 200):
        s, Ls = n * d, 3001
        sub = _resample(x[:, s:s + Ls], t, u, d, 0)
        m = np.arange(sub.shape[1])
        inside = (m * d - c >= 0) & (m * d + c <= (Ls - 1) * u)              # the whole support of sub-row output m lies inside the sub-row
        assert inside.sum() > 2000
        assert np.array_equal(_bits(sub[0, inside]), _bits(full[0, m[inside] + n * u])), n


# ------------------------------------------------------------------------------------------------ 3. non-finite samples
@pytest.mark.parametrize("U, D, M, L", [(4, 5, 367, 1500), (1, 1, 75, 600), (25, 32, 2347, 2600), (3, 2, 31, 400)])
def test_non_finite_samples_reach_exactly_their_support(U, D, M, L):
    rng = np.random.default_rng(M)
    taps = _taps(rng, M)
    for edge in (0, 1):
        for bad in (np.nan, np.inf, -np.inf):
            for idx in (0, L // 2 + 3, L - 1):
                x = rng.standard_normal((2, L)).astype(np.float32)
                x[1, idx] = bad
                got = _resample(x, taps, U, D, edge)
                mask = R.resample_support_mask(L, M, U, D, idx, edge)
                assert mask.any() and not mask.all()
                assert np.all(np.isfinite(got[0])), (edge, bad, idx)
                assert np.array_equal(~np.isfinite(got[1]), mask), (edge, bad, idx)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_y_untouched():
    import gpu_util as G
    h = G.ctx().h
    x = torch.randn(2, 300, device="cuda")
    xi = torch.zeros(2, 300, device="cuda", dtype=torch.int16)
    t = torch.randn(16400, device="cuda")
    gn = torch.ones(2, device="cuda")
    y = torch.full((2, 400), 5.0, device="cuda")
    P = G.ptr

    def off(tensor, nbytes):
        import ctypes
        return ctypes.c_void_p(tensor.data_ptr() + nbytes)

    def call(x_=P(x), ldx=300, xtype=0, g=None, o=None, t_=P(t), M=15, U=4, D=5, y_=P(y), ldy=400, B=2, L=300, edge=1, ctx=h):
        return G.lib.eegldm_resample_fir(ctx, x_, ldx, xtype, g, o, t_, M, U, D, y_, ldy, B, L, edge)
    cases = {
        "null ctx": (dict(ctx=None), "null argument"), "null x": (dict(x_=None), "null argument"), "null taps": (dict(t_=None), "null argument"),
        "null y": (dict(y_=None), "null argument"),
        "even M": (dict(M=14), "M 14 is even"), "M 0": (dict(M=0), "M 0 outside [1, 16383]"), "M 16385": (dict(M=16385), "M 16385 outside [1, 16383]"),
        "U 0": (dict(U=0), "U 0 outside [1, 64]"), "U 65": (dict(U=65), "U 65 outside [1, 64]"),
        "D 0": (dict(D=0), "D 0 outside [1, 4096]"), "D 4097": (dict(D=4097), "D 4097 outside [1, 4096]"),
        "L 0": (dict(L=0), "L 0 outside [1, 2^30]"), "L 2^30 + 1": (dict(L=(1 << 30) + 1, ldx=1 << 31, ldy=1 << 31), "outside [1, 2^30]"),
        "edge 2": (dict(edge=2), "edge 2 is neither"),
        "reflect too long": (dict(M=2401, L=300), "reflect needs ceil(c / U) <= L - 1"),
        "short ldx": (dict(ldx=299), "row strides 299 / 400 shorter than the rows 300 / 240"),
        "short ldy": (dict(ldy=239), "row strides 300 / 239 shorter than the rows 300 / 240"),
        "in place": (dict(y_=P(x)), "x == y"),
        "misaligned x": (dict(x_=off(x, 2)), "4-byte aligned"), "misaligned taps": (dict(t_=off(t, 1)), "4-byte aligned"),
        "misaligned y": (dict(y_=off(y, 2)), "4-byte aligned"), "misaligned int16 x": (dict(x_=off(xi, 1), xtype=1, g=P(gn), o=P(gn)), "2-byte aligned"),
        "int16 without gain": (dict(x_=P(xi), xtype=1, g=None, o=P(gn)), "int16 rows need gain and offset"),
        "int16 without offset": (dict(x_=P(xi), xtype=1, g=P(gn), o=None), "int16 rows need gain and offset"),
        "unknown type": (dict(xtype=2), "xtype 2 is neither 0 (fp32) nor 1 (int16)"),
        "negative B": (dict(B=-1), "B -1 outside"),
    }
    for name, (kw, msg) in cases.items():
        rc = call(**kw)
        err = G.lib.eegldm_last_error().decode()
        assert rc == -1, (name, rc)                                  # EEGLDM_ERR_INVALID
        assert err.startswith("eegldm_resample_fir: ") and msg in err, (name, err)
    assert call(M=2393, L=300) == 0                                   # ceil(1196 / 4) = 299 = L - 1: the longest reflection is accepted
    torch.cuda.synchronize()
    y.fill_(5.0)
    for name, (kw, msg) in cases.items():
        call(**kw)
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert bool((y == 5.0).all()), "a refused call (or B == 0) wrote into y"
    out = torch.full((2, 3, 4), 5.0, device="cuda")
    e = lambda **kw: G.lib.eegldm_epoch_stats(kw.get("ctx", h), kw.get("x", P(x)), kw.get("ldx", 300), 2, kw.get("L", 300), kw.get("E", 100), kw.get("out", P(out)))
    for kw, msg in [(dict(ctx=None), "null argument"), (dict(x=None), "null argument"), (dict(out=None), "null argument"), (dict(E=0), "E 0 outside [1, 12288]"),
                    (dict(E=12289), "E 12289 outside [1, 12288]"), (dict(ldx=299), "row stride 299 shorter than L 300"), (dict(x=off(x, 2)), "4-byte aligned")]:
        assert e(**kw) == -1 and msg in G.lib.eegldm_last_error().decode(), (kw, G.lib.eegldm_last_error().decode())
    assert e(L=99) == 0                                               # no whole epoch: a no-op
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


# ------------------------------------------------------------------------------------------------ 5. epoch statistics
def _stats(x, E, ld=None):
    import gpu_util as G
    x = np.asarray(x, np.float32)
    B, L = x.shape
    ld = L if ld is None else ld
    _b, xv = _carve(x, ld, 1, torch.float32)
    out = torch.full((B, L // E, 4), float("nan"), device="cuda")
    G.check(G.lib.eegldm_epoch_stats(G.ctx().h, G.ptr(xv), ld, B, L, E, G.ptr(out)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_stats(x, E, tag, **kw):
    got = _stats(x, E, **kw).astype(np.float64)
    want = R.epoch_stats64(x, E)
    bm, bs = R.epoch_stats_bounds(x, E)
    assert got.shape == want.shape, tag
    assert np.array_equal(got[..., 0], want[..., 0]) and np.array_equal(got[..., 1], want[..., 1]), tag
    em, es = np.abs(got[..., 2] - want[..., 2]), np.abs(got[..., 3] - want[..., 3])
    print(f"resample_numerics: epoch stats {tag}: mean off by {em.max():.3e} (bound {bm.min():.3e}), sd off by {es.max():.3e} (bound {bs.min():.3e})")
    assert np.all(em <= bm) and np.all(es <= bs), tag
    return got


def test_epoch_stats_against_float64():
    rng = np.random.default_rng(5)
    for k in (0.0, 30.0, 100.0):                                       # the mean in standard deviations: a one-pass variance about zero loses sd here
        x = (rng.standard_normal((3, 5 * 3000 + 1234)) * 2.5e-5 + k * 2.5e-5).astype(np.float32)     # a partial last epoch, not counted
        got = _check_stats(x, 3000, f"mean = {k:g} sd", ld=x.shape[1] + 3)
        assert got.shape == (3, 5, 4)
    x = np.full((2, 6000), 3.3e-5, np.float32)
    got = _stats(x, 3000)
    assert np.all(got[..., 3] == 0.0) and np.all(got[..., 0] == np.float32(3.3e-5)) and np.all(got[..., 2] == np.float32(3.3e-5))
    _check_stats(rng.standard_normal((2, 700)).astype(np.float32), 1, "E = 1")
    assert np.all(_stats(rng.standard_normal((2, 50)), 1)[..., 3] == 0.0)
    _check_stats((rng.standard_normal((2, 2 * 12288 + 5)) + 4.0).astype(np.float32), 12288, "E = 12288")
    x = rng.standard_normal((2, 4 * 300)).astype(np.float32)
    x[1, 650] = np.nan
    got = _stats(x, 300)
    bad = np.zeros((2, 4), bool); bad[1, 2] = True
    assert np.array_equal(np.isnan(got).all(-1), bad) and np.array_equal(np.isnan(got).any(-1), bad)
    assert np.array_equal(_bits(got[~bad]), _bits(_stats(x, 300)[~bad]))
    y = rng.standard_normal((3, 9000)).astype(np.float32)
    assert np.array_equal(_bits(_stats(y, 3000)), _bits(_stats(y, 3000)))


# ------------------------------------------------------------------------------------------------ 6. the pipeline
N2_EPOCHS = list(range(12, 20)) + list(range(24, 28))
NOISE_UV = 0.5


def _recording_125(tmp, rng, spike_epoch=None):
    """40 epochs at 125 Hz: two EEG channels (noise + a 10 Hz sine in the N2 epochs + a 40 Hz tone throughout) and a 1 Hz marker channel."""
    n = 40 * 30 * 125
    tt = np.arange(n) / 125.0
    in_n2 = np.isin((tt // 30).astype(int), N2_EPOCHS)
    chans = []
    for k in range(2):
        phys = 20.0 * np.sin(2 * np.pi * 10.0 * tt) * in_n2 + 15.0 * np.sin(2 * np.pi * 40.0 * tt + k) + NOISE_UV * rng.standard_normal(n)
        if spike_epoch is not None and k == 0:
            s = (spike_epoch * 30 + 11) * 125
            phys[s:s + 60] += 150.0
        chans.append(np.clip(np.round((phys + 200.0) / (400.0 / 4095) - 2048), -2048, 2047).astype(np.int16))
    sigs = [R.eeg_signal("EEG Fpz-Cz", chans[0], 125), R.eeg_signal("EEG Pz-Oz", chans[1], 125),
            R.eeg_signal("Event marker", rng.integers(0, 5, 40 * 30).astype(np.int16), 1, dim="")]
    psg = R.write_edf(os.path.join(tmp, "SC4011E0-PSG.edf"), sigs, record_duration="1")
    annots = [(0, 360, "Sleep stage W"), (360, 240, "Sleep stage 2"), (600, 30, "Sleep stage ?"), (630, 90, "Sleep stage 4"), (720, 120, "Sleep stage 2"),
              (840, 60, "Sleep stage R"), (900, 240, "Sleep stage W")]                # 38 epochs: the recording's last two are not covered
    R.write_edf_annotations(os.path.join(tmp, "SC4011EC-Hypnogram.edf"), annots)
    stages = np.array([0] * 12 + [2] * 8 + [-1] + [3] * 3 + [2] * 4 + [4] * 2 + [0] * 8, np.int32)
    return psg, chans, stages


def _recording_100(tmp, rng):
    n = 50 * 3000
    d = np.clip(np.round(300.0 * rng.standard_normal(n)), -2048, 2047).astype(np.int16)
    R.write_edf(os.path.join(tmp, "shhs1-200001.edf"), [R.eeg_signal("EEG", d, 3000, pmin=-0.125, pmax=0.125, dmin=-128 * 16, dmax=128 * 16 - 1, dim="mV")],
                record_duration="30")
    codes = [0] * 20 + [1, 2, 2, 3, 4, 5, 5, 6, 2, 9] + [0] * 18                       # 48 epochs of 50
    os.makedirs(os.path.join(tmp, "xml"), exist_ok=True)
    R.write_profusion(os.path.join(tmp, "xml", "shhs1-200001-profusion.xml"), codes)
    return d, np.array([0] * 20 + [1, 2, 2, 3, 3, 4, 4, -1, 2, -1] + [0] * 18, np.int32)


def _pipeline64(d, gain, offset, fin, e0, e1):
    from eegldm.recordings import lowpass_resample_design
    u, dd, t = lowpass_resample_design(fin, 100)
    t32 = t.astype(np.float32)
    g32, o32 = np.array([gain], np.float32), np.array([offset], np.float32)
    y = R.resample64(d[None], t32, u, dd, 1, g32, o32)[0]
    E = R.resample_error_bound(d[None], t32, u, dd, 1, g32, o32)[0]
    return y[e0 * 3000:e1 * 3000], E[e0 * 3000:e1 * 3000]


def test_pipeline_end_to_end(tmp_path):
    from eegldm.entry import prepare_recordings as P
    from eegldm.entry.common import WindowLoader
    rng = np.random.default_rng(42)
    src, out = str(tmp_path / "raw"), str(tmp_path / "out")
    os.makedirs(src)
    psg, chans, stages = _recording_125(src, rng)
    rc = P.main(["--edf", os.path.join(src, "*-PSG.edf"), "--hypnogram_suffix", "-Hypnogram.edf", "--channels", "EEG Fpz-Cz", "EEG Pz-Oz", "--wake_mins", "2",
                 "--units", "uV", "--output_dir", out])
    assert rc == 0
    names = ["SC4011E0-PSG-Fpz-Cz", "SC4011E0-PSG-Pz-Oz"]
    assert sorted(os.listdir(out)) == sorted([n + ".npy" for n in names] + [n + ".stages.npy" for n in names] + ["ids.csv", "prepare_report.json"])
    e0, e1 = 8, 34                                                     # sleep from epoch 12 to 29, 2 min = 4 epochs of wake on both sides
    gain = 400.0 / 4095
    offset = -200.0 + 2048 * gain
    for name, d in zip(names, chans):
        sig, st = np.load(os.path.join(out, name + ".npy")), np.load(os.path.join(out, name + ".stages.npy"))
        assert sig.dtype == np.float32 and sig.shape == (1, (e1 - e0) * 3000) and st.dtype == np.int32 and np.array_equal(st, stages[e0:e1])
        want, E = _pipeline64(d, gain, offset, 125, e0, e1)
        assert np.all(np.abs(sig[0] - want) <= E), name
        tt = (np.arange(e0 * 3000, e1 * 3000)) / 100.0
        # per epoch, by projection on 300 / 1200 whole cycles: the 10 Hz amplitude in N2 within the passband bound, the 40 Hz residue everywhere
        # within the stop-band bound (the 0.5 uV of planted noise moves such an estimate by about 6e-4 of the 20 uV sine, one sd)
        for e in range(e0 + 1, e1 - 1):
            s = slice((e - e0) * 3000, (e - e0 + 1) * 3000)
            amp = lambda f: 2.0 * np.abs(np.mean(sig[0, s].astype(np.float64) * np.exp(-2j * np.pi * f * tt[s])))
            inner = e in N2_EPOCHS and e - 1 in N2_EPOCHS and e + 1 in N2_EPOCHS
            if inner:
                assert abs(amp(10.0) / 20.0 - 1.0) <= R.PASS_TOL, (name, e, amp(10.0))
            assert amp(40.0) / 15.0 <= R.STOP_TOL, (name, e, amp(40.0))
    rows = list(csv.DictReader(open(os.path.join(out, "ids.csv"))))
    assert [r["FILE_NAME_EEG"] for r in rows] == names and all(r["recording"] == "SC4011E0-PSG" and r["subject"] == "01" and r["night"] == "1" for r in rows)
    assert [r["channel"] for r in rows] == ["EEG Fpz-Cz", "EEG Pz-Oz"] and all(r["sfreq_in"] == "125" and r["n_epochs"] == "26" for r in rows)
    rep = json.load(open(os.path.join(out, "prepare_report.json")))
    assert not rep["failed"] and [(f["U"], f["D"], f["n_taps"], f["e0"], f["e1"]) for f in rep["files"]] == [(4, 5, 367, 8, 34)] * 2
    assert rep["files"][0]["stage_counts"] == {"-1": 1, "0": 8, "2": 12, "3": 3, "4": 2} and rep["files"][0]["rejected_ptp"] == 0
    batch = next(iter(WindowLoader(out, 8, path_ids=os.path.join(out, "ids.csv"), stages=True, windows_per_recording=4)))
    assert batch["eeg"].shape == (8, 1, 3072) and batch["label"].shape == (8,) and bool(((batch["label"] >= 0) & (batch["label"] <= 4)).all())


def test_pipeline_profusion_split_rejection_and_failures(tmp_path, capsys):
    from eegldm.entry import prepare_recordings as P
    rng = np.random.default_rng(43)
    src, out = str(tmp_path / "raw"), str(tmp_path / "out")
    os.makedirs(src)
    d, stages = _recording_100(src, rng)
    for k, sid in enumerate((200002, 200003, 200004)):                 # three more subjects: copies of the first under other names
        for a, b in ((f"shhs1-200001.edf", f"shhs1-{sid}.edf"), (os.path.join("xml", "shhs1-200001-profusion.xml"), os.path.join("xml", f"shhs1-{sid}-profusion.xml"))):
            open(os.path.join(src, b), "wb").write(open(os.path.join(src, a), "rb").read())
    open(os.path.join(src, "shhs1-200009.edf"), "wb").write(open(os.path.join(src, "shhs1-200001.edf"), "rb").read()[:5000])      # corrupt: truncated
    open(os.path.join(src, "xml", "shhs1-200009-profusion.xml"), "wb").write(open(os.path.join(src, "xml", "shhs1-200001-profusion.xml"), "rb").read())
    rc = P.main(["--edf", os.path.join(src, "shhs1-*.edf"), "--profusion_dir", os.path.join(src, "xml"), "--channels", "EEG", "--wake_mins", "5",
                 "--split", "0.5,0.25,0.25", "--seed", "3", "--output_dir", out])
    assert rc == 1
    assert "FAILED" in capsys.readouterr().err
    rep = json.load(open(os.path.join(out, "prepare_report.json")))
    assert len(rep["failed"]) == 1 and "shhs1-200009.edf" in rep["failed"][0]["edf"] and "truncated" in rep["failed"][0]["error"]
    assert not os.path.exists(os.path.join(out, "shhs1-200009-EEG.npy"))
    e0, e1 = 10, 39                                                    # sleep 20..28, 5 min = 10 epochs on both sides
    sig, st = np.load(os.path.join(out, "shhs1-200001-EEG.npy")), np.load(os.path.join(out, "shhs1-200001-EEG.stages.npy"))
    assert sig.dtype == np.float32 and sig.shape == (1, (e1 - e0) * 3000) and st.dtype == np.int32 and np.array_equal(st, stages[e0:e1])
    gain = 0.25 / 4095 * 1e-3                                          # mV to volts
    want, E = _pipeline64(d, gain, (-0.125 + 2048 * (0.25 / 4095)) * 1e-3, 100, e0, e1)
    assert np.all(np.abs(sig[0] - want) <= E) and 1e-6 < np.abs(sig).max() < 1e-3
    rows = list(csv.DictReader(open(os.path.join(out, "ids.csv"))))
    assert [r["subject"] for r in rows] == ["200001", "200002", "200003", "200004"] and all(r["sfreq_in"] == "100" and r["n_epochs"] == "29" for r in rows)
    parts = [{r["subject"] for r in csv.DictReader(open(os.path.join(out, f"ids_{k}.csv")))} for k in ("train", "valid", "test")]
    assert [len(p) for p in parts] == [2, 1, 1] and len(parts[0] | parts[1] | parts[2]) == 4

    src2, out2 = str(tmp_path / "raw2"), str(tmp_path / "out2")
    os.makedirs(src2)
    _psg, _chans, stages125 = _recording_125(src2, rng, spike_epoch=15)
    rc = P.main(["--edf", os.path.join(src2, "SC4011E0-PSG.edf"), "--hypnogram_suffix", "-Hypnogram.edf", "--channels", "EEG Fpz-Cz", "EEG Pz-Oz", "--wake_mins", "2",
                 "--units", "uV", "--reject_ptp", "120", "--output_dir", out2])
    assert rc == 0
    want = stages125[8:34].copy()
    assert np.array_equal(np.load(os.path.join(out2, "SC4011E0-PSG-Pz-Oz.stages.npy")), want)
    want[15 - 8] = -2
    assert np.array_equal(np.load(os.path.join(out2, "SC4011E0-PSG-Fpz-Cz.stages.npy")), want)
    rep = json.load(open(os.path.join(out2, "prepare_report.json")))
    assert [f["rejected_ptp"] for f in rep["files"]] == [1, 0]
