"""-m gpu: the three primitives of csrc/complexity.hip and the metrics built on them.  eegldm_template_matches and eegldm_ordinal_counts EQUAL to
the numpy definitions of tests/complexity_reference.py in every integer (row lengths around every chunk edge, every m, scales that do and do not
divide L, the smallest template set, ties, every kind of tolerance, non-finite samples, the last sample, batch and launch-geometry independence,
repeat runs); eegldm_row_moments within the operation-count bound of a float64 two-pass evaluation, exact where the definition is; every refusal;
the entropies of planted signals; the entry script.  Inputs go through carved buffers filled with 7e30, so a read outside a row shows."""
import json
import math
import os
import time

import numpy as np
import pytest
import torch

import complexity_reference as R

pytestmark = pytest.mark.gpu
FILL = 7.0e30
SENT = -77
SCALES = (1, 2, 3, 7, 20, 64)
WORST = {"ratio": 0.0, "where": ""}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.time()
    yield
    print(f"\ncomplexity_numerics: worst moments error over bound {WORST['ratio']:.3f} ({WORST['where']}); "
          f"wall time of tests/test_gpu_complexity.py {time.time() - t:.1f} s")


def _carve(a, ld, off, fill=FILL):
    """Rows of `a` on the device with row stride ld (>= L), starting `off` floats into an allocation filled with `fill`."""
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


def _out(shape, dtype, fill):
    """An output table inside an allocation with two guard elements on either side -> (allocation, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 4,), fill, dtype=dtype, device="cuda")
    return buf, buf[2:2 + n].view(*shape)


def _guards_intact(buf, fill):
    g = torch.cat([buf[:2], buf[-2:]])
    return bool((g == fill).all())


def _tm(x, r, m, scale, off=1, pad=3):
    """counts (B, 2) int64 numpy of host rows x (B, L) and tolerances r (B,)."""
    import gpu_util as G
    x = np.asarray(x, np.float32)
    B, L = x.shape
    _xb, xv = _carve(x, L + pad, off)
    rv = _dev_vec(np.asarray(r, np.float32), (off + 1) % 4)
    cb, cv = _out((B, 2), torch.int64, SENT)
    G.check(G.lib.eegldm_template_matches(G.ctx().h, G.ptr(xv), L + pad, B, L, m, scale, G.ptr(rv), G.ptr(cv)))
    torch.cuda.synchronize()
    assert _guards_intact(cb, SENT), "a write outside counts"
    return cv.cpu().numpy().copy()


def _sd(x):
    v = np.asarray(x, np.float64)
    return np.sqrt(np.mean((v - v.mean(1, keepdims=True)) ** 2, 1))


def _mixed_rows(rng, B, L):
    """Even rows Gaussian, odd rows small integers (many differences equal an integer tolerance exactly)."""
    x = rng.standard_normal((B, L)).astype(np.float32)
    x[1::2] = rng.integers(0, 4, (len(x[1::2]), L)).astype(np.float32)
    return x


def _tolerances(x, shift):
    """A different kind of tolerance per row, rotated by `shift`: 0.2 sd, 1 (ties on the integer rows), 0, tiny, inf, NaN."""
    kinds = [0.2 * _sd(x), np.ones(len(x)), np.zeros(len(x)), np.full(len(x), 1e-30), np.full(len(x), np.inf), np.full(len(x), np.nan)]
    return np.array([kinds[(b + shift) % 6][b] for b in range(len(x))], np.float32)


def _combos(L):
    full = [(m, s) for s in SCALES for m in (1, 2, 3, 4)]
    if L > 100:                                                  # every scale, m rotating; every m at scale 1
        full = [(m, 1) for m in (1, 2, 3, 4)] + [(1 + i % 4, s) for i, s in enumerate(SCALES[1:])]
    return [(m, s) for m, s in full if L // s - m >= 2]


# ------------------------------------------------------------------------------------------------ 1. template matches, equal to the reference
@pytest.mark.parametrize("L", [4, 5, 63, 64, 65, 255, 256, 257, 300, 3000, 4096])
def test_template_counts_equal_reference(L):
    rng = np.random.default_rng(L)
    B = 5 if L < 1000 else 3
    x = _mixed_rows(rng, B, L)
    combos = _combos(L)
    assert combos and (L > 5 or any(L // s - m == 2 for m, s in combos))          # L = 4, 5 hold the smallest template set
    for i, (m, s) in enumerate(combos):
        r = _tolerances(x, i)
        got, want = _tm(x, r, m, s, off=i % 4), R.template_counts_rows(x, m, s, r)
        assert np.array_equal(got, want), f"L {L} m {m} scale {s} r {r.tolist()}: {got.tolist()} want {want.tolist()}"


@pytest.fixture(scope="module")
def batch130():
    rng = np.random.default_rng(130)
    x = _mixed_rows(rng, 130, 300)
    r = _tolerances(x, 0)
    return x, r, R.template_counts_rows(x, 2, 1, r), R.template_counts_rows(x, 3, 2, r)


def test_template_counts_batch_130(batch130):
    """130 rows against the reference; a row alone gives what it gives inside the batch; a second run gives the same."""
    x, r, want21, want32 = batch130
    got = _tm(x, r, 2, 1)
    assert np.array_equal(got, want21) and np.array_equal(_tm(x, r, 3, 2), want32)
    assert np.array_equal(_tm(x, r, 2, 1, off=2, pad=9), got)
    for b in (0, 1, 77, 129):
        assert np.array_equal(_tm(x[b:b + 1], r[b:b + 1], 2, 1), got[b:b + 1]), b
    # enough rows for the rule to give every row one four-wave workgroup (two workgroups per CU from the rows alone)
    reps = (2 * torch.cuda.get_device_properties(0).multi_processor_count + 129) // 130
    assert np.array_equal(_tm(np.tile(x, (reps, 1)), np.tile(r, reps), 2, 1), np.tile(want21, (reps, 1)))


def test_template_counts_do_not_depend_on_the_launch_geometry():
    import gpu_util as G
    rng = np.random.default_rng(7)
    x = _mixed_rows(rng, 2, 3000)
    r = np.array([0.2 * _sd(x)[0], 1.0], np.float32)
    want = R.template_counts_rows(x, 2, 1, r)
    try:
        for waves, split in ((4, 1), (4, 3), (4, 32), (1, 1), (1, 5), (1, 32)):
            os.environ["EEGLDM_TM_WAVES"], os.environ["EEGLDM_TM_SPLIT"] = str(waves), str(split)
            G.lib.eegldm_debug_reload_env()
            assert np.array_equal(_tm(x, r, 2, 1), want), (waves, split)
    finally:
        os.environ.pop("EEGLDM_TM_WAVES", None); os.environ.pop("EEGLDM_TM_SPLIT", None)
        G.lib.eegldm_debug_reload_env()
    assert np.array_equal(_tm(x, r, 2, 1), want)


def test_template_counts_largest_count():
    """An all-equal row of 4096 samples: every pair of the N - m templates matches at both lengths."""
    x = np.full((1, 4096), -3.25, np.float32)
    for m, s, r in ((2, 1, 0.0), (1, 1, np.inf), (4, 1, 1e-30), (2, 3, 0.0)):
        t = 4096 // s - m
        assert _tm(x, [r], m, s).tolist() == [[t * (t - 1) // 2, t * (t - 1) // 2]], (m, s, r)
    assert _tm(x, [np.nan], 2, 1).tolist() == [[0, 0]] and _tm(x, [-1.0], 2, 1).tolist() == [[0, 0]]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_template_counts_non_finite_samples(bad):
    """A NaN, +inf or -inf at the first, the last and an interior sample: equal to the reference (which tests/test_complexity_cpu.py holds to the
    double loop on such rows), so only the pairs whose templates hold the sample change; the clean rows of the batch keep their counts."""
    rng = np.random.default_rng(11)
    L = 300
    base = _mixed_rows(rng, 2, L)
    rows, where = [base[0], base[1]], [None, None]
    for idx in (0, L - 1, 137):
        for b in (0, 1):
            v = base[b].copy(); v[idx] = bad
            rows.append(v); where.append(idx)
    x = np.stack(rows)
    clean = _tm(base, [0.2 * _sd(base)[0], 1.0], 2, 1)
    for r_int in (1.0, np.inf):
        r = np.array([0.2 * _sd(base)[0], r_int] * 4, np.float32)
        for m, s in ((2, 1), (3, 1), (1, 2)):
            got, want = _tm(x, r, m, s), R.template_counts_rows(x, m, s, r)
            assert np.array_equal(got, want), (bad, r_int, m, s, got.tolist(), want.tolist())
        got = _tm(x, r, 2, 1)
        if r_int == 1.0:
            assert np.array_equal(got[:2], clean)
            assert np.all(got[2:] <= np.tile(clean, (3, 1))) and np.all(got[3::2, 1] < clean[1, 1])       # (the integer rows have matches at every sample)
            # the last sample enters A only: B is the clean row's
            assert np.array_equal(got[4:6, 0], clean[:, 0])


def test_template_counts_last_sample_enters_a_only():
    rng = np.random.default_rng(12)
    x = rng.integers(0, 3, (4, 257)).astype(np.float32)
    y = x.copy(); y[:, -1] = 50.0
    r = np.ones(4, np.float32)
    for m in (1, 2, 3, 4):
        a, b = _tm(x, r, m, 1), _tm(y, r, m, 1)
        assert np.array_equal(a, R.template_counts_rows(x, m, 1, r)) and np.array_equal(b, R.template_counts_rows(y, m, 1, r))
        assert np.array_equal(a[:, 0], b[:, 0]) and np.all(b[:, 1] < a[:, 1]), m
    # coarse-grained: the samples past N * scale are not part of the row's result
    z = x.copy(); z[:, 255:] = 1e30
    assert np.array_equal(_tm(x, r, 2, 3), _tm(z, r, 2, 3))


# ------------------------------------------------------------------------------------------------ 2. ordinal patterns, equal to the reference
def _ordinal(x, order, delay, off=1, pad=5):
    import gpu_util as G
    x = np.asarray(x, np.float32)
    B, L = x.shape
    _xb, xv = _carve(x, L + pad, off)
    cb, cv = _out((B, math.factorial(order)), torch.int32, SENT)
    sb, sv = _out((B,), torch.int32, SENT)
    G.check(G.lib.eegldm_ordinal_counts(G.ctx().h, G.ptr(xv), L + pad, B, L, order, delay, G.ptr(cv), G.ptr(sv)))
    torch.cuda.synchronize()
    assert _guards_intact(cb, SENT) and _guards_intact(sb, SENT), "a write outside the tables"
    return cv.cpu().numpy().copy(), sv.cpu().numpy().copy()


def _ordinal_rows(rng, L):
    """Gaussian, tied small integers, plateaus, signed zeros among a few values, and a row with non-finite samples."""
    x = rng.standard_normal((6, L)).astype(np.float32)
    x[1] = rng.integers(0, 3, L)
    x[2] = np.repeat(rng.standard_normal((L + 6) // 7), 7)[:L]
    x[3] = np.array([0.0, -0.0, 1.0, -1.0], np.float32)[rng.choice(4, L, p=[0.4, 0.4, 0.1, 0.1])]
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        x[4, (k * 97 + L // 2) % L] = v
    x[4, 0] = np.nan; x[4, L - 1] = np.inf
    x[5] = np.arange(L)[::-1]
    return x


@pytest.mark.parametrize("L", [7, 64, 301, 3000, 4096])
def test_ordinal_counts_equal_reference(L):
    rng = np.random.default_rng(L)
    x = _ordinal_rows(rng, L)
    done = 0
    for order in (2, 3, 4, 5, 6):
        for delay in (1, 2, 7, 100):
            if (order - 1) * delay >= L:
                continue
            got, want = _ordinal(x, order, delay, off=(order + delay) % 4), R.ordinal_counts(x, order, delay)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (L, order, delay)
            assert np.all(got[0].sum(1) + got[1] == L - (order - 1) * delay)
            assert got[0][5, -1] == L - (order - 1) * delay and got[1][4] > 0
            done += 1
    assert done >= 6


@pytest.mark.parametrize("order", [2, 3, 4, 5, 6])
def test_ordinal_counts_exactly_one_position(order):
    rng = np.random.default_rng(order)
    for delay in (1, 2, 7, 100):
        L = (order - 1) * delay + 1
        x = _ordinal_rows(rng, max(L, 7))[:, :L]
        x[4] = rng.standard_normal(L); x[4, 0] = np.nan
        got, want = _ordinal(x, order, delay), R.ordinal_counts(x, order, delay)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (order, delay)
        assert np.all(got[0].sum(1) + got[1] == 1) and got[1][4] == 1
    big = _ordinal_rows(rng, 300)
    assert all(np.array_equal(a, b) for a, b in zip(_ordinal(big, order, 3), _ordinal(big, order, 3)))
    alone = _ordinal(big[2:3], order, 3)
    assert np.array_equal(alone[0], _ordinal(big, order, 3)[0][2:3])


# ------------------------------------------------------------------------------------------------ 3. moments within the float64 bound
def _moments(x, off=1, pad=3):
    import gpu_util as G
    x = np.asarray(x, np.float32)
    B, L = x.shape
    _xb, xv = _carve(x, L + pad, off)
    ob, ov = _out((B, 8), torch.float64, -77.5)
    G.check(G.lib.eegldm_row_moments(G.ctx().h, G.ptr(xv), L + pad, B, L, G.ptr(ov)))
    torch.cuda.synchronize()
    assert _guards_intact(ob, -77.5), "a write outside out"
    return ov.cpu().numpy().copy()


@pytest.mark.parametrize("L", [1, 2, 3, 64, 3000, 4096])
def test_moments_within_the_float64_bound(L):
    rng = np.random.default_rng(L)
    rows = [((mean_sd + rng.standard_normal(L)) * mag).astype(np.float32) for mean_sd in (0.0, 30.0, 100.0) for mag in (1e-3, 1.0, 1e3)]
    x = np.stack(rows)
    got, want, bound = _moments(x, off=L % 4), R.row_moments(x), R.moments_bound(x)
    assert L < 2 or R.sign_changes_safe(x).all()
    assert np.array_equal(got[:, 5:], want[:, 5:]), "sign_changes, min, max are exact"
    err = np.abs(got[:, :5] - want[:, :5])
    assert np.all(err[bound[:, :5] == 0] == 0)
    ratio = np.where(bound[:, :5] > 0, err / np.where(bound[:, :5] > 0, bound[:, :5], 1.0), 0.0)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"complexity_numerics: moments L {L}: worst error over bound {ratio.max():.3f} ({R.MOMENT_FIELDS[i[1]]}, row {i[0]})")
    if ratio.max() > WORST["ratio"]:
        WORST.update(ratio=float(ratio.max()), where=f"L {L} {R.MOMENT_FIELDS[i[1]]}")
    assert np.all(err <= bound[:, :5]), (L, i, err[i], bound[:, :5][i])
    # the rows of a batch do not know of each other, and a second run repeats the bits
    again = _moments(x, off=2, pad=11)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    assert np.array_equal(_moments(x[4:5]).view(np.int64), got[4:5].view(np.int64))


@pytest.mark.parametrize("L", [6, 64, 3000, 4096])
def test_moments_of_small_integers_are_exact(L):
    rng = np.random.default_rng(L)
    x = np.stack([R.integer_row(rng, L) for _ in range(4)])
    got, want = _moments(x), R.row_moments(x)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got - want).tolist()
    assert np.all(got[:, 0] == 0) and np.array_equal(got[:, 1], np.sum(x.astype(np.float64) ** 2, 1))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_moments_non_finite_samples(bad):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 300)).astype(np.float32)
    clean = _moments(x)
    for idx in (0, 150, 299):
        y = x.copy(); y[1, idx] = bad
        got, want = _moments(y), R.row_moments(y)
        assert np.array_equal(got[[0, 2]].view(np.int64), clean[[0, 2]].view(np.int64))
        assert np.array_equal(np.isnan(got[1]), np.isnan(want[1])) and np.isnan(got[1, 1]) and np.isnan(got[1, 2])
        fin = ~np.isnan(want[1])
        assert np.array_equal(got[1][fin], want[1][fin]), (bad, idx, got[1], want[1])


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals():
    import gpu_util as G
    h, lib = G.ctx().h, G.lib
    x = torch.zeros(4, 304, device="cuda")
    r = torch.ones(4, device="cuda")
    mom = torch.full((4, 8), -77.5, dtype=torch.float64, device="cuda")
    cnt = torch.full((4, 720), SENT, dtype=torch.int32, device="cuda")
    skp = torch.full((4,), SENT, dtype=torch.int32, device="cuda")
    tmc = torch.full((4, 2), SENT, dtype=torch.int64, device="cuda")
    P = G.ptr
    odd = x.view(-1)[1:].data_ptr() - 2                              # a float pointer that is not 4-byte aligned
    cases = {
        "moments null ctx": lambda: lib.eegldm_row_moments(None, P(x), 304, 4, 300, P(mom)),
        "moments null x": lambda: lib.eegldm_row_moments(h, None, 304, 4, 300, P(mom)),
        "moments null out": lambda: lib.eegldm_row_moments(h, P(x), 304, 4, 300, None),
        "moments L 0": lambda: lib.eegldm_row_moments(h, P(x), 304, 4, 0, P(mom)),
        "moments L 4097": lambda: lib.eegldm_row_moments(h, P(x), 5000, 4, 4097, P(mom)),
        "moments ldx": lambda: lib.eegldm_row_moments(h, P(x), 299, 4, 300, P(mom)),
        "moments B < 0": lambda: lib.eegldm_row_moments(h, P(x), 304, -1, 300, P(mom)),
        "moments x alignment": lambda: lib.eegldm_row_moments(h, odd, 304, 1, 300, P(mom)),
        "moments out alignment": lambda: lib.eegldm_row_moments(h, P(x), 304, 3, 300, mom.data_ptr() + 4),
        "ordinal null ctx": lambda: lib.eegldm_ordinal_counts(None, P(x), 304, 4, 300, 3, 1, P(cnt), P(skp)),
        "ordinal null x": lambda: lib.eegldm_ordinal_counts(h, None, 304, 4, 300, 3, 1, P(cnt), P(skp)),
        "ordinal null counts": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 3, 1, None, P(skp)),
        "ordinal null skipped": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 3, 1, P(cnt), None),
        "ordinal order 1": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 1, 1, P(cnt), P(skp)),
        "ordinal order 7": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 7, 1, P(cnt), P(skp)),
        "ordinal delay 0": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 3, 0, P(cnt), P(skp)),
        "ordinal delay -3": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 3, -3, P(cnt), P(skp)),
        "ordinal no position": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 4, 100, P(cnt), P(skp)),
        "ordinal delay overflow": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 6, 0x7fffffff, P(cnt), P(skp)),
        "ordinal L 0": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, 4, 0, 3, 1, P(cnt), P(skp)),
        "ordinal L 4097": lambda: lib.eegldm_ordinal_counts(h, P(x), 5000, 4, 4097, 3, 1, P(cnt), P(skp)),
        "ordinal ldx": lambda: lib.eegldm_ordinal_counts(h, P(x), 299, 4, 300, 3, 1, P(cnt), P(skp)),
        "ordinal B < 0": lambda: lib.eegldm_ordinal_counts(h, P(x), 304, -1, 300, 3, 1, P(cnt), P(skp)),
        "ordinal alignment": lambda: lib.eegldm_ordinal_counts(h, odd, 304, 1, 300, 3, 1, P(cnt), P(skp)),
        "tm null ctx": lambda: lib.eegldm_template_matches(None, P(x), 304, 4, 300, 2, 1, P(r), P(tmc)),
        "tm null x": lambda: lib.eegldm_template_matches(h, None, 304, 4, 300, 2, 1, P(r), P(tmc)),
        "tm null r": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 300, 2, 1, None, P(tmc)),
        "tm null counts": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 300, 2, 1, P(r), None),
        "tm m 0": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 300, 0, 1, P(r), P(tmc)),
        "tm m 5": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 300, 5, 1, P(r), P(tmc)),
        "tm scale 0": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 300, 2, 0, P(r), P(tmc)),
        "tm scale 65": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 300, 2, 65, P(r), P(tmc)),
        "tm one template": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 300, 4, 60, P(r), P(tmc)),
        "tm L 3 m 2": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 3, 2, 1, P(r), P(tmc)),
        "tm L 0": lambda: lib.eegldm_template_matches(h, P(x), 304, 4, 0, 1, 1, P(r), P(tmc)),
        "tm L 4097": lambda: lib.eegldm_template_matches(h, P(x), 5000, 4, 4097, 2, 1, P(r), P(tmc)),
        "tm ldx": lambda: lib.eegldm_template_matches(h, P(x), 299, 4, 300, 2, 1, P(r), P(tmc)),
        "tm B < 0": lambda: lib.eegldm_template_matches(h, P(x), 304, -1, 300, 2, 1, P(r), P(tmc)),
        "tm x alignment": lambda: lib.eegldm_template_matches(h, odd, 304, 1, 300, 2, 1, P(r), P(tmc)),
        "tm counts alignment": lambda: lib.eegldm_template_matches(h, P(x), 304, 3, 300, 2, 1, P(r), tmc.data_ptr() + 4),
    }
    for name, call in cases.items():
        assert call() != 0, name
        assert len(lib.eegldm_last_error()) > 0
    torch.cuda.synchronize()
    assert bool((mom == -77.5).all()) and bool((cnt == SENT).all()) and bool((skp == SENT).all()) and bool((tmc == SENT).all()), "a refused call wrote"
    # B == 0: successful no-ops
    assert lib.eegldm_row_moments(h, P(x), 304, 0, 300, P(mom)) == 0 and lib.eegldm_ordinal_counts(h, P(x), 304, 0, 300, 3, 1, P(cnt), P(skp)) == 0
    assert lib.eegldm_template_matches(h, P(x), 304, 0, 300, 2, 1, P(r), P(tmc)) == 0
    torch.cuda.synchronize()
    assert bool((mom == -77.5).all()) and bool((cnt == SENT).all()) and bool((skp == SENT).all()) and bool((tmc == SENT).all())
    # the edges of the accepted ranges
    assert lib.eegldm_template_matches(h, P(x), 304, 4, 300, 2, 64, P(r), P(tmc)) == 0                 # N - m = 4 - 2
    assert lib.eegldm_ordinal_counts(h, P(x), 304, 4, 300, 4, 99, P(cnt), P(skp)) == 0                 # (order - 1) delay = L - 3
    torch.cuda.synchronize()
    assert tmc.tolist() == [[1, 1]] * 4 and bool((skp == 0).all()) and cnt.view(-1)[:24].tolist() == [3] + [0] * 23


# ------------------------------------------------------------------------------------------------ 5. properties on planted signals
@pytest.mark.parametrize("seed", R.PLANT_SEEDS)
def test_entropies_of_planted_signals(seed):
    """L = 3000.  For white Gaussian noise the samples of a template are independent, so A / B estimates P(|y_i - y_j| <= r) = erf(r / (2 sd_y)):
    with r = 0.2 sd of the raw window and sd_y = sd / sqrt(scale) after coarse-graining, SampEn = -ln erf(0.1 sqrt(scale)) = 2.185, 1.393, 0.749
    at scales 1, 5, 20.  A is about 6400, 2700, 1100 pairs there; with pairs sharing samples counted as half as many independent ones the
    relative sd of A is 2 / sqrt(A) = 2.5 %, 3.8 %, 6 %, and the bands are three to four of those: 0.1, 0.15, 0.2.  A 1-Hz sine at 100 Hz is
    the issue's 0.16, held to 0.10 .. 0.25 (the reference gives 0.161 .. 0.164 over the seeds)."""
    from eegldm import metrics as M
    noise, sine = R.white_noise(seed), R.sine(seed)
    both = torch.from_numpy(np.concatenate([noise, sine]))[:, None, :]
    se = M.sample_entropy(both, m=2, r=0.2, r_mode="sd", scales=(1, 5, 20))
    print(f"complexity_numerics: seed {seed}: SampEn noise {se[0].round(3).tolist()}, sine {se[1].round(3).tolist()}")
    assert se.shape == (2, 3) and np.all(np.isfinite(se))
    for got, scale, band in zip(se[0], (1, 5, 20), (0.1, 0.15, 0.2)):
        assert abs(got - (-math.log(math.erf(0.1 * math.sqrt(scale))))) < band, (scale, got)
    assert se[0, 0] > se[0, 1] > se[0, 2]
    assert 0.10 < se[1, 0] < 0.25 and se[1, 0] < se[0, 0] - 1.5
    # A > 0 for noise at every m <= 4: every entropy read here is finite; the counts through the Python layer equal the reference
    r_abs = float(np.float32(0.2 * _sd(noise)[0]))
    for m in (1, 2, 3, 4):
        c = M.template_match_counts(both[:1], m=m, r=r_abs)
        assert c.dtype == np.int64 and c[0, 1] > 0 and np.array_equal(c, R.template_counts_rows(noise, m, 1, [r_abs]))
    assert abs(M.sample_entropy(both[:1], m=2, r=r_abs, r_mode="abs")[0, 0] - se[0, 0]) < 0.02
    pe = M.permutation_entropy(both, order=3)
    assert pe[0] > 0.99 and pe[1] < 0.6
    assert abs(M.permutation_entropy(both, order=3, normalize=False)[0] - pe[0] * math.log(6)) < 1e-12
    assert np.allclose(pe, R.permutation_entropy(R.ordinal_counts(np.concatenate([noise, sine]), 3, 1)[0]), rtol=0, atol=1e-14)
    h = M.hjorth(both)
    assert abs(h[1, 1] / (2 * math.sin(math.pi / 100)) - 1) < 2 / 3000 and abs(h[1, 2] - 1) < 4 / 3000 and h[0, 1] > 1.3 and abs(h[0, 0] - 1) < 0.1


def test_python_layer_shapes_and_crop():
    from eegldm import metrics as M
    rng = np.random.default_rng(5)
    w = rng.standard_normal((3, 1, 3072)).astype(np.float32)
    w[:, :, :36] = 0; w[:, :, -36:] = 0
    inner = w[:, 0, 36:-36]
    mom = M.row_moments(torch.from_numpy(w))
    assert mom.shape == (3, 8) and np.array_equal(mom, M.row_moments(inner)) and np.array_equal(mom[:, 5:], R.row_moments(inner)[:, 5:])
    f, names = M.complexity_features(torch.from_numpy(w), orders=(3, 4), scales=(1, 10))
    assert f.shape == (3, 9) and f.dtype == np.float64 and names == M.complexity_feature_names((3, 4), (1, 10)) and np.all(np.isfinite(f))
    assert np.array_equal(f[:, :3], M.hjorth(inner)) and np.array_equal(f[:, 5], M.permutation_entropy(inner, 3))
    assert np.array_equal(f[:, 7:], M.sample_entropy(inner, scales=(1, 10)))
    assert M.row_moments(torch.zeros(0, 300)).shape == (0, 8) and M.sample_entropy(torch.zeros(0, 300), scales=(1, 2)).shape == (0, 2)
    c, s = M.ordinal_counts(inner, order=4, delay=2)
    assert c.shape == (3, 24) and s.shape == (3,) and np.array_equal(c, R.ordinal_counts(inner, 4, 2)[0])
    # a constant window: every pair matches under r = 0.2 sd = 0, SampEn 0; Hjorth mobility is 0 / 0
    const = torch.full((1, 500), 2.5)
    assert M.sample_entropy(const)[0, 0] == 0.0 and np.isnan(M.hjorth(const)[0, 1])


# ------------------------------------------------------------------------------------------------ 6. the entry script
def test_complexity_script_round_trip(tmp_path):
    from eegldm.entry import complexity as S
    real = np.concatenate([R.white_noise(0, 8), R.sine(0), R.sine(1, 2.0), R.sine(2, 0.5), R.sine(3, 5.0)])[:, None, :]       # (12, 1, 3000)
    syn = np.concatenate([R.white_noise(1, 4), R.sine(4), R.sine(5, 3.0)])[:, None, :]                                        # (6, 1, 3000)
    os.makedirs(tmp_path / "syn")
    np.save(tmp_path / "syn" / "sample_0.npy", syn[:2]); np.save(tmp_path / "syn" / "sample_1.npy", syn[2:])
    np.save(tmp_path / "syn" / "sample_0_label.npy", np.array([0, 0])); np.save(tmp_path / "syn" / "sample_1_label.npy", np.array([0, 0, 3, 3]))
    np.save(tmp_path / "hold.npy", real)
    out = str(tmp_path / "complexity.json")
    argv = ["--samples", str(tmp_path / "syn" / "sample_*.npy"), "--holdout_npy", str(tmp_path / "hold.npy"), "--orders", "3", "4", "--scales", "1", "5",
            "--seed", "1", "--output", out]
    res = S.main(S.parse_args(argv + ["--labels_from_samples", "--chunk", "5"]))
    with open(out) as f:
        back = json.load(f)
    assert back == json.loads(json.dumps(res))
    names = ["activity", "mobility", "complexity", "sign_change_rate", "line_length_per_sample", "perm_entropy_o3", "perm_entropy_o4",
             "sample_entropy_s1", "sample_entropy_s5"]
    assert back["features"] == names and back["n_real"] == 12 and back["n_synthetic"] == 6 and len(back["files"]) == 2
    assert back["window_samples"] == {"real": 3000, "synthetic": 3000} and back["args"]["m"] == 2 and back["args"]["r"] == 0.2
    for side, n in (("real", 12), ("synthetic", 6)):
        assert back[side]["n_windows"] == n
        for name in names:
            b = back[side][name]
            assert b["n"] + b["n_nonfinite"] == n and b["n"] > 0 and b["q25"] <= b["median"] <= b["q75"]
    assert "per_stage" not in back["real"]
    st = back["synthetic"]["per_stage"]
    assert sorted(st) == ["0", "3"] and st["0"]["n_windows"] == 4 and st["3"]["n_windows"] == 2
    assert st["0"]["sample_entropy_s1"]["mean"] > 2.0 > 0.5 > st["3"]["sample_entropy_s1"]["mean"]
    for block in ("real_vs_synthetic", "real_vs_real"):
        for name in names:
            v = back[block][name]
            assert 0.0 <= v["ks"] <= 1.0 and v["wasserstein"] >= 0.0 and v["n_real"] > 0 and v["n_synthetic"] > 0 and v["n_real_nonfinite"] == 0
    assert back["real_vs_real"]["n"] == [6, 6]
    assert "Nobody has measured" in back["caveat"] and "not evidence of realism" in back["caveat"]
    # chunking changes nothing
    res2 = S.main(S.parse_args(argv))
    assert res2["real"] == res["real"] and res2["real_vs_synthetic"] == res["real_vs_synthetic"]
    assert res2["synthetic"] == {k: v for k, v in res["synthetic"].items() if k != "per_stage"}
