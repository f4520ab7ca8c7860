"""-m gpu: the nearest-neighbour search of csrc/knn.hip against a float64 evaluation of the same definition (tests/knn_reference.py) --
order statistics within the operation-count bound E, the bit-exact anchors (chunking, repeat runs, ties, self exclusion, NaN rows,
short corpora), the helpers, precision / recall / coverage, and the memorisation audit with planted copies."""
import json
import os

import numpy as np
import pytest
import torch

import knn_reference as R

pytestmark = pytest.mark.gpu

INF = float("inf")


def _carve(a, ld, off):
    """Rows of the float64/32 array `a` on the device with row stride ld (> D), starting `off` floats into the allocation."""
    n, d = a.shape
    buf = torch.full((off + max(n, 1) * ld + 4,), 7.0e30, device="cuda")       # a read outside the rows shows in every score
    view = buf[off:off + max(n, 1) * ld].view(max(n, 1), ld)[:n, :d]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    return buf, view


def _state(nq, k, off=0):
    bs = torch.full((off + nq * k,), INF, device="cuda")
    bi = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
    return bs, bs[off:].view(nq, k), bi


def _update(q, x, xbias, k, best_s, best_i, index_base=0, self_base=-1, D=None):
    import gpu_util as G
    c = G.ctx()
    nq, nc = q.shape[0], x.shape[0]
    D = q.shape[1] if D is None else D
    G.check(G.lib.eegldm_knn_update(c.h, G.ptr(q), q.stride(0), G.ptr(x) if nc else G.ptr(q), x.stride(0) if nc else D, G.ptr(xbias), nq, nc, D, k,
                                    index_base, self_base, G.ptr(best_s), G.ptr(best_i)))


def _sqnorm(x):
    import gpu_util as G
    out = torch.empty(x.shape[0], device="cuda")
    G.check(G.lib.eegldm_rows_sqnorm(G.ctx().h, G.ptr(x), x.stride(0), x.shape[0], x.shape[1], G.ptr(out)))
    return out


def _search(q, x, k, chunks=None, xbias="sqnorm", self_base=-1):
    """One-shot (chunks None) or chunked over the given row boundaries -> (scores, indices) numpy."""
    _b, bs, bi = _state(q.shape[0], k)
    xb = _sqnorm(x) if isinstance(xbias, str) else xbias
    bounds = [0, x.shape[0]] if chunks is None else chunks
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        _update(q, x[lo:hi], None if xb is None else xb[lo:hi], k, bs, bi, index_base=lo, self_base=self_base)
    torch.cuda.synchronize()
    return bs.cpu().numpy().copy(), bi.cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------ 1. search against float64
NQS, NCS, KS = (1, 5, 127, 128, 129, 257), (1, "k-1", 127, 129, 1000), (1, 3, 16, 32)


@pytest.mark.parametrize("D", [1, 3, 16, 17, 302, 3000])
def test_search_against_float64(D):
    """The r-th returned score lies within max_j E(i, j) of the r-th smallest float64 score, the float64 score of the r-th returned index
    within twice that (order statistics are 1-Lipschitz under a sup-norm perturbation), every list is non-decreasing with distinct
    indices.  E and c(D): knn_reference.error_bound / c_of.  Row strides > D, every pointer 0..3 floats off its allocation."""
    combos = [(129, 257)] if D == 3000 else [(nq, nc) for nq in NQS for nc in NCS]
    n = 0
    worst = 0.0
    for mag in (1e-3, 1.0, 1e3):
        rng = np.random.default_rng(1000 * D + int(np.log10(mag)) + 7)
        Q = (rng.standard_normal((max(c[0] for c in combos), D)) * mag).astype(np.float32)
        X = (rng.standard_normal((1000 if D != 3000 else 257, D)) * mag).astype(np.float32)
        xb64 = (X.astype(np.float64) ** 2).sum(1)
        S = R.scores64(Q, X, xb64)
        E = R.error_bound(Q, X)
        ref_cache = {}
        for nq, nc_spec in combos:
            for k in KS:
                nc = k - 1 if nc_spec == "k-1" else nc_spec
                n += 1
                oq, ox, ob, os_ = n % 4, (n // 4) % 4, (n // 16) % 4, (n // 64) % 4
                _qb, q = _carve(Q[:nq], D + 1 + n % 3, oq)
                _xb, x = _carve(X[:nc], D + 2 + n % 5, ox)
                xbuf = torch.zeros(ob + nc + 4, device="cuda")
                xbias = xbuf[ob:ob + nc]
                if nc:
                    import gpu_util as G
                    G.check(G.lib.eegldm_rows_sqnorm(G.ctx().h, G.ptr(x), x.stride(0), nc, D, G.ptr(xbias)))
                _sb, bs, bi = _state(nq, k, os_)
                _update(q, x, xbias if nc else None, k, bs, bi, D=D)
                got_s, got_i = bs.cpu().numpy().astype(np.float64), bi.cpu().numpy()
                if (nc, k) not in ref_cache:
                    ref_cache[(nc, k)] = R.topk64(S[:, :nc], k)
                ref_s, _ri = (a[:nq] for a in ref_cache[(nc, k)])
                m = min(k, nc)
                tag = f"D={D} mag={mag} Nq={nq} Nc={nc} k={k}"
                assert np.all(np.isinf(got_s[:, m:])) and np.all(got_i[:, m:] == -1), tag
                if m == 0:
                    continue
                emax = E[:nq, :nc].max(1)[:, None]
                assert np.all(got_i[:, :m] >= 0) and np.all(got_i[:, :m] < nc), tag
                err = np.abs(got_s[:, :m] - ref_s[:, :m])
                assert np.all(err <= emax), f"{tag}: score off by {err.max():.3e}, bound {emax.max():.3e}"
                worst = max(worst, float((err / emax).max()))
                s_of_idx = np.take_along_axis(S[:nq, :nc], got_i[:, :m], 1)
                assert np.all(np.abs(s_of_idx - ref_s[:, :m]) <= 2 * emax), tag
                assert np.all(np.diff(got_s[:, :m], axis=1) >= 0), tag
                srt = np.sort(got_i[:, :m], axis=1)
                assert np.all(np.diff(srt, axis=1) > 0), tag
    print(f"D={D}: {n} cases, worst score error {worst:.3f} of E")


# ------------------------------------------------------------------------------------------------ 2. bit-exact anchors
@pytest.fixture(scope="module")
def anchor():
    rng = np.random.default_rng(5)
    Q = rng.standard_normal((129, 33)).astype(np.float32)
    X = rng.standard_normal((1000, 33)).astype(np.float32)
    X[[17, 400, 401, 999]] = X[3]                   # duplicated corpus rows
    _a, q = _carve(Q, 40, 1)
    _b, x = _carve(X, 37, 2)
    return {"Q": Q, "X": X, "q": q, "x": x, "keep": (_a, _b), "one": {k: _search(q, x, k) for k in (3, 32)}}


@pytest.mark.parametrize("k", [3, 32])
@pytest.mark.parametrize("split", ["1", "100", "128", "uneven"])
def test_chunking_does_not_change_a_bit(anchor, k, split):
    n = 1000
    bounds = {"1": list(range(n + 1)), "100": list(range(0, n + 1, 100)), "128": list(range(0, n, 128)) + [n],
              "uneven": [0, 1, 130, 131, 517, 901, n]}[split]
    s, i = _search(anchor["q"], anchor["x"], k, chunks=bounds)
    s0, i0 = anchor["one"][k]
    assert np.array_equal(s.view(np.int32), s0.view(np.int32)) and np.array_equal(i, i0)


def test_two_runs_agree_and_ties_come_lowest_index_first(anchor):
    for k in (3, 32):
        s, i = _search(anchor["q"], anchor["x"], k)
        assert np.array_equal(s.view(np.int32), anchor["one"][k][0].view(np.int32)) and np.array_equal(i, anchor["one"][k][1])
    s, i = anchor["one"][32]
    dup = [3, 17, 400, 401, 999]
    # a query that is the duplicated row: its five copies tie bit for bit and lead the list in index order
    _a, q = _carve(anchor["X"][3:4], 35, 3)
    s1, i1 = _search(q, anchor["x"], 8)
    assert list(i1[0, :5]) == dup and len(set(s1[0, :5].view(np.int32).tolist())) == 1
    for r in range(s.shape[0]):            # everywhere: equal scores are ordered by index
        eq = s[r, 1:] == s[r, :-1]
        assert np.all(i[r, 1:][eq] > i[r, :-1][eq])


def test_self_base_removes_exactly_the_diagonal():
    rng = np.random.default_rng(6)
    X = rng.standard_normal((300, 17)).astype(np.float32)
    _a, x = _carve(X, 20, 1)
    for k in (1, 3, 31):
        s_all, i_all = _search(x, x, k + 1)
        for base, bounds in ((0, None), (0, [0, 100, 129, 300])):
            s, i = _search(x, x, k, chunks=bounds, self_base=base)
            for r in range(300):
                keep = i_all[r] != r
                assert np.array_equal(i[r], i_all[r][keep][:k]) and np.array_equal(s[r].view(np.int32), s_all[r][keep][:k].view(np.int32))
    # a base that matches no pair changes nothing
    s, i = _search(x, x, 3, self_base=5000)
    s0, i0 = _search(x, x, 3)
    assert np.array_equal(i, i0) and np.array_equal(s.view(np.int32), s0.view(np.int32))


def test_short_corpus_nan_rows_and_null_bias():
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((130, 16)).astype(np.float32)
    X = rng.standard_normal((200, 16)).astype(np.float32)
    _a, q = _carve(Q, 19, 0)
    _b, x = _carve(X, 18, 3)
    s, i = _search(q, x[:5], 16)                      # Nc < k: the tail stays +inf / -1
    assert np.all(i[:, :5] >= 0) and np.all(np.isfinite(s[:, :5])) and np.all(i[:, 5:] == -1) and np.all(np.isinf(s[:, 5:]))
    s2, i2 = _search(q, x, 16, chunks=[0, 5, 200])    # ... and fills up with the next chunk
    s3, i3 = _search(q, x, 16)
    assert np.array_equal(i2, i3) and np.array_equal(s2.view(np.int32), s3.view(np.int32))
    Xn = X.copy(); Xn[[0, 77, 199]] = np.nan; Xn[150, 3] = np.nan
    _c, xn = _carve(Xn, 18, 1)
    sn, in_ = _search(q, xn, 32)
    assert not np.isin(in_, [0, 77, 150, 199]).any() and np.all(np.isfinite(sn)) and np.all(in_ >= 0)
    good = np.setdiff1d(np.arange(200), [0, 77, 150, 199])
    sg, ig = _search(q, x, 32, xbias=_sqnorm(x))
    for r in range(130):                              # the other rows are scored as if the NaN rows were not there
        keep = np.isin(ig[r], good)
        m = int(keep.sum())
        assert np.array_equal(in_[r, :m], ig[r][keep]) and np.array_equal(sn[r, :m].view(np.int32), sg[r][keep].view(np.int32))
    s_null, i_null = _search(q, x, 8, xbias=None)
    s_zero, i_zero = _search(q, x, 8, xbias=torch.zeros(200, device="cuda"))
    assert np.array_equal(i_null, i_zero) and np.array_equal(s_null.view(np.int32), s_zero.view(np.int32))
    want_s, want_i = R.topk64(R.scores64(Q, X), 8)
    assert np.all(np.abs(s_null - want_s) <= R.error_bound(Q, X).max(1)[:, None])


# ------------------------------------------------------------------------------------------------ 2b. many corpus tiles per workgroup
@pytest.fixture(scope="module")
def long_corpus():
    """9731 rows = 77 corpus tiles: more than the 32 slabs a call is cut into, so a workgroup walks 3 tiles (the last slab 2: 77 is no
    multiple of 3) and carries its lists and thresholds from tile to tile.  Duplicates and a NaN row sit in late tiles."""
    rng = np.random.default_rng(77)
    D, nc = 17, 9731
    Q = rng.standard_normal((129, D)).astype(np.float32)
    X = rng.standard_normal((nc, D)).astype(np.float32)
    X[[4000, 9000, 9730]] = X[200]                       # duplicates across slabs
    X[9500] = Q[3]; X[300] = Q[3]                        # an exact match in the first and in a late tile
    X[[8200, 9729]] = np.nan
    _a, q = _carve(Q, D + 3, 1)
    _b, x = _carve(X, D + 2, 3)
    xb64 = (X.astype(np.float64) ** 2).sum(1)
    return {"Q": Q, "X": X, "q": q, "x": x, "keep": (_a, _b), "S": R.scores64(Q, X, xb64), "E": R.error_bound(Q, np.nan_to_num(X))}


@pytest.mark.parametrize("k", [1, 32])
@pytest.mark.parametrize("nq", [5, 129])
def test_many_tiles_per_workgroup(long_corpus, nq, k):
    c = long_corpus
    nc = c["X"].shape[0]
    s, i = _search(c["q"][:nq], c["x"], k)
    ref_s, _ri = R.topk64(c["S"][:nq], k)
    emax = c["E"][:nq].max(1)[:, None]
    assert np.all(i >= 0) and np.all(i < nc) and not np.isin(i, [8200, 9729]).any()
    assert np.all(np.abs(s - ref_s) <= emax), np.abs(s - ref_s).max()
    assert np.all(np.abs(np.take_along_axis(c["S"][:nq], i, 1) - ref_s) <= 2 * emax)
    assert np.all(np.diff(s, axis=1) >= 0) and np.all(np.diff(np.sort(i, axis=1), axis=1) > 0)
    for r in range(nq):                                  # ties by index, also across tiles and slabs
        eq = s[r, 1:] == s[r, :-1]
        assert np.all(i[r, 1:][eq] > i[r, :-1][eq])
    if nq > 3:
        assert i[3, 0] == 300 and (k == 1 or i[3, 1] == 9500)
    # the same corpus in 128-row chunks runs one tile per workgroup: the multi-tile walk must agree with it bit for bit
    s1, i1 = _search(c["q"][:nq], c["x"], k, chunks=list(range(0, nc, 128)) + [nc])
    assert np.array_equal(i, i1) and np.array_equal(s.view(np.int32), s1.view(np.int32))
    # ... and an uneven split whose pieces run 2, 1 and 2 tiles per workgroup
    s2, i2 = _search(c["q"][:nq], c["x"], k, chunks=[0, 4097, 4200, 9731])
    assert np.array_equal(i, i2) and np.array_equal(s.view(np.int32), s2.view(np.int32))


# ------------------------------------------------------------------------------------------------ 3. helpers
@pytest.mark.parametrize("D", [1, 3, 63, 64, 65, 302, 3000])
def test_row_helpers_against_float64(D):
    import gpu_util as G
    c = G.ctx()
    rng = np.random.default_rng(D)
    for mag, shift in ((1e-3, 0.0), (1.0, 0.5), (1e3, -2e3)):
        X = (rng.standard_normal((37, D)) * mag + shift).astype(np.float32)
        X[5] = 0.25; X[6] = 0.0; X[7] = -3.0e5                       # constant rows
        _a, x = _carve(X, D + 3, 1 + D % 3)
        got = _sqnorm(x).cpu().numpy().astype(np.float64)
        want = (X.astype(np.float64) ** 2).sum(1)
        assert np.all(np.abs(got - want) <= R.gamma(R.sum_path(D)) * want), f"sqnorm D={D} mag={mag}"
        one = torch.empty(1, device="cuda")                           # the sum of a row does not depend on N
        for r in (0, 5, 36):
            G.check(G.lib.eegldm_rows_sqnorm(c.h, G.ptr(x[r:r + 1]), x.stride(0), 1, D, G.ptr(one)))
            assert float(one) == np.float32(got[r])
        out = torch.full((37, D + 2), 9.0, device="cuda")
        G.check(G.lib.eegldm_rows_standardize(c.h, G.ptr(x), x.stride(0), 37, D, G.ptr(out), D + 2))
        z = out[:, :D].cpu().numpy().astype(np.float64)
        assert np.all(out[:, D:].cpu().numpy() == 9.0)
        assert np.all(z[[5, 6, 7]] == 0.0), "constant rows become zeros"
        ref = R.standardize64(X)
        if D == 1:
            assert np.all(z == 0.0)
            continue
        assert np.all(np.abs(z - ref) <= R.standardize_bound(X) + 1e-300), f"standardize D={D} mag={mag}: {np.abs(z - ref).max():.3e}"
        o1 = torch.empty(1, D, device="cuda")
        G.check(G.lib.eegldm_rows_standardize(c.h, G.ptr(x[36:37]), x.stride(0), 1, D, G.ptr(o1), D))
        assert torch.equal(o1[0], out[36, :D])


@pytest.mark.parametrize("D", [1, 17, 302, 3000])
def test_rescore_direct_form(D):
    import gpu_util as G
    c = G.ctx()
    rng = np.random.default_rng(40 + D)
    Q = (rng.standard_normal((9, D)) * 3 + 100).astype(np.float32)          # a large common offset: the expanded form cancels badly here
    X = (rng.standard_normal((50, D)) * 3 + 100).astype(np.float32)
    X[20] = Q[4]
    _a, q = _carve(Q, D + 1, 1)
    _b, x = _carve(X, D + 2, 2)
    k = 4
    idx = torch.from_numpy(rng.integers(0, 50, (9, k))).cuda()
    idx[4, 1] = 30; idx[0, 0] = -1; idx[1, 1] = 1000; idx[2, 2] = 5         # row 20 of the chunk is a copy of query 4; outside [10, 60): left alone
    out = torch.full((9, k), -7.0, device="cuda")
    G.check(G.lib.eegldm_knn_rescore(c.h, G.ptr(q), q.stride(0), G.ptr(x), x.stride(0), 9, D, k, 10, 50, G.ptr(idx), G.ptr(out)))
    got, ii = out.cpu().numpy().astype(np.float64), idx.cpu().numpy() - 10
    d2 = R.sqdist64(Q, X)
    for r in range(9):
        for s in range(k):
            if 0 <= ii[r, s] < 50:
                want = d2[r, ii[r, s]]
                assert (r, s) != (4, 1) or want == 0.0
                assert abs(got[r, s] - want) <= (D + 2) * R.U * want, (D, r, s, got[r, s], want)
            else:
                assert got[r, s] == -7.0


def test_exact_copies_rescored_and_correlated():
    from eegldm.metrics import NearestNeighbours
    rng = np.random.default_rng(11)
    D = 302
    X = (rng.standard_normal((400, D)) + 50).astype(np.float32)
    Q = np.concatenate([X[[7, 250]], (rng.standard_normal((3, D)) + 50).astype(np.float32)])
    x, q = torch.from_numpy(X), torch.from_numpy(Q)
    nn = NearestNeighbours(q, 2).update(x[:130]).update(x[130:])
    d, i = nn.result(rescore=x.cuda())
    assert i[0, 0] == 7 and i[1, 0] == 250 and float(d[0, 0]) == 0.0 and float(d[1, 0]) == 0.0 and bool((d[2:, 0] > 0).all())
    d2 = R.sqdist64(Q, X)
    want = np.take_along_axis(d2, i.cpu().numpy(), 1)
    assert np.all(np.abs(d.cpu().numpy() - want) <= (D + 2) * R.U * want)
    dc, ic = NearestNeighbours(q, 1, "correlation").update(x).result()
    assert ic[0, 0] == 7 and ic[1, 0] == 250
    assert float(dc[:2].max()) <= 4 * R.U * R.c_of(D)


# ------------------------------------------------------------------------------------------------ 4. metrics
PRC_SEEDS, PRC_SHIFT = (21, 22), 0.08      # checked with the float64 reference: no row within 2 E of a ball surface


def _prc_sets():
    D = 302
    real = np.random.default_rng(PRC_SEEDS[0]).standard_normal((300, D)).astype(np.float32)
    fake = (np.random.default_rng(PRC_SEEDS[1]).standard_normal((257, D)) * 0.97 + PRC_SHIFT).astype(np.float32)
    return real, fake


def test_kth_radius_against_float64():
    from eegldm.metrics import kth_radius
    real, _f = _prc_sets()
    for k in (1, 3):
        got = kth_radius(torch.from_numpy(real), k, squared=True, chunk=128).cpu().numpy().astype(np.float64)
        want = R.kth_radius2_64(real, k)
        # a neighbour swapped inside the search's 2 E still changes the order statistic by at most 2 E; the direct form adds (D + 2) u
        tol = 2 * R.error_bound(real, real).max(1) + (302 + 2) * R.U * want
        assert np.all(np.abs(got - want) <= tol), np.abs(got - want).max()
        assert np.allclose(kth_radius(torch.from_numpy(real), k, chunk=300).cpu().numpy(), np.sqrt(got), rtol=1e-6)


def test_precision_recall_coverage_against_float64():
    from eegldm.metrics import precision_recall_coverage
    real, fake = _prc_sets()
    got = precision_recall_coverage(torch.from_numpy(real), torch.from_numpy(fake), k=3, chunk=100)
    want, margins = R.prc64(real, fake, 3)
    e_rf, e_fr = 2 * R.error_bound(real, fake).max(1), 2 * R.error_bound(fake, real).max(1)
    close = {"precision": int((np.abs(margins["precision"]) < e_fr).sum()), "recall": int((np.abs(margins["recall"]) < e_rf).sum()),
             "coverage": int((np.abs(margins["coverage"]) < e_rf).sum())}
    rows = {"precision": 257, "recall": 300, "coverage": 300}
    print(got, want, close)
    for name in rows:
        assert close[name] <= 0.01 * rows[name], f"{name}: {close[name]} rows sit within 2 E of their ball's surface -- other seeds are needed"
        assert abs(got[name] - want[name]) * rows[name] <= close[name] + 1e-9, (name, got[name], want[name], close[name])


def test_precision_recall_coverage_extremes():
    from eegldm.metrics import precision_recall_coverage
    real, _f = _prc_sets()
    same = precision_recall_coverage(torch.from_numpy(real), torch.from_numpy(real.copy()), k=3)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0
    far = precision_recall_coverage(torch.from_numpy(real), torch.from_numpy(real[:257] + 100.0), k=3)
    assert far["precision"] == far["recall"] == far["coverage"] == 0.0


# ------------------------------------------------------------------------------------------------ 5. audit
def _audit_sets():
    """Seed 33: fresh windows are drawn like the held-out ones, so each falls below a 1 % quantile of those 1 % of the time by construction;
    with this seed the float64 correlations put every fresh window at least 7e-3 above the threshold, with and without lags (fp32 error
    of 1 - r at D = 3000: below 4e-4)."""
    rng = np.random.default_rng(33)
    L = 3000
    train = rng.standard_normal((300, L)).astype(np.float32)
    hold = rng.standard_normal((40, L)).astype(np.float32)
    fresh = rng.standard_normal((20, L)).astype(np.float32)
    exact = train[[5, 131, 299]].copy()
    shifted = rng.standard_normal((2, L)).astype(np.float32)
    shifted[0, :L - 5] = train[17, 5:]            # the training window, 5 samples early
    shifted[1, 5:] = train[200, :L - 5]           # ... and 5 samples late
    syn = np.concatenate([exact, shifted, fresh])
    return train, hold, syn, [5, 131, 299, 17, 200]


def test_audit_flags_planted_copies():
    from eegldm.metrics import memorisation_audit
    train, hold, syn, planted = _audit_sets()
    chunks = lambda: (torch.from_numpy(train[s:s + 128]) for s in range(0, 300, 128))
    a = memorisation_audit(torch.from_numpy(syn), chunks(), torch.from_numpy(hold), lags=(-5, 0, 5))
    assert a["flagged"] == [0, 1, 2, 3, 4] and [r[0] for r in a["nearest_index"][:5]] == planted
    assert a["n_train"] == 300 and a["n_synthetic"] == 25 and a["n_holdout"] == 40 and a["lags"] == [-5, 0, 5]
    b = memorisation_audit(torch.from_numpy(syn).unsqueeze(1), chunks(), torch.from_numpy(hold))
    assert b["flagged"] == [0, 1, 2] and [r[0] for r in b["nearest_index"][:3]] == planted[:3]
    assert max(r[0] for r in b["nearest_distance"][:3]) <= 4 * R.U * R.c_of(3000)
    assert b["holdout_quantiles"]["0.0"] <= b["threshold"] <= b["holdout_quantiles"]["0.05"] and 0.5 < b["threshold"] < 1.0


def test_audit_script_round_trip(tmp_path):
    from eegldm.entry import audit_memorisation as A
    train, hold, syn, planted = _audit_sets()
    os.makedirs(tmp_path / "syn")
    np.save(tmp_path / "syn" / "sample_0.npy", syn[:10].reshape(10, 1, 3000))
    np.save(tmp_path / "syn" / "sample_1.npy", syn[10:].reshape(15, 1, 3000))
    np.save(tmp_path / "train.npy", train); np.save(tmp_path / "hold.npy", hold)
    out = str(tmp_path / "audit.json")
    res = A.main(A.parse_args(["--synthetic", str(tmp_path / "syn"), "--train_npy", str(tmp_path / "train.npy"), "--holdout_npy",
                               str(tmp_path / "hold.npy"), "--lags", "-5", "0", "5", "--chunk", "100", "--output", out]))
    with open(out) as f:
        back = json.load(f)
    assert back == json.loads(json.dumps(res)) and back["flagged"] == [0, 1, 2, 3, 4]
    assert [r[0] for r in back["nearest_index"][:5]] == planted and len(back["files"]) == 2


def test_feature_space_audit_and_script(tmp_path):
    """Plumbing of space="features": 3000- and 3072-sample windows through fid_features of a randomly initialised U-Sleep, a planted copy
    found at its index, and the entry script's precision / recall / coverage block."""
    from eegldm.entry import audit_memorisation as A
    from eegldm.entry.common import synthetic_windows
    from eegldm.metrics import USleep, memorisation_audit
    train = synthetic_windows(40, seed=1)                    # (40, 1, 3072), zero pads
    hold = synthetic_windows(10, seed=2)
    syn = synthetic_windows(12, seed=3)[:, :, 36:-36].copy() # (12, 1, 3000), as the samplers write them
    syn[4] = train[21, :, 36:-36]
    torch.manual_seed(0)
    model = USleep(in_chans=2, sfreq=100, depth=12, with_skip_connection=True, n_classes=5, input_size_s=30, apply_softmax=False).eval()
    a = memorisation_audit(torch.from_numpy(syn), [torch.from_numpy(train[:25]), torch.from_numpy(train[25:])], torch.from_numpy(hold),
                           space="features", k=2, usleep=model)
    assert a["n_train"] == 40 and a["n_synthetic"] == 12 and a["n_holdout"] == 10 and a["space"] == "features"
    d = np.asarray(a["nearest_distance"]); i = np.asarray(a["nearest_index"])
    assert d.shape == (12, 2) and np.all(np.isfinite(d)) and np.all(d >= 0) and np.all((i >= 0) & (i < 40))
    # the planted copy has the features of training row 21: its expanded-form distance is rounding alone, E(i, j) for q = x plus |q|^2's own
    # error, 5 c(302) u |f|^2 (no index is asserted: a randomly initialised extractor need not separate windows by more than that)
    from eegldm.metrics import fid_features
    f2 = float(fid_features(model, torch.from_numpy(syn[4:5])).double().pow(2).sum())
    assert d[4, 0] <= 5 * R.c_of(302) * R.U * f2
    with pytest.raises(ValueError, match="lags"):
        memorisation_audit(torch.from_numpy(syn), [torch.from_numpy(train)], torch.from_numpy(hold), space="features", lags=(0, 5), usleep=model)
    os.makedirs(tmp_path / "syn")
    np.save(tmp_path / "syn" / "sample_0.npy", syn)
    np.save(tmp_path / "train.npy", train); np.save(tmp_path / "hold.npy", hold)
    out = str(tmp_path / "audit.json")
    res = A.main(A.parse_args(["--synthetic", str(tmp_path / "syn"), "--train_npy", str(tmp_path / "train.npy"), "--holdout_npy",
                               str(tmp_path / "hold.npy"), "--space", "features", "--chunk", "16", "--output", out]))
    with open(out) as f:
        back = json.load(f)
    assert back == json.loads(json.dumps(res)) and back["n_train"] == 40 and len(back["nearest_index"]) == 12
    prc = back["precision_recall_coverage"]
    assert prc["n_real"] == 40 and prc["n_fake"] == 12 and prc["k"] == 3
    assert all(0.0 <= prc[n] <= 1.0 for n in ("precision", "recall", "coverage"))
