"""-m gpu: R = K(A, B) V of csrc/kmm.hip (eegldm_kernel_matmul) against a float64 evaluation of the same definition within the
operation-count bound of tests/kmm_reference.py, the bit-exact anchors (repeat runs, column and row independence, exact integer data), streaming with
`accumulate`, the left-out diagonal, non-finite inputs, the refusals, and the statistics built on it (MMD^2, KID, witness, permutation test,
the entry script)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import kmm_reference as R
from test_kmm_cpu import PERM_SEEDS, perm_kw, perm_sets

pytestmark = pytest.mark.gpu

# The statistics are float64 algebra on R, on the host or in torch: sums of at most 300 terms, each rounding at most 2^-53 of the terms'
# absolute sum, 3.3e-14 of sum |k V| in all.  The bound of R holds at least g(33) = 2.0e-6 of that same sum, so the algebra's own rounding is
# below 2e-8 of the propagated bound: the factor below covers it.
F64_ALGEBRA = 1.0 + 1e-6

NO_DIAG = R.NO_DIAG


def _carve(a, ld, off, fill=7.0e30):
    """Rows of `a` on the device with row stride ld (>= D), starting `off` floats into an allocation filled with `fill`: a read outside the rows
    shows in every result."""
    n, d = a.shape
    buf = torch.full((off + max(n, 1) * ld + 4,), fill, device="cuda")
    view = buf[off:off + max(n, 1) * ld].view(max(n, 1), ld)[:n, :d]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    return buf, view


def _sqnorm(x, off=0):
    """eegldm_rows_sqnorm of a device view, `off` floats into its own allocation."""
    import gpu_util as G
    buf = torch.full((off + x.shape[0] + 4,), 7.0e30, device="cuda")
    out = buf[off:off + x.shape[0]]
    if x.shape[0]:
        G.check(G.lib.eegldm_rows_sqnorm(G.ctx().h, G.ptr(x), x.stride(0), x.shape[0], x.shape[1], G.ptr(out)))
    return out


def _raw(a, asq, b, bsq, v, out, Na, Nb, D, P, kind="poly", degree=3, gamma=None, coef0=1.0, betas=None, diag_off=NO_DIAG, accumulate=0,
         lda=None, ldb=None, ldv=None, ldo=None):
    """The export itself -> return code."""
    import gpu_util as G
    bt = np.asarray([0.0] if betas is None else betas, np.float32)
    return G.lib.eegldm_kernel_matmul(G.ctx().h, G.ptr(a), a.stride(0) if lda is None else lda, G.ptr(asq), G.ptr(b), b.stride(0) if ldb is None else ldb,
                                      G.ptr(bsq), G.ptr(v), v.stride(0) if ldv is None else ldv, Na, Nb, D, P, 1 if kind == "rbf" else 0, degree,
                                      1.0 / max(D, 1) if gamma is None else gamma, coef0, (ctypes.c_float * len(bt))(*bt.tolist()),
                                      len(bt) if kind == "rbf" else 0, diag_off, accumulate, G.ptr(out), out.stride(0) if ldo is None else ldo)


def _run(a, b, v, kind="poly", asq=None, bsq=None, out=None, accumulate=0, **kw):
    """R (Na, P) float64 numpy of device views a (Na, D), b (Nb, D), v (Nb, P)."""
    import gpu_util as G
    na, nb, d, p = a.shape[0], b.shape[0], a.shape[1], v.shape[1]
    if kind == "rbf" and asq is None:
        asq, bsq = _sqnorm(a), _sqnorm(b)
    if out is None:
        out = torch.full((na, p + 1), -7.0, dtype=torch.float64, device="cuda")[:, :p]
    # an empty tensor has no address: with Nb == 0 any valid pointer stands in for b, bsq and v
    G.check(_raw(a, asq, b if nb else a, bsq if nb else asq, v if nb else a, out, na, nb, d, p, kind=kind, accumulate=accumulate, lda=a.stride(0),
                 ldb=b.stride(0) if nb > 1 else d, ldv=v.stride(0) if nb > 1 else p, **kw))
    torch.cuda.synchronize()
    return out.cpu().numpy().copy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


# ------------------------------------------------------------------------------------------------ 1. against float64
NAS, NBS, PS, SS = (1, 127, 128, 129, 257), (0, 1, 127, 129, 1000), (1, 2, 63, 64), (1, 3, 8)
SIGMA_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)


@pytest.mark.parametrize("D", [1, 15, 16, 17, 302, 3000])
def test_against_float64(D):
    """|R - R64| <= E elementwise (kmm_reference.error_bound) for both kernels over Na x Nb, P, degree 1..4, S in {1, 3, 8}, magnitudes 1e-3 .. 1e3,
    row strides above D and P, every float pointer 0..3 floats off its allocation in buffers filled with 7e30."""
    combos = [(129, 257)] if D == 3000 else [(na, nb) for na in NAS for nb in NBS]
    n = 0
    worst = {"poly": 0.0, "rbf": 0.0}
    seen = set()
    for mag in (1e-3, 1.0, 1e3):
        rng = np.random.default_rng(1000 * D + int(np.log10(mag)) + 7)
        A = (rng.standard_normal((max(c[0] for c in combos), D)) * mag).astype(np.float32)
        B = (rng.standard_normal((max(c[1] for c in combos), D)) * mag).astype(np.float32)
        V = rng.standard_normal((B.shape[0], 64)).astype(np.float32)
        for na, nb in combos:
            n += 1
            kind = ("poly", "rbf")[n % 2]
            P, degree, S = PS[(n // 2) % 4], 1 + (n // 8) % 4, SS[(n // 8) % 3]
            _ab, a = _carve(A[:na], D + 1 + n % 3, n % 4)
            _bb, b = _carve(B[:nb], D + 2 + n % 5, (n // 4) % 4)
            _vb, v = _carve(V[:nb, :P], P + n % 3, (n // 16) % 4)
            obuf = torch.full((na * (P + 2) + 2,), -7.0, dtype=torch.float64, device="cuda")
            out = obuf[1:1 + na * (P + 2)].view(na, P + 2)[:, :P]
            kw = dict(kind=kind)
            if kind == "poly":
                kw.update(degree=degree, gamma=(None, 0.37 / (mag * mag))[n % 3 == 0], coef0=(1.0, -0.5, 0.0)[n % 3])
                got = _run(a, b, v, out=out, **kw)
            else:
                asq, bsq = _sqnorm(a, (n // 2) % 4), _sqnorm(b, (n // 3) % 4)
                kw.update(betas=[1.0 / (2.0 * (s * mag * np.sqrt(D)) ** 2) for s in SIGMA_SCALES[:S]])
                got = _run(a, b, v, asq=asq, bsq=bsq, out=out, **kw)
                kw.update(asq=asq.cpu().numpy(), bsq=bsq.cpu().numpy())
            seen.add((kind, P)); seen.add((kind, degree if kind == "poly" else S))
            tag = f"D={D} mag={mag} Na={na} Nb={nb} P={P} {kw['kind']} degree={degree} S={S}"
            gut = obuf.cpu().numpy()
            assert gut[0] == -7.0 and gut[-1] == -7.0 and np.all(gut[1:-1].reshape(na, P + 2)[:, P:] == -7.0), f"{tag}: a write outside out"
            want, _k = R.kmm64(A[:na], B[:nb], V[:nb, :P], **kw)
            E = R.error_bound(A[:na], B[:nb], V[:nb, :P], **kw)
            assert np.all(np.isfinite(got)), tag
            err = np.abs(got - want)
            assert np.all(err <= E), f"{tag}: off by {err.max():.3e}, bound {E[np.unravel_index(np.argmax(err - E), E.shape)]:.3e}"
            if nb:
                worst[kind] = max(worst[kind], float((err / E).max()))
            else:
                assert not got.any(), tag
    if D != 3000:
        assert all((k, p) in seen for k in ("poly", "rbf") for p in PS), "every P for both kernels"
        assert all(("poly", d) in seen for d in (1, 2, 3, 4)) and all(("rbf", s) in seen for s in SS)
    print(f"kmm_numerics: D={D}: {n} calls, worst error / bound: poly {worst['poly']:.3f}, rbf {worst['rbf']:.3f}")


# ------------------------------------------------------------------------------------------------ 2. anchors
@pytest.fixture(scope="module")
def anchor():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((257, 33)).astype(np.float32)
    B = rng.standard_normal((1000, 33)).astype(np.float32)
    V = rng.standard_normal((1000, 64)).astype(np.float32)
    _a, a = _carve(A, 40, 1)
    _b, b = _carve(B, 37, 2)
    _v, v = _carve(V, 67, 3)
    kws = {"poly": dict(kind="poly", degree=3), "rbf": dict(kind="rbf", betas=[0.01, 0.03])}
    return {"a": a, "b": b, "v": v, "keep": (_a, _b, _v), "kws": kws, "full": {k: _run(a, b, v, **kw) for k, kw in kws.items()}}


@pytest.mark.parametrize("kernel", ["poly", "rbf"])
def test_repeat_column_and_row_independence(anchor, kernel):
    a, b, v, kw, full = anchor["a"], anchor["b"], anchor["v"], anchor["kws"][kernel], anchor["full"][kernel]
    assert np.array_equal(_bits(_run(a, b, v, **kw)), _bits(full)), "run == run"
    for p in (0, 31, 32, 63):              # a column of a P = 1 call is the same column of the 64-wide call
        assert np.array_equal(_bits(_run(a, b, v[:, p:p + 1], **kw)[:, 0]), _bits(full[:, p])), p
    assert np.array_equal(_bits(_run(a, b, v[:, 7:40], **kw)), _bits(full[:, 7:40]))
    for lo, hi in ((0, 1), (100, 131), (128, 257), (255, 257)):          # rows of A computed alone
        assert np.array_equal(_bits(_run(a[lo:hi], b, v, **kw)), _bits(full[lo:hi])), (lo, hi)


@pytest.fixture(scope="module")
def long_b():
    """Nb = 4233 = 34 tiles, D = 5: 17 slabs of two tiles, the last slab ragged (its second tile holds 9 rows)."""
    rng = np.random.default_rng(77)
    A = rng.standard_normal((129, 5)).astype(np.float32)
    B = rng.standard_normal((4233, 5)).astype(np.float32)
    V = rng.standard_normal((4233, 64)).astype(np.float32)
    _a, a = _carve(A, 7, 1)
    _b, b = _carve(B, 6, 3)
    _v, v = _carve(V, 64, 2)
    return {"A": A, "B": B, "V": V, "a": a, "b": b, "v": v, "keep": (_a, _b, _v)}


@pytest.mark.parametrize("kernel", ["poly", "rbf"])
def test_many_tiles_per_slab_and_accumulate(long_b, kernel):
    """Against float64; then B streamed with `accumulate`.  NOT bit-equal by construction: a slab adds its 32-row chains one after the other
    into one float64 register, a chunked call folds the same chains in other groups.  Chunking at multiples of 32 rows leaves every chain's
    fp32 result as it is and only re-associates the float64 additions: held to Nb 2^-53 sum |k V| (of the device's k: the reference's plus
    its bound), at multiples of the slab size (256 rows here) as at any other.  Chunks that cut a chain (1000 = 31 x 32 + 8 rows) change
    which rows share an fp32 chain: held to E against float64 like any other call."""
    c = long_b
    a, b, v = c["a"], c["b"], c["v"]
    assert R.slab_rows(4233) == 256
    kw = dict(kind="poly", degree=2) if kernel == "poly" else dict(kind="rbf", betas=[0.05, 0.2, 0.8])
    asq, bsq = (_sqnorm(a), _sqnorm(b)) if kernel == "rbf" else (None, None)
    one = _run(a, b, v, asq=asq, bsq=bsq, **kw)
    ref_kw = dict(kw, asq=asq.cpu().numpy(), bsq=bsq.cpu().numpy()) if kernel == "rbf" else kw
    want, k64 = R.kmm64(c["A"], c["B"], c["V"], **ref_kw)
    E = R.error_bound(c["A"], c["B"], c["V"], **ref_kw)
    err = np.abs(one - want)
    assert np.all(err <= E), f"off by {err.max():.3e}"
    print(f"kmm_numerics: Nb=4233 D=5 {kernel}: worst error / bound {float((err / E).max()):.3f}")

    def streamed(step):
        out = torch.full((129, 64), -7.0, dtype=torch.float64, device="cuda")
        for s in range(0, 4233, step):
            _run(a, b[s:s + step], v[s:s + step], asq=asq, bsq=None if bsq is None else bsq[s:s + step], out=out, accumulate=1 if s else 0, **kw)
        return out.cpu().numpy()
    tol = 4233 * 2.0 ** -53 * ((np.abs(k64) @ np.abs(c["V"].astype(np.float64))) + E)
    for step in (256, 1024, 384, 4096, 32 * 33):
        assert np.all(np.abs(streamed(step) - one) <= tol), step
    assert np.all(np.abs(streamed(1000) - want) <= E)


def test_small_integers_are_exact():
    """degree 1, gamma 1, coef0 0, V = 1: every product, chain and sum is an integer below 2^24, so the device result IS the float64 one."""
    rng = np.random.default_rng(9)
    A = rng.integers(-3, 4, (130, 17)).astype(np.float32)
    B = rng.integers(-3, 4, (1000, 17)).astype(np.float32)
    V = np.ones((1000, 3), np.float32)
    _a, a = _carve(A, 19, 1); _b, b = _carve(B, 18, 2); _v, v = _carve(V, 5, 3)
    got = _run(a, b, v, kind="poly", degree=1, gamma=1.0, coef0=0.0)
    want = (A.astype(np.float64) @ B.astype(np.float64).T).sum(1, keepdims=True).repeat(3, 1)
    assert np.array_equal(got, want)
    got = _run(a, b[:130], v[:130], kind="poly", degree=1, gamma=1.0, coef0=0.0, diag_off=0)
    k = A.astype(np.float64) @ B[:130].astype(np.float64).T
    assert np.array_equal(got[:, 0], k.sum(1) - np.diag(k))


# ------------------------------------------------------------------------------------------------ 3. the left-out diagonal
@pytest.mark.parametrize("kernel", ["poly", "rbf"])
@pytest.mark.parametrize("off", [0, 3, 130, -2, -129])
def test_diagonal_is_left_out_not_subtracted(kernel, off):
    """Rows 5, 131 and 260 have 1e3 times the norm of the others and meet THEMSELVES on the left-out diagonal: those pairs dominate the full
    sum (poly: 1e18 against 1e10), so a sum-then-subtract implementation cannot meet the bound of the sum without them."""
    rng = np.random.default_rng(100 + abs(off))
    X = rng.standard_normal((300, 17)).astype(np.float32)
    X[[5, 131, 260]] *= 1e3
    A, B = (X[off:], X) if off >= 0 else (X, X[-off:])           # a_i = b_(i + off)
    V = rng.standard_normal((B.shape[0], 2)).astype(np.float32)
    _a, a = _carve(A, 20, 1); _b, b = _carve(B, 19, 2); _v, v = _carve(V, 3, 1)
    kw = dict(kind="poly", degree=3) if kernel == "poly" else dict(kind="rbf", betas=[1.0 / (2 * 17.0), 1.0 / (2 * 68.0)])
    asq, bsq = (_sqnorm(a), _sqnorm(b)) if kernel == "rbf" else (None, None)
    ref_kw = dict(kw, asq=asq.cpu().numpy(), bsq=bsq.cpu().numpy()) if kernel == "rbf" else kw
    got = _run(a, b, v, asq=asq, bsq=bsq, diag_off=off, **kw)
    want, _k = R.kmm64(A, B, V, diag_off=off, **ref_kw)
    E = R.error_bound(A, B, V, diag_off=off, **ref_kw)
    assert np.all(np.abs(got - want) <= E), np.abs(got - want).max()
    full, kfull = R.kmm64(A, B, V, **ref_kw)
    i = 260 - max(off, 0)                                         # the row of A that is X[260]
    left_out = kfull[i, i + off] * np.abs(V[i + off].astype(np.float64))
    assert np.all(left_out > 1e3 * E[i]), "the left-out term dwarfs the bound: subtracting it afterwards would fail"
    got_full = _run(a, b, v, asq=asq, bsq=bsq, diag_off=NO_DIAG, **kw)
    assert np.all(np.abs(got_full - full) <= R.error_bound(A, B, V, **ref_kw))
    far = _run(a, b, v, asq=asq, bsq=bsq, diag_off=5000, **kw)   # a diagonal that meets no pair changes nothing
    assert np.array_equal(_bits(far), _bits(got_full))


# ------------------------------------------------------------------------------------------------ 4. non-finite values
@pytest.mark.parametrize("kernel", ["poly", "rbf"])
def test_non_finite_inputs(kernel):
    rng = np.random.default_rng(12)
    A = rng.standard_normal((130, 16)).astype(np.float32)
    B = rng.standard_normal((200, 16)).astype(np.float32)
    V = rng.standard_normal((200, 5)).astype(np.float32)
    V[77] = 0.0
    kw = dict(kind="poly", degree=2) if kernel == "poly" else dict(kind="rbf", betas=[0.02, 0.1])
    _a, a = _carve(A, 19, 0); _b, b = _carve(B, 18, 3); _v, v = _carve(V, 7, 1)
    clean = _run(a, b, v, **kw)
    An = A.copy(); An[3] = np.nan
    _c, an = _carve(An, 19, 2)
    got = _run(an, b, v, **kw)
    assert np.isnan(got[3]).all() and np.array_equal(_bits(np.delete(got, 3, 0)), _bits(np.delete(clean, 3, 0))), "a NaN row of A poisons that row only"
    Bn = B.copy(); Bn[77] = np.nan                                # V[77] == 0: NaN * 0 is NaN, as in K @ V
    _d, bn = _carve(Bn, 18, 1)
    ref_kw = dict(kw, asq=_sqnorm(a).cpu().numpy(), bsq=_sqnorm(bn).cpu().numpy()) if kernel == "rbf" else kw
    assert np.isnan(R.kmm64(A, Bn, V, **ref_kw)[0]).all()
    assert np.isnan(_run(a, bn, v, **kw)).all(), "a NaN row of B poisons all of R"
    # ... unless the pair is left out: the NaN row of B on the left-out diagonal of a one-row A
    alone = _run(a[70:71], bn[:100], v[:100], diag_off=77, **kw)
    assert np.all(np.isfinite(alone))
    # inf in the stride gutters and around the rows changes nothing
    _e, ai = _carve(A, 19, 0, fill=float("inf")); _f, bi = _carve(B, 18, 3, fill=float("-inf")); _g, vi = _carve(V, 7, 1, fill=float("inf"))
    assert np.array_equal(_bits(_run(ai, bi, vi, **kw)), _bits(clean))


def test_expf_error_within_the_bound_s_3_ulp():
    """The device expf alone: a = 0, bsq = 0, Nb = 1, V = 1, S = 1 make R[i] = expf(-beta * asq[i]) exactly (asq is taken as given), beta = +-1.
    The largest error against float64 exp of the same fp32 argument, in ulps of the result, is printed (profiles/kmm_numerics.txt) and held
    to the EXPF_ULPS the bound assumes."""
    n = 4096
    rng = np.random.default_rng(3)
    args = np.concatenate([rng.uniform(0, 87, n // 2), np.exp(rng.uniform(np.log(1e-6), np.log(87), n // 2))]).astype(np.float32)
    a = torch.zeros(n, 1, device="cuda"); b = torch.zeros(1, 1, device="cuda"); v = torch.ones(1, 1, device="cuda")
    asq = torch.from_numpy(args).cuda(); bsq = torch.zeros(1, device="cuda")
    worst = 0.0
    for beta in (1.0, -1.0):
        got = _run(a, b, v, kind="rbf", asq=asq, bsq=bsq, betas=[beta])[:, 0]
        want = np.exp(-beta * args.astype(np.float64))
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.array_equal(got, got.astype(np.float32).astype(np.float64)), "R is the fp32 kernel value itself"
        worst = max(worst, float((np.abs(got - want) / ulp).max()))
    print(f"kmm_numerics: device expf on {2 * n} arguments in [-87, 87]: largest error {worst:.3f} ulp (bound assumes {R.EXPF_ULPS:g})")
    assert worst <= R.EXPF_ULPS


# ------------------------------------------------------------------------------------------------ 5. refusals of the export
def test_export_refusals_leave_out_untouched():
    import gpu_util as G
    a = torch.zeros(8, 6, device="cuda"); b = torch.zeros(9, 6, device="cuda"); v = torch.ones(9, 4, device="cuda")
    sq = torch.zeros(16, device="cuda")
    out = torch.full((8, 4), -7.0, dtype=torch.float64, device="cuda")
    base = dict(Na=8, Nb=9, D=6, P=4)
    cases = [
        (dict(base, P=0), {}, "P 0"), (dict(base, P=65), {}, "P 65"),
        (base, dict(degree=0), "degree"), (base, dict(degree=5), "degree"),
        (base, dict(kind="rbf", betas=[]), "n_betas"), (base, dict(kind="rbf", betas=[0.1] * 9), "n_betas"),
        (dict(base, D=0), {}, "D 0"),
        (base, dict(lda=5), "row strides"), (base, dict(ldb=5), "row strides"), (base, dict(ldv=3), "row strides"), (base, dict(ldo=3), "row strides"),
    ]
    for sizes, kw, msg in cases:
        asq = sq if kw.get("kind") == "rbf" else None
        rc = _raw(a, asq, b, asq, v, out, **sizes, **kw)
        assert rc != 0 and msg.encode() in G.lib.eegldm_last_error(), (msg, G.lib.eegldm_last_error())
    for asq, bsq in ((None, sq), (sq, None)):
        rc = _raw(a, asq, b, bsq, v, out, kind="rbf", betas=[0.1], **base)
        assert rc != 0 and b"squared norms" in G.lib.eegldm_last_error()
    rc = G.lib.eegldm_kernel_matmul(G.ctx().h, G.ptr(a), 6, None, G.ptr(b), 6, None, G.ptr(v), 4, 8, 9, 6, 4, 0, 3, 1.0, 1.0, None, 0, NO_DIAG, 0,
                                    ctypes.c_void_p(out.data_ptr() + 4), 4)
    assert rc != 0 and b"8-byte aligned" in G.lib.eegldm_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()), "a refused call wrote to out"
    # Nb == 0: zeros, or out left alone when accumulating
    assert not _run(a, b[:0], v[:0]).any()
    keep = torch.full((8, 4), 2.5, dtype=torch.float64, device="cuda")
    assert np.all(_run(a, b[:0], v[:0], out=keep, accumulate=1) == 2.5)


# ------------------------------------------------------------------------------------------------ 6. statistics
def _stat_sets():
    rng = np.random.default_rng(21)
    return rng.standard_normal((150, 16)).astype(np.float32), (rng.standard_normal((130, 16)) * 1.1 + 0.2).astype(np.float32)


def _ref_kw(kernel, a, b, sigmas=(2.0, 4.0, 8.0)):
    """Reference keywords with asq / bsq as the device computes them."""
    from eegldm.metrics import rbf_betas, rows_sqnorm
    if kernel == "poly":
        return dict(kind="poly", degree=3, gamma=None, coef0=1.0)
    sq = lambda t: rows_sqnorm(torch.from_numpy(t).cuda()).cpu().numpy()
    return dict(kind="rbf", betas=rbf_betas(sigmas), asq=sq(a), bsq=sq(b))


@pytest.mark.parametrize("kernel", ["poly", "rbf"])
def test_mmd2_and_witness_against_float64(kernel):
    """The statistics are float64 algebra on R, so their error is the bound of R pushed through that algebra."""
    from eegldm import metrics as M
    x, y = _stat_sets()
    n, m = len(x), len(y)
    one_n, one_m = np.ones((n, 1), np.float32), np.ones((m, 1), np.float32)
    args = dict(kernel=kernel, sigmas=(2.0, 4.0, 8.0) if kernel == "rbf" else None)
    for unbiased in (True, False):
        d = 0 if unbiased else None
        got = M.mmd2(torch.from_numpy(x), torch.from_numpy(y), unbiased=unbiased, chunk=100, **args)
        sxx, exx = R.kmm64(x, x, one_n, diag_off=d, **_ref_kw(kernel, x, x))[0].sum(), R.error_bound(x, x, one_n, diag_off=d, **_ref_kw(kernel, x, x)).sum()
        syy, eyy = R.kmm64(y, y, one_m, diag_off=d, **_ref_kw(kernel, y, y))[0].sum(), R.error_bound(y, y, one_m, diag_off=d, **_ref_kw(kernel, y, y)).sum()
        sxy, exy = R.kmm64(x, y, one_m, **_ref_kw(kernel, x, y))[0].sum(), R.error_bound(x, y, one_m, **_ref_kw(kernel, x, y)).sum()
        want = M.mmd2_from_sums(sxx, syy, sxy, n, m, unbiased)
        dx, dy = (n * (n - 1), m * (m - 1)) if unbiased else (n * n, m * m)
        # chunk = 100 re-associates the float64 sums: Nb 2^-53 sum |k V| per element, already part of E
        tol = F64_ALGEBRA * (exx / dx + eyy / dy + 2 * exy / (n * m))
        assert abs(got["mmd2"] - want["mmd2"]) <= tol, (got["mmd2"], want["mmd2"], tol)
        assert set(got) == {"mmd2", "kxx", "kyy", "kxy", "n", "m"} and got["n"] == n and got["m"] == m
        assert abs(got["kxx"] - want["kxx"]) <= F64_ALGEBRA * exx / dx and abs(got["kxy"] - want["kxy"]) <= F64_ALGEBRA * exy / (n * m)
        print(f"kmm_numerics: mmd2 {kernel} unbiased={unbiased}: {got['mmd2']:.9e} (float64 {want['mmd2']:.9e}), error {abs(got['mmd2'] - want['mmd2']):.2e}, bound {tol:.2e}")
    pts = np.concatenate([x[:20], y[:17]])
    w = M.mmd_witness(torch.from_numpy(pts), torch.from_numpy(x), torch.from_numpy(y), **args)
    rx, ex = R.kmm64(pts, x, one_n, **_ref_kw(kernel, pts, x))[0], R.error_bound(pts, x, one_n, **_ref_kw(kernel, pts, x))
    ry, ey = R.kmm64(pts, y, one_m, **_ref_kw(kernel, pts, y))[0], R.error_bound(pts, y, one_m, **_ref_kw(kernel, pts, y))
    assert w.shape == (37,) and w.dtype == np.float64
    assert np.all(np.abs(w - M.witness_from_r(rx, ry, n, m)) <= F64_ALGEBRA * (ex[:, 0] / n + ey[:, 0] / m))


def test_kid_against_float64():
    from eegldm import metrics as M
    x, y = _stat_sets()
    n, m = len(x), len(y)
    got = M.kid(torch.from_numpy(x), torch.from_numpy(y), subsets=70, subset_size=1000, seed=4, chunk=128)      # 70 columns: two column groups
    assert got["subset_size"] == 130 and len(got["per_subset"]) == 70
    rng = np.random.default_rng(4)
    ix, iy = M.subset_indicators(n, 130, 70, rng), M.subset_indicators(m, 130, 70, rng)
    kw = _ref_kw("poly", x, y)
    rxx, exx = R.kmm64(x, x, ix, diag_off=0, **kw)[0], R.error_bound(x, x, ix, diag_off=0, **kw)
    ryy, eyy = R.kmm64(y, y, iy, diag_off=0, **kw)[0], R.error_bound(y, y, iy, diag_off=0, **kw)
    rxy, exy = R.kmm64(x, y, iy, **kw)[0], R.error_bound(x, y, iy, **kw)
    want = M.kid_from_r(ix, iy, rxx, ryy, rxy)
    k = 130.0
    tol = F64_ALGEBRA * ((ix * exx).sum(0) / (k * (k - 1)) + (iy * eyy).sum(0) / (k * (k - 1)) + 2 * (ix * exy).sum(0) / (k * k))
    assert np.all(np.abs(np.asarray(got["per_subset"]) - want) <= tol)
    assert got["kid_mean"] == pytest.approx(want.mean(), abs=tol.max()) and got["kid_std"] == pytest.approx(want.std(), abs=2 * tol.max())
    small = M.kid(torch.from_numpy(x), torch.from_numpy(y), subsets=3, subset_size=50, seed=4)
    assert small["subset_size"] == 50 and small == M.kid(torch.from_numpy(x), torch.from_numpy(y), subsets=3, subset_size=50, seed=4)


def _perm_reference(kernel, x, y, seed):
    """float64 statistics of every split, and the bound of the statistic pushed through permutation_stats_from_r."""
    from eegldm import metrics as M
    z = np.concatenate([x, y])
    n, m = len(x), len(y)
    ind = M.permutation_indicators(n, m, 199, seed=seed)
    kw = _ref_kw(kernel, z, z) if kernel == "rbf" else perm_kw(kernel, z)
    r64 = R.kmm64(z, z, ind, diag_off=0, **kw)[0]
    E = R.error_bound(z, z, ind, diag_off=0, **kw)
    a = ind[:, :-1].astype(np.float64)
    # the statistic is linear in R: collect the coefficient of every R[i][a] (rows with a_i = 1) and of every R[i][ones] (a_i = 1 / a_i = 0)
    c_aa, c_a1, c_b1 = 1 / (n * (n - 1)) + 1 / (m * (m - 1)) + 2 / (n * m), 1 / (m * (m - 1)) + 2 / (n * m), 1 / (m * (m - 1))
    bound = c_aa * (a * E[:, :-1]).sum(0) + c_a1 * (a * E[:, -1:]).sum(0) + c_b1 * ((1 - a) * E[:, -1:]).sum(0)
    return M.permutation_stats_from_r(ind, r64, n, m), F64_ALGEBRA * float(bound.max())


@pytest.mark.parametrize("kernel", ["poly", "rbf"])
@pytest.mark.parametrize("seed", PERM_SEEDS)
def test_permutation_test(kernel, seed):
    from eegldm import metrics as M
    args = dict(kernel=kernel, sigmas=(2.0, 4.0, 8.0) if kernel == "rbf" else None, n_perm=199, seed=seed)
    x, y = perm_sets(seed, 0.5)
    got = M.mmd_permutation_test(torch.from_numpy(x), torch.from_numpy(y), **args)
    assert got["p_value"] == 1 / 200 and got["n_perm"] == 199 and len(got["null"]) == 199
    stats, bound = _perm_reference(kernel, x, y, seed)
    assert abs(got["mmd2"] - stats[0]) <= bound and np.all(np.abs(np.asarray(got["null"]) - stats[1:]) <= bound)
    x, y = perm_sets(seed, 0.0)
    got = M.mmd_permutation_test(torch.from_numpy(x), torch.from_numpy(y), **args)
    stats, bound = _perm_reference(kernel, x, y, seed)
    uncertain = int(np.sum(np.abs(stats[1:] - stats[0]) <= 2 * bound))
    assert uncertain <= 5, f"{uncertain} of 199 null values sit within twice the bound of the observed value -- other seeds are needed"
    count_ref = int(np.sum(stats[1:] >= stats[0]))
    count_dev = round(got["p_value"] * 200) - 1
    print(f"kmm_numerics: permutation {kernel} seed {seed}: p {got['p_value']:.4f} (float64 {(1 + count_ref) / 200:.4f}), bound {bound:.2e}, {uncertain} uncertain")
    assert abs(count_dev - count_ref) <= uncertain
    assert np.all(np.abs(np.asarray(got["null"]) - stats[1:]) <= bound)


# ------------------------------------------------------------------------------------------------ 7. the script
def test_two_sample_script_round_trip(tmp_path):
    from eegldm.entry import two_sample as T
    from eegldm.entry.common import synthetic_windows
    hold = synthetic_windows(40, seed=2)                      # (40, 1, 3072), zero pads
    syn = synthetic_windows(12, seed=3)[:, :, 36:-36].copy()  # (12, 1, 3000), as the samplers write them
    os.makedirs(tmp_path / "syn")
    np.save(tmp_path / "syn" / "sample_0.npy", syn[:5]); np.save(tmp_path / "syn" / "sample_1.npy", syn[5:])
    np.save(tmp_path / "hold.npy", hold)
    out = str(tmp_path / "two_sample.json")
    res = T.main(T.parse_args(["--samples", str(tmp_path / "syn" / "sample_*.npy"), "--holdout_npy", str(tmp_path / "hold.npy"), "--n_perm", "49",
                               "--kid_subsets", "5", "--kid_subset_size", "10", "--witness_top", "4", "--seed", "1", "--output", out]))
    with open(out) as f:
        back = json.load(f)
    assert back == json.loads(json.dumps(res))
    assert back["n_real"] == 40 and back["n_synthetic"] == 12 and back["space"] == "features" and back["kernel"] == "poly" and len(back["files"]) == 2
    for block, n, m in (("real_vs_synthetic", 40, 12), ("real_vs_real", 20, 20)):
        b = back[block]
        assert set(b) == {"kid_mean", "kid_std", "kid_subset_size", "mmd2", "p_value", "n", "m"} and (b["n"], b["m"]) == (n, m)
        assert all(np.isfinite(b[k]) for k in ("kid_mean", "kid_std", "mmd2")) and 1 / 50 <= b["p_value"] <= 1.0 and b["kid_subset_size"] == 10
    w = back["witness"]
    assert len(w["index"]) == 4 and len(set(w["index"])) == 4 and all(0 <= i < 12 for i in w["index"]) and w["value"] == sorted(w["value"])
    assert "not evidence" in back["caveat"] and "safe to release" in back["caveat"]
    sig = T.main(T.parse_args(["--samples", str(tmp_path / "syn" / "sample_*.npy"), "--holdout_npy", str(tmp_path / "hold.npy"), "--space", "signal",
                               "--kernel", "rbf", "--n_perm", "19", "--kid_subsets", "2", "--kid_subset_size", "8", "--output", out]))
    assert sig["dim"] == 3000 and len(sig["sigmas"]) == 3 and len(sig["witness"]["index"]) == 12 and 1 / 20 <= sig["real_vs_real"]["p_value"] <= 1.0
