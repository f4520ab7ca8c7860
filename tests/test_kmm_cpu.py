"""CPU: everything of the kernel two-sample statistics that needs no device -- the refusals, the indicator and permutation builders, the
float64 algebra that turns R = K V into MMD^2 / KID / permutation nulls / p-values (against the direct O(N^2) definitions of
tests/kmm_reference.py), the reference's own bound, the seeds the GPU permutation test relies on, and the header."""
import os
import re

import numpy as np
import pytest
import torch

import kmm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_come_before_the_device():
    from eegldm import metrics as M
    x, y = torch.zeros(4, 8), torch.zeros(6, 8)
    calls = {
        "mmd2": lambda a, b, **kw: M.mmd2(a, b, **kw),
        "kid": lambda a, b, **kw: M.kid(a, b, **{k: v for k, v in kw.items() if k not in ("kernel", "sigmas", "degree")}),
        "perm": lambda a, b, **kw: M.mmd_permutation_test(a, b, **kw),
        "witness": lambda a, b, **kw: M.mmd_witness(a, a, b, **kw),
        "bandwidth": lambda a, b, **kw: M.median_bandwidth(a, b),
    }
    for name, fn in calls.items():
        with pytest.raises(ValueError, match="feature dimensions differ"):
            fn(x, torch.zeros(6, 7))
        for bad in (torch.zeros(8), torch.zeros(2, 3, 8)):
            with pytest.raises(ValueError, match="2-D"):
                fn(bad, y)
            with pytest.raises(ValueError, match="2-D"):
                fn(x, bad)
        if name != "bandwidth":
            with pytest.raises(ValueError, match="at least 2 rows"):
                fn(torch.zeros(1, 8), y)
            with pytest.raises(ValueError, match="at least 2 rows"):
                fn(x, torch.zeros(1, 8))
    for name in ("mmd2", "perm", "witness"):
        fn = calls[name]
        with pytest.raises(ValueError, match="kernel must be"):
            fn(x, y, kernel="laplace")
        with pytest.raises(ValueError, match="sigmas"):
            fn(x, y, kernel="rbf", sigmas=())
        with pytest.raises(ValueError, match="sigmas"):
            fn(x, y, kernel="rbf", sigmas=tuple(range(1, 10)))
        with pytest.raises(ValueError, match="positive"):
            fn(x, y, kernel="rbf", sigmas=(1.0, 0.0))
        for deg in (0, 5, 2.5):
            with pytest.raises(ValueError, match="degree"):
                fn(x, y, kernel="poly", degree=deg)
    for n_perm in (0, -3):
        with pytest.raises(ValueError, match="n_perm"):
            M.mmd_permutation_test(x, y, n_perm=n_perm)
    with pytest.raises(ValueError, match="subsets"):
        M.kid(x, y, subsets=0)
    with pytest.raises(ValueError, match="subset_size"):
        M.kid(x, y, subset_size=1)
    v = torch.ones(6, 3)
    with pytest.raises(ValueError, match="feature dimensions differ"):
        M.kernel_matmul(x, torch.zeros(6, 7), v)
    with pytest.raises(ValueError, match="2-D"):
        M.kernel_matmul(x, y, torch.ones(6))
    with pytest.raises(ValueError, match="rows"):
        M.kernel_matmul(x, y, torch.ones(5, 3))
    with pytest.raises(ValueError, match="empty"):
        M.kernel_matmul(torch.zeros(0, 8), y, v)
    with pytest.raises(ValueError, match="kernel must be"):
        M.kernel_matmul(x, y, v, kernel="cosine")
    with pytest.raises(ValueError, match="chunk"):
        M.kernel_matmul(x, y, v, chunk=0)
    with pytest.raises(ValueError, match="sigmas"):
        M.kernel_matmul(x, y, v, kernel="rbf", sigmas=[])
    with pytest.raises(ValueError, match="points"):
        M.mmd_witness(torch.zeros(3, 7), x, y)


def test_builders_are_reproducible_from_the_seed():
    from eegldm.metrics import permutation_indicators, subset_indicators
    a = subset_indicators(50, 20, 7, np.random.default_rng(3))
    b = subset_indicators(50, 20, 7, np.random.default_rng(3))
    assert a.dtype == np.float32 and a.shape == (50, 7) and np.array_equal(a, b)
    assert set(np.unique(a)) == {0.0, 1.0} and np.all(a.sum(0) == 20)
    assert not np.array_equal(a, subset_indicators(50, 20, 7, np.random.default_rng(4)))
    assert np.all(subset_indicators(9, 9, 2, np.random.default_rng(0)) == 1.0)
    with pytest.raises(ValueError):
        subset_indicators(9, 10, 2, np.random.default_rng(0))
    p = permutation_indicators(12, 9, 30, seed=5)
    assert p.shape == (21, 32) and p.dtype == np.float32 and np.array_equal(p, permutation_indicators(12, 9, 30, seed=5))
    assert np.all(p[:12, 0] == 1) and np.all(p[12:, 0] == 0) and np.all(p[:, -1] == 1) and np.all(p[:, :-1].sum(0) == 12)
    assert len({tuple(c) for c in p[:, 1:-1].T}) > 25 and not np.array_equal(p, permutation_indicators(12, 9, 30, seed=6))
    with pytest.raises(ValueError, match="n_perm"):
        permutation_indicators(12, 9, 0)


def _sets(seed, n=37, m=29, d=6, shift=0.3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d)).astype(np.float32), (rng.standard_normal((m, d)) + shift).astype(np.float32)


def _kw(kernel, x, y):
    if kernel == "poly":
        return dict(kind="poly", degree=3, gamma=None, coef0=1.0)
    z = np.concatenate([x, y])
    sq = (z.astype(np.float64) ** 2).sum(1).astype(np.float32)
    return dict(kind="rbf", betas=[0.5 / 4.0, 0.5 / 16.0]), sq


@pytest.mark.parametrize("kernel", ["poly", "rbf"])
def test_statistics_from_r_equal_the_direct_definitions(kernel):
    """mmd2_from_sums, kid_from_r and permutation_stats_from_r on float64 R = K V against the O(N^2) definitions on the full matrices:
    1e-12 relative (relative to the size of the terms a statistic is the difference of)."""
    from eegldm import metrics as M
    x, y = _sets(1)
    n, m = len(x), len(y)
    z = np.concatenate([x, y])
    if kernel == "poly":
        kw, sq = _kw(kernel, x, y), None
        kzz = R.kernel64(z, z, **kw)
    else:
        kw, sq = _kw(kernel, x, y)
        kzz = R.kernel64(z, z, asq=sq, bsq=sq, **kw)
    kxx, kyy, kxy = kzz[:n, :n], kzz[n:, n:], kzz[:n, n:]
    scale = np.abs(kzz).mean()
    for unbiased in (True, False):
        mx = (1.0 - np.eye(n)) if unbiased else 1.0
        my = (1.0 - np.eye(m)) if unbiased else 1.0
        got = M.mmd2_from_sums((kxx * mx).sum(), (kyy * my).sum(), kxy.sum(), n, m, unbiased)
        assert abs(got["mmd2"] - R.mmd2_direct(kxx, kyy, kxy, unbiased)) <= 1e-12 * scale
        assert got["mmd2"] == got["kxx"] + got["kyy"] - 2 * got["kxy"] and got["n"] == n and got["m"] == m
    # KID subsets
    rng = np.random.default_rng(0)
    ix, iy = M.subset_indicators(n, 20, 9, rng), M.subset_indicators(m, 20, 9, rng)
    k0x, k0y = kxx * (1.0 - np.eye(n)), kyy * (1.0 - np.eye(m))
    per = M.kid_from_r(ix, iy, k0x @ ix, k0y @ iy, kxy @ iy)
    for s in range(9):
        sx, sy = np.nonzero(ix[:, s])[0], np.nonzero(iy[:, s])[0]
        want = R.mmd2_direct(kxx[np.ix_(sx, sx)], kyy[np.ix_(sy, sy)], kxy[np.ix_(sx, sy)])
        assert abs(per[s] - want) <= 1e-12 * scale
    # permutation nulls
    ind = M.permutation_indicators(n, m, 40, seed=2)
    stats = M.permutation_stats_from_r(ind, (kzz * (1.0 - np.eye(n + m))) @ ind.astype(np.float64), n, m)
    assert stats.shape == (41,)
    for c in range(41):
        assert abs(stats[c] - R.split_mmd2_direct(kzz, ind[:, c] > 0)) <= 1e-12 * scale
    assert abs(stats[0] - R.mmd2_direct(kxx, kyy, kxy)) <= 1e-12 * scale
    # witness
    pts = z[::5]
    kp = R.kernel64(pts, z, **kw) if kernel == "poly" else R.kernel64(pts, z, asq=sq[::5], bsq=sq, **kw)
    w = M.witness_from_r(kp[:, :n].sum(1), kp[:, n:].sum(1), n, m)
    assert np.allclose(w, kp[:, :n].mean(1) - kp[:, n:].mean(1), rtol=0, atol=1e-12 * scale)


def test_p_value_formula():
    from eegldm.metrics import permutation_p_value
    null = np.array([0.1, 0.2, 0.3, 0.3, 0.5])
    assert permutation_p_value(0.3, null) == (1 + 3) / 6          # ties count against the observed value
    assert permutation_p_value(0.6, null) == 1 / 6 and permutation_p_value(-1.0, null) == 1.0
    assert permutation_p_value(0.5, np.zeros(199)) == 1 / 200


def test_reference_and_bound():
    """The reference leaves exactly the requested diagonal out, and its bound covers an fp32 evaluation that follows the kernel's order of
    operations (numpy fp32, one rounding per operation; the dot product in fp32 pairwise order is no worse than the chain the bound counts)."""
    rng = np.random.default_rng(8)
    a, b = rng.standard_normal((5, 7)).astype(np.float32), rng.standard_normal((9, 7)).astype(np.float32)
    v = rng.standard_normal((9, 3)).astype(np.float32)
    full, k = R.kmm64(a, b, v)
    for off in (0, 2, -3):
        r, km = R.kmm64(a, b, v, diag_off=off)
        want = full.copy()
        for i in range(5):
            if 0 <= i + off < 9:
                want[i] -= k[i, i + off] * v[i + off].astype(np.float64)
                assert km[i, i + off] == 0.0
        assert np.allclose(r, want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(R.kmm64(a, b, v, diag_off=R.NO_DIAG)[0], full) and np.array_equal(R.kmm64(a, b, v, diag_off=50)[0], full)
    assert R.kmm64(a, b[:0], v[:0])[0].shape == (5, 3) and not R.kmm64(a, b[:0], v[:0])[0].any()
    asq, bsq = (a * a).sum(1), (b * b).sum(1)
    for kw in (dict(kind="poly", degree=4, gamma=0.3, coef0=0.5), dict(kind="rbf", betas=[0.05, 0.2, 1.0], asq=asq, bsq=bsq)):
        r64, _k = R.kmm64(a, b, v, **kw)
        dot = (a @ b.T).astype(np.float32)
        if kw["kind"] == "poly":
            t = np.float32(0.3) * dot + np.float32(0.5)
            k32 = t * t * t * t
        else:
            d2 = np.maximum(np.float32(0), (asq[:, None] + bsq[None, :]) - np.float32(2) * dot)
            k32 = sum(np.exp((-np.float32(bb) * d2).astype(np.float32)).astype(np.float32) for bb in kw["betas"]) / np.float32(3)
        r32 = (k32.astype(np.float32) @ v).astype(np.float64)
        e = R.error_bound(a, b, v, **kw)
        assert np.all(e > 0) and np.all(np.abs(r32 - r64) <= e) and np.all(e <= 1e-4 * (np.abs(_k) @ np.abs(v)) + 1e-30)
    nan_b = b.copy(); nan_b[4] = np.nan
    assert np.isnan(R.kmm64(a, nan_b, np.zeros_like(v))[0]).all()              # NaN * 0: K @ V poisons every column
    assert R.slab_rows(1000) == 128 and R.slab_rows(4233) == 256 and R.slab_rows(4096) == 128 and R.slab_rows(4097) == 256


PERM_SEEDS = (11, 12, 13)


def perm_sets(seed, shift):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((96, 16)).astype(np.float32)
    y = (rng.standard_normal((80, 16)) + shift).astype(np.float32)
    return x, y


def perm_kw(kernel, z):
    if kernel == "poly":
        return dict(kind="poly", degree=3, gamma=None, coef0=1.0)
    sq = (z.astype(np.float64) ** 2).sum(1).astype(np.float32)
    return dict(kind="rbf", betas=[1.0 / (2.0 * s * s) for s in (2.0, 4.0, 8.0)], asq=sq, bsq=sq)


@pytest.mark.parametrize("kernel", ["poly", "rbf"])
@pytest.mark.parametrize("seed", PERM_SEEDS)
def test_permutation_seeds_in_float64(kernel, seed):
    """What tests/test_gpu_kmm.py relies on, in float64: with shift 0.5 the observed value exceeds every null value by more than 0.9 (poly) /
    0.04 (rbf), so p = 1 / 200 whatever the device's rounding; with shift 0 the p-value is unremarkable."""
    from eegldm import metrics as M
    margin = {"poly": 0.9, "rbf": 0.04}[kernel]
    x, y = perm_sets(seed, 0.5)
    z = np.concatenate([x, y])
    ind = M.permutation_indicators(96, 80, 199, seed=seed)
    kzz = R.kernel64(z, z, **perm_kw(kernel, z))
    stats = M.permutation_stats_from_r(ind, (kzz * (1.0 - np.eye(176))) @ ind.astype(np.float64), 96, 80)
    assert stats[0] - stats[1:].max() > margin, (stats[0], stats[1:].max())
    assert M.permutation_p_value(stats[0], stats[1:]) == 1 / 200
    x, y = perm_sets(seed, 0.0)
    z = np.concatenate([x, y])
    kzz = R.kernel64(z, z, **perm_kw(kernel, z))
    stats = M.permutation_stats_from_r(ind, (kzz * (1.0 - np.eye(176))) @ ind.astype(np.float64), 96, 80)
    p = M.permutation_p_value(stats[0], stats[1:])
    print(f"seed {seed} {kernel}: shift 0 p = {p:.3f}, nearest null at {np.abs(stats[1:] - stats[0]).min() / np.abs(kzz).mean():.2e} of mean |k|")
    assert 0.05 < p < 0.95


def test_header_declares_the_export_and_abi_8():
    src = open(os.path.join(ROOT, "include", "eegldm.h")).read()
    assert re.search(r"#define\s+EEGLDM_ABI_VERSION\s+8\b", src)
    assert re.search(r"#define\s+EEGLDM_KMM_NO_DIAG\s+\(-0x7fffffffffffffffL - 1\)", src)
    assert "int eegldm_kernel_matmul(eegldm_ctx*" in src
    from eegldm._lib import SIGNATURES, lib
    from eegldm.metrics import KMM_NO_DIAG
    assert len(SIGNATURES["eegldm_kernel_matmul"]) == 23 and hasattr(lib, "eegldm_kernel_matmul") and KMM_NO_DIAG == R.NO_DIAG == -2 ** 63
    assert lib.eegldm_abi_version() == 8
    args = [None, None, 0, None, None, 0, None, None, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, None, 0, 0, 0, None, 0]
    assert lib.eegldm_kernel_matmul(*args) != 0 and b"null argument" in lib.eegldm_last_error()           # argument check, no device
