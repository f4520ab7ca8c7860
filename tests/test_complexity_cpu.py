"""No device: the refusals of the Python layer of the signal-complexity metrics (each a ValueError before a context is created), the references
of tests/complexity_reference.py against the literal definitions, and the host algebra on known tables."""
import math

import numpy as np
import pytest
import torch

import complexity_reference as R


@pytest.fixture()
def no_context(monkeypatch):
    """Any attempt to create or fetch a context fails the test: a refusal has to come first."""
    from eegldm import metrics as M

    def boom(*_a, **_k):
        raise AssertionError("the device was touched before the argument was refused")
    monkeypatch.setattr(M, "default_context", boom)
    return M


def test_python_layer_refusals(no_context):
    M = no_context
    w = torch.zeros(4, 300)
    bad = {
        "moments 1-D": lambda: M.row_moments(torch.zeros(300)),
        "moments 4-D": lambda: M.row_moments(torch.zeros(2, 2, 2, 30)),
        "moments two channels": lambda: M.row_moments(torch.zeros(2, 2, 30)),
        "moments L 0": lambda: M.row_moments(torch.zeros(4, 0)),
        "moments L 4097": lambda: M.row_moments(torch.zeros(2, 4097)),
        "hjorth L 2": lambda: M.hjorth(torch.zeros(4, 2)),
        "hjorth table L 2": lambda: M.hjorth_from_moments(np.zeros((1, 8)), 2),
        "ordinal order 1": lambda: M.ordinal_counts(w, order=1),
        "ordinal order 7": lambda: M.ordinal_counts(w, order=7),
        "ordinal order 2.5": lambda: M.ordinal_counts(w, order=2.5),
        "ordinal delay 0": lambda: M.ordinal_counts(w, delay=0),
        "ordinal delay -1": lambda: M.ordinal_counts(w, delay=-1),
        "ordinal no position": lambda: M.ordinal_counts(w, order=4, delay=100),
        "ordinal L 4097": lambda: M.ordinal_counts(torch.zeros(2, 4097)),
        "pe order 7": lambda: M.permutation_entropy(w, order=7),
        "pe counts 1-D": lambda: M.permutation_entropy_from_counts(np.zeros(6)),
        "tm no r": lambda: M.template_match_counts(w, m=2),
        "tm m 0": lambda: M.template_match_counts(w, m=0, r=0.1),
        "tm m 5": lambda: M.template_match_counts(w, m=5, r=0.1),
        "tm scale 0": lambda: M.template_match_counts(w, r=0.1, scale=0),
        "tm scale 65": lambda: M.template_match_counts(w, r=0.1, scale=65),
        "tm scale 1.5": lambda: M.template_match_counts(w, r=0.1, scale=1.5),
        "tm too few templates": lambda: M.template_match_counts(w, m=4, r=0.1, scale=60),
        "tm r 0": lambda: M.template_match_counts(w, r=0.0),
        "tm r < 0": lambda: M.template_match_counts(w, r=-0.1),
        "tm r nan": lambda: M.template_match_counts(w, r=float("nan")),
        "tm r inf": lambda: M.template_match_counts(w, r=float("inf")),
        "tm r beyond fp32": lambda: M.template_match_counts(w, r=1e39),
        "tm r shape": lambda: M.template_match_counts(w, r=np.full(3, 0.1)),
        "tm r one bad": lambda: M.template_match_counts(w, r=np.array([0.1, 0.1, 0.0, 0.1])),
        "tm L 4097": lambda: M.template_match_counts(torch.zeros(2, 4097), r=0.1),
        "se r_mode": lambda: M.sample_entropy(w, r_mode="var"),
        "se r 0": lambda: M.sample_entropy(w, r=0.0),
        "se r nan": lambda: M.sample_entropy(w, r=float("nan")),
        "se r vector": lambda: M.sample_entropy(w, r=np.full(4, 0.2)),
        "se m 5": lambda: M.sample_entropy(w, m=5),
        "se scale 65": lambda: M.sample_entropy(w, scales=(1, 65)),
        "se scale too coarse": lambda: M.sample_entropy(w, m=3, scales=(1, 64)),
        "se no scale": lambda: M.sample_entropy(w, scales=()),
        "se counts shape": lambda: M.sample_entropy_from_counts(np.zeros((4, 3))),
        "features order": lambda: M.complexity_features(w, orders=(3, 7)),
        "features scale": lambda: M.complexity_features(w, scales=(1, 100)),
        "features r": lambda: M.complexity_features(w, r=-1.0),
        "features r_mode": lambda: M.complexity_features(w, r_mode="x"),
        "features L 2": lambda: M.complexity_features(torch.zeros(4, 2)),
        "compare widths": lambda: M.compare_features(np.zeros((4, 3)), np.zeros((4, 2)), ["a", "b", "c"]),
        "compare names": lambda: M.compare_features(np.zeros((4, 3)), np.zeros((4, 3)), ["a", "b"]),
    }
    for name, call in bad.items():
        try:
            call()
        except ValueError:
            continue
        pytest.fail(f"{name}: accepted")


def test_lagwise_counter_equals_the_double_loop():
    rng = np.random.default_rng(5)
    rows = {"gauss": (rng.standard_normal(40).astype(np.float32), 0.4), "integers": (rng.integers(0, 4, 40).astype(np.float32), 1.0),
            "constant": (np.full(40, 2.5, np.float32), 0.0), "nan inside": (rng.standard_normal(40).astype(np.float32), 0.5),
            "inf ends": (rng.integers(0, 3, 40).astype(np.float32), 1.0), "r inf": (rng.standard_normal(40).astype(np.float32), np.inf),
            "r nan": (rng.standard_normal(40).astype(np.float32), np.nan)}
    rows["nan inside"][0][17] = np.nan
    rows["inf ends"][0][0] = np.inf; rows["inf ends"][0][39] = -np.inf; rows["inf ends"][0][20] = np.inf
    for name, (x, r) in rows.items():
        for m in (1, 2, 3, 4):
            for scale in (1, 2, 3):
                assert R.template_counts(x, m, scale, r) == R.template_counts_pairs(x, m, scale, r), (name, m, scale)
    # the largest count: every pair of a constant row matches, at both lengths over the same N - m templates
    for m in (1, 2, 3, 4):
        t = 40 - m
        assert R.template_counts(rows["constant"][0], m, 1, 0.0) == (t * (t - 1) // 2, t * (t - 1) // 2)
    # the last sample enters A only
    x = rows["integers"][0].copy(); y = x.copy(); y[-1] = 100.0
    bx, ax = R.template_counts(x, 2, 1, 1.0); by, ay = R.template_counts(y, 2, 1, 1.0)
    assert bx == by and ay < ax
    # coarse-graining: scale 1 compares as x, the tail past N * scale is not read
    assert np.array_equal(R.coarse_grain(x, 1), x) and np.array_equal(R.coarse_grain(x[:39], 3), R.coarse_grain(x[:41], 3)[:13])
    assert np.array_equal(R.coarse_grain(np.array([1, 2, 4, 8, 16, 32, 64], np.float32), 3), np.array([7, 56], np.float32) / np.float32(3))


@pytest.mark.parametrize("order", [2, 3, 4, 5, 6])
def test_lehmer_index_is_a_bijection(order):
    import itertools
    idx = [R.lehmer_index(p) for p in itertools.permutations(range(order))]
    assert sorted(idx) == list(range(math.factorial(order)))
    assert R.lehmer_index(range(order)) == 0 and R.lehmer_index(range(order)[::-1]) == math.factorial(order) - 1
    # ties rank by position: all-equal is the ascending pattern, and so are signed zeros
    assert R.lehmer_index([3.0] * order) == 0
    assert R.lehmer_index(([0.0, -0.0] * 3)[:order]) == 0
    if order >= 3:
        assert R.lehmer_index([1.0, 1.0, 0.0][:order] + [5.0] * (order - 3)) == R.lehmer_index([1.0, 2.0, 0.0][:order] + [5.0] * (order - 3))
    # the vectorised histogram is the per-position index
    rng = np.random.default_rng(order)
    x = rng.integers(0, 3, (2, 50)).astype(np.float32)
    for delay in (1, 3):
        c, s = R.ordinal_counts(x, order, delay)
        P = 50 - (order - 1) * delay
        want = np.zeros_like(c)
        for b in range(2):
            for p in range(P):
                want[b, R.lehmer_index(x[b, p:p + (order - 1) * delay + 1:delay])] += 1
        assert np.array_equal(c, want) and not s.any()
    x[0, 10] = np.nan; x[1, 0] = np.inf
    c, s = R.ordinal_counts(x, order, 1)
    assert s[0] == order and s[1] == 1 and np.all(c.sum(1) + s == 50 - (order - 1))


def test_host_algebra_on_known_tables():
    from eegldm import metrics as M
    # a monotone ramp has one pattern: permutation entropy 0, in both the reference and the product's algebra
    ramp = np.arange(100, dtype=np.float32)[None, :]
    for order in (2, 3, 6):
        c, s = R.ordinal_counts(ramp, order, 1)
        assert c[0, 0] == 100 - (order - 1) and c[0, 1:].sum() == 0 and s[0] == 0
        assert M.permutation_entropy_from_counts(c)[0] == 0.0 and M.permutation_entropy_from_counts(c, normalize=False)[0] == 0.0
    # uniform counts: ln(order!) unnormalised, 1 normalised; no counted position: NaN
    assert abs(M.permutation_entropy_from_counts(np.full((1, 24), 7), normalize=False)[0] - math.log(24)) < 1e-14
    assert abs(M.permutation_entropy_from_counts(np.full((1, 24), 7))[0] - 1.0) < 1e-14
    assert np.isnan(M.permutation_entropy_from_counts(np.zeros((1, 6)))[0])
    rng = np.random.default_rng(0)
    c = rng.integers(0, 50, (5, 120))
    assert np.allclose(M.permutation_entropy_from_counts(c), R.permutation_entropy(c), rtol=0, atol=1e-14)
    # a constant row: every pair matches at both lengths, A == B, SampEn 0
    b, a = R.template_counts(np.full(64, -1.5, np.float32), 2, 1, 0.0)
    assert a == b == 62 * 61 // 2
    se = M.sample_entropy_from_counts(np.array([[b, a], [0, 0], [10, 0], [10, 5]]))
    assert se[0] == 0.0 and np.isnan(se[1]) and se[2] == np.inf and abs(se[3] - math.log(2.0)) < 1e-15
    assert np.array_equal(se, R.sample_entropy(np.array([[b, a], [0, 0], [10, 0], [10, 5]])), equal_nan=True)
    assert M.sample_entropy_from_counts(np.zeros((3, 2, 2))).shape == (3, 2)


def test_hjorth_of_a_sine():
    """A sine of frequency f sampled at fs: d1 is a sine of amplitude a = 2 sin(pi f / fs) times the signal's, d2 one of a^2 times: mobility a and
    complexity 1.  The table holds the sums of squares over whole periods, m2 = amplitude^2 / 2 per term, and the algebra returns a to 1e-9.
    The moments of a FINITE window are not that table: its d1 has L - 1 terms that do not close the last period, which moves the mobility by up
    to about 1 / L of itself (derived: one term of at most a^2 is missing from a sum of a^2 (L - 1) / 2, and the count changes by one); the
    float64 reference on L = 3000 samples is held to 2 / L."""
    from eegldm import metrics as M
    for f, fs, L in ((1.0, 100.0, 3000), (12.5, 100.0, 4096), (0.3, 128.0, 1000)):
        a = 2.0 * math.sin(math.pi * f / fs)
        amp = 3.7
        table = np.array([[0.0, L * amp ** 2 / 2, (L - 1) * (amp * a) ** 2 / 2, (L - 2) * (amp * a * a) ** 2 / 2, 0.0, 0.0, -amp, amp]])
        h = M.hjorth_from_moments(table, L)
        assert abs(h[0, 0] - amp ** 2 / 2) < 1e-12 and abs(h[0, 1] - a) < 1e-9 and abs(h[0, 2] - 1.0) < 1e-9
    x = np.sin(2 * np.pi * 1.0 * np.arange(3000) / 100.0 + 0.3).astype(np.float32)[None, :]
    h = M.hjorth_from_moments(R.row_moments(x), 3000)
    a = 2.0 * math.sin(math.pi / 100.0)
    assert abs(h[0, 1] / a - 1.0) < 2.0 / 3000 and abs(h[0, 2] - 1.0) < 4.0 / 3000 and abs(h[0, 0] - 0.5) < 1e-6
    # a constant row has no variance: NaN, not an exception
    assert np.all(np.isnan(M.hjorth_from_moments(R.row_moments(np.ones((1, 10), np.float32)), 10)[0, 1:]))


def test_moments_reference_and_bound():
    rng = np.random.default_rng(1)
    x = (100.0 + rng.standard_normal((3, 500))).astype(np.float32)
    m, b = R.row_moments(x), R.moments_bound(x)
    x64 = x.astype(np.float64)
    # against exact rational arithmetic on one row: the float64 two-pass evaluation sits far inside its own bound
    from fractions import Fraction
    fr = [Fraction(float(v)) for v in x[0]]
    mean = sum(fr) / len(fr)
    m2 = sum((v - mean) ** 2 for v in fr)
    assert abs(Fraction(m[0, 0]) - mean) <= Fraction(b[0, 0]) and abs(Fraction(m[0, 1]) - m2) <= Fraction(b[0, 1])
    assert b[0, 1] < 1e-11 * m[0, 1] and np.all(b[:, 5:] == 0)
    assert np.array_equal(m[:, 6], x.min(1)) and np.array_equal(m[:, 7], x.max(1))
    assert np.allclose(m[:, 4], np.abs(np.diff(x64, axis=1)).sum(1), rtol=1e-14) and R.sign_changes_safe(x).all()
    # integer rows: exact, whatever the order of the sums
    for L in (6, 64, 3000):
        xi = R.integer_row(rng, L)
        t = R.row_moments(xi[None])[0]
        assert xi.sum() == 0 and t[0] == 0.0 and t[1] == float(np.sum(xi.astype(np.int64) ** 2))
        assert t[2] == float(np.sum(np.diff(xi.astype(np.int64)) ** 2)) and t[3] == float(np.sum(np.diff(xi.astype(np.int64), 2) ** 2))
    # L = 1, 2: empty and one-element differences give 0
    assert np.array_equal(R.row_moments(np.array([[2.0]], np.float32))[0], [2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 2.0])
    assert np.array_equal(R.row_moments(np.array([[2.0, 5.0]], np.float32))[0], [3.5, 4.5, 0.0, 0.0, 3.0, 1.0, 2.0, 5.0])


def test_compare_features_counts_non_finite_values():
    from eegldm import metrics as M
    a = np.array([[0.0, 1.0], [1.0, np.nan], [2.0, np.inf], [3.0, 2.0]])
    b = np.array([[0.5, np.nan], [1.5, np.nan]])
    out = M.compare_features(a, b, ["u", "v"])
    assert out["u"]["n_real"] == 4 and out["u"]["n_synthetic"] == 2 and out["u"]["n_real_nonfinite"] == 0
    assert out["u"]["ks"] == M.ks_statistic(a[:, 0], b[:, 0]) and out["u"]["wasserstein"] == M.wasserstein_1d(a[:, 0], b[:, 0])
    assert out["v"] == {"n_real": 2, "n_synthetic": 0, "n_real_nonfinite": 2, "n_synthetic_nonfinite": 2, "ks": None, "wasserstein": None}
    assert M.complexity_feature_names((3,), (1, 20)) == ["activity", "mobility", "complexity", "sign_change_rate", "line_length_per_sample",
                                                           "perm_entropy_o3", "sample_entropy_s1", "sample_entropy_s20"]
