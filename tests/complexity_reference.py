"""Integer and float64 numpy references of the three primitives of csrc/complexity.hip, and the operation-count bound the moments are held to.
Shared by tests/test_complexity_cpu.py and tests/test_gpu_complexity.py.

eegldm_template_matches and eegldm_ordinal_counts have INTEGER results built on exact fp32 comparisons: `template_counts` (lag by lag) and
`ordinal_counts` below are the definitions, and the device must equal them in every integer.  `template_counts_pairs` is the definition of the
pair counts as a literal double loop over the template pairs; tests/test_complexity_cpu.py holds the lag-wise counter to it.  The fp32 parts of
the definition are done in fp32 here as on the device, each one correctly rounded IEEE operation on the same operands, so that they are THE SAME
numbers: the coarse-graining sum in ascending order from +0 and its one divide, and the one subtraction |a - b| before the comparison with r.

eegldm_row_moments.  `row_moments` evaluates the definition in float64 numpy FROM THE fp32 SAMPLES, two passes: v is x, d1 = diff(x) or d2 =
diff(d1) (each difference one correctly rounded float64 subtraction on the same operands as on the device: the terms v are the same numbers on
both sides), mean_v = sum(v) / n, m2_v = sum((v - mean_v)^2).  The device sums in another order (a chain per thread, a butterfly, the waves),
numpy pairwise.  Error bound (`moments_bound`), u = 2^-53, g(k) = k u / (1 - k u) (Higham, lemma 3.1), n the number of terms:

* a sum of n terms in any order:                                   |s^ - s| <= g(n - 1) sum |v|
* mean = fl(s^ / n), one more rounding:                            |mean^ - mean| <= g(n) sum |v| / n =: delta_v
  two evaluations differ by at most                                e_mean = 2 delta_x
* line_length = sum |d1| (|.| is exact):                           e_ll = 2 g(n) sum |d1|
* m2 about the COMPUTED mean: a term fl(fl(v - mean^)^2) carries three roundings (two if the square is fused into the sum), the sum n - 1:
                                                                   |m2^ - S(mean^)| <= g(n + 2) S(mean^),   S(c) = sum (v - c)^2 = m2 + n (c - mean)^2
  so S(mean^) <= m2 + n delta_v^2, and two evaluations, each with its own computed mean, differ by at most
                                                                   e_m2 = 2 g(n + 2) (m2 + n delta_v^2) + n delta_v^2
  with m2 the reference's value.  The second term is why the mean is taken first: it is of second order in the mean's error (a one-pass
  sum x^2 - n mean^2 would lose everything at a row mean of 100 standard deviations in fp32, and still 10^4 of the 10^16 in float64).
* min and max are exact fp32 comparisons; both are NaN when the row holds a NaN.
* sign_changes counts sign flips of c = x - mean^ and is exact unless a sample lies within delta_x of the mean; `sign_changes_safe` says whether
  a row has no such sample, and the tests' rows are asserted to have none.

Small integers: when every sample is an integer, the row sum is zero and d1 and d2 sum to zero too, every term and every partial sum is an
integer below 2^53: the two evaluations agree in every bit (tests/test_gpu_complexity.py demands that).
"""
import math

import numpy as np

U64 = 2.0 ** -53
MAX_L, MAX_ORDER, MAX_M, MAX_SCALE = 4096, 6, 4, 64
MOMENT_FIELDS = ("mean", "m2_x", "m2_d1", "m2_d2", "line_length", "sign_changes", "min", "max")
PLANT_SEEDS = (0, 1, 2, 3, 4)


def g(k):
    return k * U64 / (1.0 - k * U64)


# ---------------------------------------------------------------------------------------------------- template matches
def coarse_grain(x, scale):
    """(L,) fp32 -> (L // scale,) fp32: y[j] = (x[j s] + ... + x[j s + s - 1]) / (float)s, the sum in fp32 in ascending order from +0."""
    x = np.asarray(x, np.float32)
    n = x.size // scale
    blocks = x[:n * scale].reshape(n, scale)
    acc = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for k in range(scale):
            acc = acc + blocks[:, k]
        return acc / np.float32(scale)


def template_counts_pairs(x, m, scale, r):
    """(B, A) by the definition, a double loop over the pairs i < j of templates in [0, N - m): B counts the pairs with |y[i+k] - y[j+k]| <= r
    for all k < m, A those where it also holds at k = m."""
    y = coarse_grain(x, scale)
    r = np.float32(r)
    t = y.size - m
    cb = ca = 0
    with np.errstate(all="ignore"):
        for i in range(t):
            for j in range(i + 1, t):
                ok = all(bool(np.abs(y[i + k] - y[j + k]) <= r) for k in range(m))
                cb += ok
                ca += ok and bool(np.abs(y[i + m] - y[j + m]) <= r)
    return int(cb), int(ca)


def template_counts(x, m, scale, r):
    """(B, A) lag by lag: for d = j - i the pair (i, i + d), i < T - d, matches at length m iff e_d[n] = |y[n] - y[n + d]| <= r holds for
    n = i .. i + m - 1, at length m + 1 iff also at n = i + m; windows of consecutive true values are counted through a running sum."""
    c = template_counts_rows(np.asarray(x, np.float32)[None, :], m, scale, [r])
    return int(c[0, 0]), int(c[0, 1])


def template_counts_rows(x, m, scale, r):
    """(B, 2) int64 = (B, A) of rows x (B, L) with tolerances r (B,): `template_counts`, every row at once per lag."""
    x = np.asarray(x, np.float32)
    y = np.stack([coarse_grain(row, scale) for row in x])
    r = np.asarray(r, np.float32).reshape(-1, 1)
    assert r.shape[0] == x.shape[0]
    n = y.shape[1]
    t = n - m
    assert t >= 2
    out = np.zeros((x.shape[0], 2), np.int64)
    zero = np.zeros((x.shape[0], 1), np.int64)
    with np.errstate(all="ignore"):
        for d in range(1, t):
            e = np.abs(y[:, :n - d] - y[:, d:]) <= r                 # fp32 subtraction, one rounding
            c = np.concatenate([zero, np.cumsum(e, 1)], 1)           # c[k] = trues among e[0 .. k)
            out[:, 0] += np.sum(c[:, m:t - d + m] - c[:, :t - d] == m, 1)
            out[:, 1] += np.sum(c[:, m + 1:t - d + m + 1] - c[:, :t - d] == m + 1, 1)
    return out


def sample_entropy(counts):
    """-ln(A / B) of (..., 2) = (B, A): NaN where B == 0, +inf where A == 0 < B."""
    c = np.asarray(counts, np.float64)
    out = np.full(c.shape[:-1], np.nan)
    b, a = c[..., 0], c[..., 1]
    out[(b > 0) & (a == 0)] = np.inf
    ok = (b > 0) & (a > 0)
    out[ok] = -np.log(a[ok] / b[ok])
    return out


# ---------------------------------------------------------------------------------------------------- ordinal patterns
def lehmer_index(v):
    """Pattern index of one vector: sum_k c_k (order - 1 - k)!, c_k = #{l > k : v_l < v_k} by exact `<` (ties rank by position)."""
    v = np.asarray(v, np.float32)
    n = v.size
    return int(sum(sum(1 for l in range(k + 1, n) if v[l] < v[k]) * math.factorial(n - 1 - k) for k in range(n)))


def ordinal_counts(x, order, delay):
    """(counts (B, order!) int32, skipped (B,) int32) of rows x (B, L)."""
    x = np.asarray(x, np.float32)
    B, L = x.shape
    P = L - (order - 1) * delay
    assert P >= 1
    nb = math.factorial(order)
    counts, skipped = np.zeros((B, nb), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        V = np.stack([x[b, k * delay:k * delay + P] for k in range(order)])      # (order, P)
        fin = np.all(np.isfinite(V), 0)
        idx = np.zeros(P, np.int64)
        with np.errstate(invalid="ignore"):
            for k in range(order):
                ck = np.zeros(P, np.int64)
                for l in range(k + 1, order):
                    ck += V[l] < V[k]
                idx += ck * math.factorial(order - 1 - k)
        counts[b] = np.bincount(idx[fin], minlength=nb)
        skipped[b] = P - int(fin.sum())
    return counts, skipped


def permutation_entropy(counts, normalize=True):
    c = np.asarray(counts, np.float64)
    p = c / c.sum(1, keepdims=True)
    h = -np.sum(np.where(c > 0, p * np.log(np.where(c > 0, p, 1.0)), 0.0), 1)
    return h / np.log(c.shape[1]) if normalize else h


# ---------------------------------------------------------------------------------------------------- moments
def _terms(row):
    x = np.asarray(row, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d1 = np.diff(x)
        d2 = np.diff(d1)
    return x, d1, d2


def _mean_m2(v):
    if v.size == 0:
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        mean = np.sum(v) / v.size
        c = v - mean
        return float(mean), float(np.sum(c * c))


def row_moments(x):
    """(B, 8) float64, columns MOMENT_FIELDS, of rows x (B, L) fp32: two passes in float64."""
    x = np.asarray(x, np.float32)
    out = np.zeros((x.shape[0], 8))
    for b, row in enumerate(x):
        v, d1, d2 = _terms(row)
        mean, m2 = _mean_m2(v)
        with np.errstate(all="ignore"):
            neg = (v - mean) < 0
            out[b] = (mean, m2, _mean_m2(d1)[1], _mean_m2(d2)[1], np.sum(np.abs(d1)), np.sum(neg[1:] != neg[:-1]), np.min(row), np.max(row))
    return out


def moments_bound(x):
    """(B, 8): the most two float64 evaluations of the definition may differ by, per column (0 where the column is exact); see the docstring."""
    x = np.asarray(x, np.float32)
    out = np.zeros((x.shape[0], 8))
    for b, row in enumerate(x):
        terms = _terms(row)
        out[b, 0] = 2.0 * g(terms[0].size) * np.sum(np.abs(terms[0])) / terms[0].size
        for col, v in zip((1, 2, 3), terms):
            n = v.size
            if n < 2:
                continue
            delta = g(n) * np.sum(np.abs(v)) / n
            out[b, col] = 2.0 * g(n + 2) * (_mean_m2(v)[1] + n * delta * delta) + n * delta * delta
        out[b, 4] = 2.0 * g(max(terms[1].size, 1)) * np.sum(np.abs(terms[1]))
    return out


def sign_changes_safe(x):
    """(B,) bool: no sample of the row lies within the mean's error bound of the mean, so the sign of x - mean does not depend on the evaluation."""
    x = np.asarray(x, np.float32)
    v = x.astype(np.float64)
    mean = v.sum(1) / x.shape[1]
    delta = g(x.shape[1]) * np.abs(v).sum(1) / x.shape[1]
    return np.all((np.abs(v - mean[:, None]) > 2.0 * delta[:, None]) | (delta[:, None] == 0.0), 1)


def integer_row(rng, L, lo=-9, hi=9):
    """Small integers whose row sum, sum of d1 and sum of d2 are all zero (L >= 6): every float64 term and partial sum is an integer."""
    x = rng.integers(lo, hi + 1, L).astype(np.int64)
    k = int(rng.integers(1, 4))
    x[L - 1] = x[0]; x[1] = x[0] + k; x[L - 2] = x[0] - k        # d1[0] = d1[L - 2] = k: d2 telescopes to zero, d1 to x[L - 1] - x[0] = 0
    x[3] -= x.sum()
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- planted signals
def white_noise(seed, n=1, L=3000):
    return np.random.default_rng(1000 + seed).standard_normal((n, L)).astype(np.float32)


def sine(seed, f_hz=1.0, sfreq=100.0, L=3000):
    """One row: a sine of f_hz with a seeded phase."""
    ph = np.random.default_rng(2000 + seed).uniform(0, 2 * np.pi)
    return np.sin(2 * np.pi * f_hz * np.arange(L) / sfreq + ph).astype(np.float32)[None, :]
