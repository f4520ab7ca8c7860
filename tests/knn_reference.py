"""float64 numpy reference of the nearest-neighbour search (csrc/knn.hip, eegldm.metrics) and the operation-count error bounds the tests
hold the device results to.  Shared by tests/test_knn_cpu.py and tests/test_gpu_knn.py."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def gamma(n):
    """n roundings compound to at most n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1)."""
    return n * U / (1.0 - n * U)


def c_of(D):
    """Longest chain of fp32 roundings a term of s = xbias - 2 <q, x> passes through.  A product q_k x_k enters the fmaf chain of the
    f32 MFMA at step k and is rounded once per remaining step, at most D times (the first step adds to zero: its rounding is the
    product's), then once more in s = fmaf(-2, dot, xbias): D + 1.  |x|^2 comes from eegldm_rows_sqnorm: a lane's chain of ceil(D / 64)
    fmafs and six butterfly additions, of which at most D round at all (adding a zero is exact), one more for a ball's |x|^2 - radius^2,
    and the final fmaf: <= D + 2.  As a multiple of u, with the compounding of the roundings kept: c(D) = (D + 2) / (1 - (D + 2) u)."""
    return gamma(D + 2) / U


def scores64(q, x, xbias=None):
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    s = -2.0 * (q @ x.T)
    return s if xbias is None else s + np.asarray(xbias, np.float64)[None, :]


def error_bound(q, x):
    """E(i, j) = c(D) 2^-24 (|q_i|^2 + |x_j|^2 + 2 sum |q x|)."""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    return c_of(q.shape[1]) * U * ((q * q).sum(1)[:, None] + (x * x).sum(1)[None, :] + 2.0 * (np.abs(q) @ np.abs(x).T))


def topk64(S, k, index_base=0, self_base=None):
    """Rows of the score matrix sorted by (score, index), the first k: (scores (Nq, k), indices (Nq, k) int64), padded with inf / -1.
    NaN scores never enter; `self_base` removes the pair index_base + j == self_base + i."""
    S = np.array(S, np.float64)
    nq, nc = S.shape
    if self_base is not None:
        for i in range(nq):
            j = self_base + i - index_base
            if 0 <= j < nc:
                S[i, j] = np.nan
    S[np.isnan(S)] = np.inf
    order = np.argsort(S, axis=1, kind="stable")[:, :k]
    sc = np.take_along_axis(S, order, 1)
    idx = np.where(np.isinf(sc), -1, order + index_base).astype(np.int64)
    out_s, out_i = np.full((nq, k), np.inf), np.full((nq, k), -1, np.int64)
    out_s[:, :sc.shape[1]], out_i[:, :sc.shape[1]] = sc, idx
    return out_s, out_i


def sqdist64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


def standardize64(x):
    x = np.asarray(x, np.float64)
    d = x - x.mean(1, keepdims=True)
    n = np.sqrt((d * d).sum(1, keepdims=True))
    flat = (x.max(1, keepdims=True) == x.min(1, keepdims=True)) | (n == 0)
    return np.where(flat, 0.0, d / np.where(n == 0, 1.0, n))


def sum_path(D):
    """Roundings on the longest path of the helpers' row sums: a lane's chain of ceil(D / 64) steps, then six butterfly levels."""
    return -(-D // 64) + 6


def standardize_bound(x):
    """|out - z| per element, z = d / n, d = x - mean, n = |d|: with p = sum_path(D) the mean carries dm = gamma(p + 1) mean|x|; every
    d_i then has u |d_i| + dm, the norm u n + dm sqrt(D) from its terms and (p / 2 + 1) u from its own sum and root, the division one u:
    |z_i| u (p / 2 + 4) + (dm / n) (1 + |z_i| sqrt(D)), times 1.01 for the products of these terms."""
    x = np.asarray(x, np.float64)
    D = x.shape[1]
    p = sum_path(D)
    d = x - x.mean(1, keepdims=True)
    n = np.sqrt((d * d).sum(1, keepdims=True))
    n = np.where(n == 0, 1.0, n)
    z = np.abs(d / n)
    dm = gamma(p + 1) * np.abs(x).mean(1, keepdims=True)
    return 1.01 * (z * U * (p / 2 + 4) + (dm / n) * (1.0 + z * np.sqrt(D)))


def kth_radius2_64(f, k):
    d2 = sqdist64(f, f)
    np.fill_diagonal(d2, np.inf)
    return np.sort(d2, axis=1)[:, k - 1]


def prc64(real, fake, k):
    """-> (dict of shares, margins): fake_margin[i] = min_j d2(fake_i, real_j) - r2_real[j], real_margin likewise against the fake balls,
    cover_margin[j] = min_i d2(real_j, fake_i) - r2_real[j]."""
    r2r, r2f = kth_radius2_64(real, k), kth_radius2_64(fake, k)
    d_fr = sqdist64(fake, real)
    fake_margin = (d_fr - r2r[None, :]).min(1)
    real_margin = (d_fr.T - r2f[None, :]).min(1)
    cover_margin = d_fr.T.min(1) - r2r
    shares = {"precision": float(np.mean(fake_margin <= 0)), "recall": float(np.mean(real_margin <= 0)), "coverage": float(np.mean(cover_margin <= 0))}
    return shares, {"precision": fake_margin, "recall": real_margin, "coverage": cover_margin}
