"""float64 numpy reference of R = K(A, B) V (csrc/kmm.hip, eegldm_kernel_matmul), the operation-count bound the device result is held to,
and the direct O(N^2) float64 definitions of the two-sample statistics.  Shared by tests/test_kmm_cpu.py and tests/test_gpu_kmm.py.

The reference evaluates the definition in float64 FROM THE fp32 INPUTS: a, b, v, gamma, coef0 and the betas are the fp32 values handed to
the call, asq / bsq the fp32 arrays handed to it (the kernel takes them as given), so their own rounding is no part of the error.

    R[i][p] = sum_j k(a_i, b_j) V[j][p], pairs with j - i == diag_off left out
    poly: k = (gamma <a, b> + coef0)^degree        rbf: k = (1 / S) sum_s exp(-beta_s d2), d2 = max(0, asq[i] + bsq[j] - 2 <a, b>)

Error bound (`error_bound`), u = 2^-24, g(n) = n u / (1 - n u) (Higham, lemma 3.1), every term evaluated in float64 on the reference's values:

* dot product: one fmaf chain of D steps on the f32 MFMA:                          e_dot = g(D) sum_k |a_ik b_jk|
* poly: t = fmaf(gamma, dot, coef0), one rounding:                                  e_t = |gamma| e_dot + u (|t| + |gamma| e_dot)
  then degree - 1 multiplications; with T = |t| + e_t:                              e_k = degree T^(degree-1) e_t + g(degree - 1) T^degree
* rbf: s = asq + bsq and d2 = fmaf(-2, dot, s), two roundings, then the clamp, a contraction (|max(0, x') - max(0, x)| <= |x' - x|):
                                                                                    e_d = u |s| + 2 e_dot + u (|s - 2 dot| + u |s| + 2 e_dot)
  z_s = -beta_s d2, one multiplication:                                             e_z = |beta_s| e_d + u |beta_s| (d2 + e_d)
  exp of the perturbed argument, |exp(z') - exp(z)| <= exp(z) (exp(e_z) - 1), plus the device expf's own error, EXPF_ULPS = 3 ulp (the OpenCL
  full-profile bound the ROCm device library is written to; an ulp is at most 2 u of the value; tests/test_gpu_kmm.py measures the
  largest error it meets and holds it to this), plus 2^-126 where the result is subnormal (flushed or rounded, whichever the device does):
                                                                                    e_s = exp(z) expm1(e_z) + 2 EXPF_ULPS u exp(z + e_z) + 2^-126
  S - 1 additions and one division, S roundings of non-negative values:             e_k = (1 + g(S)) mean_s e_s + g(S) k
* second product: the fmaf chain restarts from zero every CHAIN = 32 rows of B (one chain per 128-row tile would be g(128 + 1);
  the kernel folds into float64 four times per tile, and is held to that):               g(32 + 1) sum_j (|k_ij| + e_k) |V_jp| + sum_j e_k |V_jp|
  and a product or partial sum below 2^-126 may be flushed:                         + Nb 2^-126
* float64 additions of the tiles and slabs:                                         + Nb 2^-53 sum_j (|k_ij| + e_k) |V_jp|
"""
import numpy as np

U = 2.0 ** -24
EXPF_ULPS = 3.0
TINY = 2.0 ** -126
NO_DIAG = -(1 << 63)
TILE = 128
CHAIN = 32


def g(n):
    return n * U / (1.0 - n * U)


def _mask(na, nb, diag_off):
    """True where the pair is left out."""
    if diag_off is None or diag_off == NO_DIAG:
        return np.zeros((na, nb), bool)
    return (np.arange(nb)[None, :] - np.arange(na)[:, None]) == diag_off


def kernel64(a, b, kind="poly", degree=3, gamma=None, coef0=1.0, betas=None, asq=None, bsq=None):
    """K (Na, Nb) float64.  gamma / coef0 / betas are rounded to fp32 first, as the call receives them."""
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        dot = a64 @ b64.T
        if kind == "poly":
            gm = float(np.float32(1.0 / a64.shape[1] if gamma is None else gamma)); c0 = float(np.float32(coef0))
            return (gm * dot + c0) ** int(degree)
        s = np.asarray(asq, np.float32).astype(np.float64)[:, None] + np.asarray(bsq, np.float32).astype(np.float64)[None, :]
        d2 = np.maximum(0.0, s - 2.0 * dot)          # np.maximum propagates a NaN
        bt = np.asarray(betas, np.float32).astype(np.float64)
        return sum(np.exp(-bb * d2) for bb in bt) / len(bt)


def kmm64(a, b, v, diag_off=None, **kw):
    """R (Na, P) float64 and the masked K it came from."""
    k = kernel64(a, b, **kw)
    k = np.where(_mask(k.shape[0], k.shape[1], diag_off), 0.0, k)
    v64 = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return (k @ v64 if k.shape[1] else np.zeros((k.shape[0], v64.shape[1]))), k


def kernel_error(a, b, kind="poly", degree=3, gamma=None, coef0=1.0, betas=None, asq=None, bsq=None):
    """(|k|, e_k) per pair: the module docstring's chain up to the kernel value."""
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    D = a64.shape[1]
    dot = a64 @ b64.T
    e_dot = g(D) * (np.abs(a64) @ np.abs(b64).T)
    if kind == "poly":
        gs = float(np.float32(1.0 / D if gamma is None else gamma)); c0 = float(np.float32(coef0))
        gm = abs(gs)
        t = gs * dot + c0
        e_t = gm * e_dot + U * (np.abs(t) + gm * e_dot)
        T = np.abs(t) + e_t
        deg = int(degree)
        return np.abs(t) ** deg, deg * T ** (deg - 1) * e_t + g(deg - 1) * T ** deg
    s = np.asarray(asq, np.float32).astype(np.float64)[:, None] + np.asarray(bsq, np.float32).astype(np.float64)[None, :]
    pre = s - 2.0 * dot
    e_d = U * np.abs(s) + 2.0 * e_dot + U * (np.abs(pre) + U * np.abs(s) + 2.0 * e_dot)
    d2 = np.maximum(0.0, pre)
    bt = np.asarray(betas, np.float32).astype(np.float64)
    S = len(bt)
    k = np.zeros_like(d2); e = np.zeros_like(d2)
    with np.errstate(over="ignore"):
        for bb in bt:
            z = -bb * d2
            e_z = abs(bb) * e_d + U * abs(bb) * (d2 + e_d)
            k += np.exp(z)
            e += np.exp(z) * np.expm1(e_z) + 2.0 * EXPF_ULPS * U * np.exp(z + e_z) + TINY
    k /= S; e /= S
    return k, (1.0 + g(S)) * e + g(S) * k


def error_bound(a, b, v, diag_off=None, **kw):
    """E (Na, P): |R_device - R64| <= E elementwise for finite inputs."""
    k, e_k = kernel_error(a, b, **kw)
    m = _mask(k.shape[0], k.shape[1], diag_off)
    k, e_k = np.where(m, 0.0, k), np.where(m, 0.0, e_k)
    av = np.abs(np.asarray(v, np.float32).astype(np.float64))
    nb = k.shape[1]
    if nb == 0:
        return np.zeros((k.shape[0], av.shape[1]))
    kv = (k + e_k) @ av
    return g(CHAIN + 1) * kv + e_k @ av + nb * TINY + nb * 2.0 ** -53 * kv


def slab_rows(nb):
    """Rows of B per slab: B's 128-row tiles are cut into at most 32 slabs by a rule that depends on Nb alone."""
    tiles = -(-nb // TILE)
    want = min(tiles, 32)
    return TILE * (-(-tiles // want)) if want else TILE


# ---------------------------------------------------------------------------------------------------- statistics, direct definitions
def mmd2_direct(kxx, kyy, kxy, unbiased=True):
    """From the three full float64 kernel matrices."""
    n, m = kxx.shape[0], kyy.shape[0]
    if unbiased:
        sxx = (kxx * (1.0 - np.eye(n))).sum()
        syy = (kyy * (1.0 - np.eye(m))).sum()
        return sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2.0 * kxy.sum() / (n * m)
    return kxx.sum() / (n * n) + kyy.sum() / (m * m) - 2.0 * kxy.sum() / (n * m)


def split_mmd2_direct(kzz, in_x):
    """Unbiased MMD^2 of the split of the pooled rows given by the boolean vector in_x, from the full pooled kernel matrix."""
    ix, iy = np.nonzero(in_x)[0], np.nonzero(~in_x)[0]
    return mmd2_direct(kzz[np.ix_(ix, ix)], kzz[np.ix_(iy, iy)], kzz[np.ix_(ix, iy)])
