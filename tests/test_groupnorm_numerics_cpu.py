"""CPU: the statistics arithmetic of the GroupNorm kernels (csrc/norm.hip) restated in numpy float32 / float64, so that the cause of the
mean-30-sigma finding and its repair stay pinned without a GPU.

The register-resident forward keeps a (sample, CC-channel chunk) in the registers of NTH threads: thread (tx, ty) owns the 4 channels
4 tx .. 4 tx + 3 of the chunk and the rows ty, ty + TY, ty + 2 TY, ... (TX = CC / 4, TY = NTH / TX).  For 16-bit inputs it takes ONE
reduction round: per thread, in fp32 and in row order, s1 += (v0 + v1) + (v2 + v3) and four sequential fmaf(v, v, s2); both partials
are widened to fp64 and added across the threads of the group (fp64: the order does not show), then scaled by 1 / n.

  `old` (before the repair): v = x, and 1 / n is the FLOAT 1.0f / (cpg L) widened to double: mean = S1 inv, var = S2 inv - mean^2.
        Two relative errors of ~1e-7 -- the inexact reciprocal whenever cpg L is no power of two, and the rounding of the fp32 partial
        of x^2 -- enter var multiplied by mean^2 / var.
  `new`: v = x - pivot with pivot = the group's first element (one value for all threads of the group), 1 / n in fp64:
        mean = pivot + S1 / n, var = S2 / n - (S1 / n)^2.  The amplification is 1 + (mean - pivot)^2 / var, a few units whatever the mean.

The rest of the forward is the kernel's in both: rstd = fp32 1 / sqrt(fp32(var) + eps), the folded scale gamma rstd and shift
fma(-mean, scale, beta) in fp32, z = fma(x, scale, shift), one rounding to the storage type.  (rsqrtf is modelled as correctly rounded;
its 1-ulp error is a relative 1e-7 on every element alike, unamplified.)

test_old_arithmetic_reproduces_the_finding: the `old` model at the finding's case (B 4, L 192, C 256, 32 groups, no SiLU, mean 30 sigma,
fp16; 256 threads on 64-channel chunks as the few-slab narrowing launches it) gives the figures recorded from the device: 8.3e-2 of the
outputs differ from RNE(ref), mean signed error +0.073 ulp.  test_new_arithmetic_is_within_check_b: the `new` model passes numerics.check_b
(mismatch share <= 2 m_emul + 1e-3 against torch's fp32 group_norm, |mean signed error| <= 0.02 ulp) in fp16 and bf16 at means of 0, 30 and
100 sigma, and its variance is right to a relative 1e-6.

Further down, with the same old / new pair: the flat G = 1 forward (two passes in fp32 over the whole sample; `old` on x itself with
xhat = fma(x, rstd, -mean rstd), `new` about the sample's first element), whose uncentred form reproduces the 1.1e-2 recorded on the
device at 30 sigma in fp16; and the split statistics kernel, which is unchanged and whose 96-element fp32 partials about zero still carry
the mean^2 / var factor (5e-4 of relative variance error at 100 sigma in fp16) -- pinned so that a later repair has its figure."""
import numpy as np
import pytest
import torch

import numerics as N

EPS = 1e-6


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64 and the sum is rounded there once more, 29 bits below
    the fp32 rounding: a double rounding that moves a result only at an exact fp32 midpoint"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def resident_stats(x, G, nth, cc, form):
    """(mean fp32, rstd fp32, var float64) per (sample, group) as gn_fwd_resident_kernel<16-bit> forms them; x (B, C, L) float64 storage values"""
    x = x.numpy()
    B, C, L = x.shape
    cpg = C // G
    assert cpg % 4 == 0 and cc % cpg == 0 and C % cc == 0
    TY = nth // (cc // 4)
    rpt = -(-L // TY)
    n = cpg * L
    xg = x.reshape(B, G, cpg // 4, 4, L).astype(np.float32)           # (b, g, column vector of the group, channel of the vector, row)
    pad = np.zeros((B, G, cpg // 4, 4, rpt * TY - L), np.float32)
    rows = np.concatenate([xg, pad], -1).reshape(B, G, cpg // 4, 4, rpt, TY)      # row = k TY + ty
    live = (np.arange(rpt)[:, None] * TY + np.arange(TY)[None, :]) < L
    pivot = xg[:, :, 0, 0, 0] if form == "new" else np.zeros((B, G), np.float32)
    s1 = np.zeros((B, G, cpg // 4, TY), np.float32); s2 = np.zeros_like(s1)
    for k in range(rpt):
        v = [(rows[:, :, :, j, k, :] - pivot[:, :, None, None]).astype(np.float32) for j in range(4)]
        t1 = (s1 + ((v[0] + v[1]).astype(np.float32) + (v[2] + v[3]).astype(np.float32)).astype(np.float32)).astype(np.float32)
        t2 = s2
        for j in range(4):
            t2 = _fma32(v[j], v[j], t2)
        s1 = np.where(live[k], t1, s1); s2 = np.where(live[k], t2, s2)
    S1 = s1.astype(np.float64).sum((2, 3)); S2 = s2.astype(np.float64).sum((2, 3))
    if form == "old":
        inv = np.float64(np.float32(1.0) / (np.float32(cpg) * np.float32(L)))
        mu = S1 * inv
        var = np.maximum(S2 * inv - mu * mu, 0.0)
        mean = mu.astype(np.float32)
    else:
        inv = 1.0 / np.float64(n)
        md = S1 * inv
        var = np.maximum(S2 * inv - md * md, 0.0)
        mean = (pivot.astype(np.float64) + md).astype(np.float32)
    rstd = (1.0 / np.sqrt((var.astype(np.float32) + np.float32(EPS)).astype(np.float64))).astype(np.float32)
    return mean, rstd, var


def resident_forward(x, G, gamma, beta, nth, cc, form, fmt):
    """the resident forward's output (float64 holding `fmt` values) and the relative error of its variance"""
    mean, rstd, var = resident_stats(x, G, nth, cc, form)
    B, C, L = x.shape
    rep = lambda t: np.repeat(t, C // G, axis=1)[:, :, None]
    ga = (gamma.numpy().astype(np.float32)[None, :, None] * rep(rstd)).astype(np.float32)
    be = _fma32(-rep(mean), ga, np.broadcast_to(beta.numpy().astype(np.float32)[None, :, None], ga.shape))
    z = _fma32(x.numpy().astype(np.float32), ga, be)
    _m, var_ref, _r = N.gn_stats(x, G, EPS)
    return N.rne(torch.from_numpy(z.astype(np.float64)), fmt), (var - var_ref.numpy()) / var_ref.numpy()


def _inputs(B, C, L, off, fmt, seed=71):
    x = N.to_storage(_randn((B, C, L), seed) + off, fmt)
    ga = N.rne(1 + 0.1 * _randn((C,), seed + 1), "f32"); be = N.rne(0.1 * _randn((C,), seed + 2), "f32")
    return x, ga, be


def test_old_arithmetic_reproduces_the_finding():
    B, L, C, G = 4, 192, 256, 32
    x, ga, be = _inputs(B, C, L, 30.0, "f16")
    ref = N.gn_fwd(x, G, ga, be, EPS)
    got, rel_var = resident_forward(x, G, ga, be, 256, 64, "old", "f16")
    share = N.mismatch_share(got, ref, "f16"); mu, _cnt = N.mean_signed_ulp(got, ref, "f16")
    print(f"[model] old arithmetic, finding's case f16: mismatch {share:.4f}, mean {mu:+.4f} ulp, rel var error max {np.abs(rel_var).max():.2e} "
          f"mean {rel_var.mean():+.2e}")
    assert 0.07 <= share <= 0.09, share
    assert mu > 0.05, mu
    assert rel_var.mean() < -5e-5, rel_var.mean()
    # the float reciprocal alone (bf16: the fp32 partials of 8-bit significands are exact) shifts every group's variance the same way
    xb, _, _ = _inputs(B, C, L, 30.0, "bf16")
    _m, _r, var = resident_stats(xb, G, 256, 64, "old")
    relb = (var - N.gn_stats(xb, G, EPS)[1].numpy()) / N.gn_stats(xb, G, EPS)[1].numpy()
    print(f"[model] old arithmetic, bf16: rel var error min {relb.min():+.2e} max {relb.max():+.2e}")
    assert relb.max() < -1e-5 and relb.min() > -5e-5, (relb.min(), relb.max())


@pytest.mark.parametrize("off", [0.0, 30.0, 100.0])
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_new_arithmetic_is_within_check_b(fmt, off):
    B, L, C, G = 4, 192, 256, 32
    x, ga, be = _inputs(B, C, L, off, fmt)
    assert bool(torch.isfinite(x).all())
    ref = N.gn_fwd(x, G, ga, be, EPS)
    emul = torch.nn.functional.group_norm(x.float(), G, ga.float(), be.float(), eps=EPS)
    for nth, cc in ((256, 64), (1024, 256)):          # the few-slab narrowing and the production launch
        got, rel_var = resident_forward(x, G, ga, be, nth, cc, "new", fmt)
        N.check_b(got, ref, emul, fmt, route=f"model: pivot statistics nth{nth} cc{cc} mean {off:g} std")
        assert np.abs(rel_var).max() < 1e-6, np.abs(rel_var).max()


# ---------------------------------------------------------------- flat G = 1 forward (gn_flat_fwd_kernel / gn_flat_fwd_wide_kernel, 16-bit types)
def _block_sum(per_thread, nt):
    """flat_block_sum: xor-shuffle tree inside each 64-lane wave (lane 0 ends with the halving sum), then the waves four at a time,
    t += (w0 + w1) + (w2 + w3); per_thread (B, nt) fp32 -> (B,) fp32"""
    a = per_thread.reshape(per_thread.shape[0], nt // 64, 64)
    w = 64
    while w > 1:
        w //= 2
        a = (a[..., :w] + a[..., w:2 * w]).astype(np.float32)
    a = a[..., 0]
    t = np.zeros(a.shape[0], np.float32)
    for i in range(0, nt // 64, 4):
        t = (t + ((a[:, i] + a[:, i + 1]).astype(np.float32) + (a[:, i + 2] + a[:, i + 3]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return t


def flat_forward(x, gamma, beta, form, fmt, nt=256):
    """One block of nt threads per sample; the sample is a flat run of n = L C elements in 8-element chunks, chunk ci held by thread
    ci % nt as its chunk ci // nt.  Two passes, fp32 all the way.
      `old`: s = sum x, mean = s (1 / n); q = sum (x - mean)^2; xhat = fma(x, rstd, -mean rstd)
      `new`: about p = the sample's first element: s = sum (x - p), md = s (1 / n), mean = p + md; q = sum ((x - p) - md)^2;
             xhat = ((x - p) - md) rstd
    then z = fma(xhat, gamma, beta) and one rounding.  Returns (output, mean fp32, rstd fp32)."""
    B, C, L = x.shape
    n = L * C
    flat = x.permute(0, 2, 1).reshape(B, n).numpy().astype(np.float32)          # NLC order: element l C + c
    nch = n // 8; kmax = -(-nch // nt)
    ch = np.zeros((B, kmax * nt, 8), np.float32); ch[:, :nch] = flat.reshape(B, nch, 8)
    ch = ch.reshape(B, kmax, nt, 8)
    live = (np.arange(kmax)[:, None] * nt + np.arange(nt)[None, :]) < nch
    pv = flat[:, 0] if form == "new" else np.zeros(B, np.float32)
    d = (ch - pv[:, None, None, None]).astype(np.float32)
    s = np.zeros((B, nt), np.float32)
    for k in range(kmax):
        v = d[:, k]
        t = (((v[..., 0] + v[..., 1]).astype(np.float32) + (v[..., 2] + v[..., 3]).astype(np.float32)).astype(np.float32)
             + ((v[..., 4] + v[..., 5]).astype(np.float32) + (v[..., 6] + v[..., 7]).astype(np.float32)).astype(np.float32)).astype(np.float32)
        s = np.where(live[k], (s + t).astype(np.float32), s)
    inv_n = np.float32(1.0) / np.float32(n)
    md = (_block_sum(s, nt) * inv_n).astype(np.float32)
    mean = (pv + md).astype(np.float32)
    c = (d - md[:, None, None, None]).astype(np.float32)                            # old: pv = 0, so this is x - mean
    q = np.zeros((B, nt), np.float32)
    for k in range(kmax):
        t = q
        for j in range(8):
            t = _fma32(c[:, k, :, j], c[:, k, :, j], t)
        q = np.where(live[k], t, q)
    var32 = (_block_sum(q, nt) * inv_n).astype(np.float32)
    rstd = (1.0 / np.sqrt((var32 + np.float32(EPS)).astype(np.float64))).astype(np.float32)
    r4 = rstd[:, None, None, None]
    if form == "new":
        xh = (c * r4).astype(np.float32)
    else:
        nmr = (-mean * rstd).astype(np.float32)
        xh = _fma32(ch, np.broadcast_to(r4, ch.shape), np.broadcast_to(nmr[:, None, None, None], ch.shape))
    idx = (np.arange(kmax * nt * 8) % C).reshape(kmax, nt, 8)                       # channel of element j of every chunk (8 % C == 0 or C | 8 k)
    ga = gamma.numpy().astype(np.float32)[idx]; be = beta.numpy().astype(np.float32)[idx]
    z = _fma32(xh, np.broadcast_to(ga, xh.shape), np.broadcast_to(be, xh.shape))
    z = z.reshape(B, kmax * nt * 8)[:, :n].reshape(B, L, C).transpose(0, 2, 1)
    return N.rne(torch.from_numpy(z.astype(np.float64)), fmt), mean, rstd


def test_flat_forward_old_carries_the_mean_into_xhat_new_does_not():
    """(3, 6144, 1, 1) at 30 sigma in fp16, the case of test_gpu_groupnorm_rounding.py (without its SiLU).  The uncentred form puts ~2^-24 x 30
    of error into xhat, the SAME on every element of a sample (fp32 sums of values near 30, the rounded -mean rstd): recorded on the device
    1.1e-2 of the fp16 outputs off RNE(ref) against 4.5e-3 for torch's fp32.  About the first element the error of xhat is that of |x - p| ~ 1."""
    B, L, C = 3, 6144, 1
    x, ga, be = _inputs(B, C, L, 30.0, "f16")
    ref = N.gn_fwd(x, 1, ga, be, EPS)
    emul = torch.nn.functional.group_norm(x.float(), 1, ga.float(), be.float(), eps=EPS)
    mean, _v, rstd = N.gn_stats(x, 1, EPS)
    out = {}
    for form in ("old", "new"):
        got, m32, r32 = flat_forward(x, ga, be, form, "f16")
        # the systematic part: error of xhat common to a whole sample, in units of 2^-24 |mean| rstd
        shift = np.abs((m32.astype(np.float64) - mean[:, 0].numpy()) * rstd[:, 0].numpy()) / (N.U32 * np.abs(mean[:, 0].numpy()) * rstd[:, 0].numpy())
        out[form] = (N.mismatch_share(got, ref, "f16"), shift.max())
        print(f"[model] flat forward {form}: mismatch {out[form][0]:.2e} (emulation {N.mismatch_share(N.rne(emul, 'f16'), ref, 'f16'):.2e}), "
              f"mean error {shift.max():.2f} x 2^-24 |mean|")
    got, _m, _r = flat_forward(x, ga, be, "new", "f16")
    N.check_b(got, ref, emul, "f16", route="model: flat forward about the first element, mean 30 std")
    assert out["new"][0] < 0.5 * out["old"][0], out
    assert out["old"][0] > 5e-3, out


@pytest.mark.parametrize("C,L", [(2, 12288), (8, 768)])
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_flat_forward_new_is_within_check_b_at_100_sigma(fmt, C, L):
    x, ga, be = _inputs(3, C, L, 100.0, fmt)
    ref = N.gn_fwd(x, 1, ga, be, EPS)
    emul = torch.nn.functional.group_norm(x.float(), 1, ga.float(), be.float(), eps=EPS)
    got, m32, r32 = flat_forward(x, ga, be, "new", fmt)
    N.check_b(got, ref, emul, fmt, route=f"model: flat forward about the first element C{C} n{C * L} mean 100 std")
    _m, _v, rstd = N.gn_stats(x, 1, EPS)
    assert np.abs(r32 / rstd[:, 0].numpy() - 1).max() < 1e-6


# ---------------------------------------------------------------- split statistics kernel (gn_stats_kernel, every type; unchanged)
def split_stats_var(x, G, rows_per_block, V=4, nt=256):
    """float64 variance as gn_stats_kernel + gn_finalize_kernel form it: a block owns rows_per_block rows of a sample, thread (tx, ty) the
    V-channel column tx and the rows ty, ty + TY, ...; fp32 s1 += x, s2 = fma(x, x, s2) per thread about ZERO, fp64 from there on and an
    fp64 divisor"""
    B, C, L = x.shape
    cpg = C // G
    TX = min(C // V, nt); TY = nt // TX
    xn = x.numpy().astype(np.float32)
    S1 = np.zeros((B, G)); S2 = np.zeros((B, G))
    for l0 in range(0, L, rows_per_block):
        for ty in range(TY):
            rows = xn[:, :, l0 + ty:min(L, l0 + rows_per_block):TY]                   # (B, C, rows of this lane)
            if rows.shape[2] == 0:
                continue
            s1 = np.zeros((B, C // V), np.float32); s2 = np.zeros_like(s1)
            for r in range(rows.shape[2]):
                for k in range(V):
                    v = rows[:, k::V, r]
                    s1 = (s1 + v).astype(np.float32); s2 = _fma32(v, v, s2)
            g = (np.arange(C // V) * V) // cpg
            for gi in range(G):
                S1[:, gi] += s1[:, g == gi].astype(np.float64).sum(1); S2[:, gi] += s2[:, g == gi].astype(np.float64).sum(1)
    n = float(cpg * L)
    mu = S1 / n
    return np.maximum(S2 / n - mu * mu, 0.0)


def test_split_statistics_keep_the_mean_squared_factor():
    """The split kernels are unchanged: with 96-element partials (384 rows per block) the relative variance error at 100 sigma in fp16 is of the
    order 2^-24 mean^2 / var, far above what the pivot leaves (1e-6, above), and inside the bound test_gpu_groupnorm_rounding.py allows it."""
    B, L, C, G = 2, 384, 64, 8
    x, _ga, _be = _inputs(B, C, L, 100.0, "f16")
    var = split_stats_var(x, G, 384)
    _m, var_ref, _r = N.gn_stats(x, G, EPS)
    rel = np.abs(var - var_ref.numpy()) / var_ref.numpy()
    amp = float((_m ** 2 / var_ref).max())
    print(f"[model] split statistics, 96-element partials, mean 100 std f16: rel var error max {rel.max():.2e}, mean^2 / var {amp:.3g}")
    assert rel.max() > 1e-5, rel.max()
    assert rel.max() < N.gamma(98) * (1 + amp), (rel.max(), N.gamma(98) * (1 + amp))
