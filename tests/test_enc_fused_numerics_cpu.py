"""CPU: the references of the fused frozen encoder (numerics.pre_conv3_ref, sums_bound, enc_stats_bounds) held against an fp32 model of the
arithmetic of csrc/enc_fused.hip, and against the same model with one defect planted at a time.

The model (pre_conv3_model) follows the kernel step by step on the CPU: fp64 (mean, var) from the (sum, sum of squares) slots, fp32 rstd and
scale = gamma rstd, mean = mh + ml split into two floats, z = fma(x - mh, scale, beta - ml scale), SiLU in fp32, ONE
rounding of the activated operand to the storage type, zero rows outside the sample, three taps accumulated in fp32, bias and residual added
in fp32, one rounding of y, and (sum, sum of squares) of the ROUNDED y: every lane sums its Cout values about the first of them, p, one-pass
in fp32 (d = y - p and d^2), rebuilds its sums in fp64 as D1 + n p and D2 + p (2 D1 + n p); fp64 from there on, added onto the
preloaded slot.  It must pass check A, check B, the exact-row reports and the statistics bound at means of 0, 30 and 100 sigma.
`about_zero=True` gives the sums as they were before the pivot (about zero): kept to pin what the pivot repaired.

Each planted defect must FAIL, on the smallest case that can show it -- a suite that passes all of them has proved nothing:
  act(0) in the padding rows | halo row from the neighbouring sample | zero halo at the tile seam 255 | 256 | taps reversed |
  residual dropped on output channels 16..31 | out_stats of the unrounded y | statistics of sample b - 1 used for sample b."""
import math

import numpy as np
import pytest
import torch

import numerics as N

EPS = 1e-6
SEAM_ROWS = (0, 1, 254, 255, 256, 257, -2, -1)


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _f32(t):
    return t.float()


def make_case(B, L, Cin, Cout, fmt, off=0.0, scale=1.0, resid=True, beta0=0.0, seed=11):
    """operands as the GPU test makes them: x = scale (randn + off) rounded to storage, fp32 gamma / beta / bias, storage-typed weights"""
    x = N.to_storage(scale * (_randn((B, Cin, L), seed) + off), fmt)
    assert bool(torch.isfinite(x).all())
    ga = N.rne(1 + 0.2 * _randn((Cin,), seed + 1), "f32"); be = N.rne(beta0 + 0.1 * _randn((Cin,), seed + 2), "f32")
    w = N.to_storage(_randn((Cout, Cin, 3), seed + 3) / math.sqrt(3 * Cin), fmt)
    bias = N.rne(0.1 * _randn((Cout,), seed + 4), "f32")
    r = N.to_storage(_randn((B, Cout, L), seed + 5), fmt) if resid else None
    xf = x.reshape(B, -1)
    in_stats = torch.stack([xf.sum(-1), (xf * xf).sum(-1)], -1)
    preload = torch.tensor([[3.0, 7.0]] * B, dtype=torch.float64) * torch.arange(1, B + 1, dtype=torch.float64)[:, None]
    return dict(x=x, ga=ga, be=be, w=w, bias=bias, resid=r, in_stats=in_stats, preload=preload, fmt=fmt, B=B, L=L, Cin=Cin, Cout=Cout)


def _lane_stats(y, about_zero=False):
    """(B, 2) float64 (sum, sum of squares) of y (B, Cout, L) float32 as the epilogue forms them: every lane sums its Cout values (rows
    64 w + 16 i + lm, channels 32 h + 16 j + 4 q + e, in the order h, j, i, e) sequentially in fp32 about the first of them, rebuilds its
    sums in fp64, and the lanes and waves are added in fp64"""
    B, C, L = y.shape
    t = y.reshape(B, C // 32, 2, 4, 4, L // 64, 4, 16)                    # (b, h, j, q, e, w, i, lm)
    t = t.permute(0, 5, 7, 3, 1, 2, 6, 4).reshape(B, L // 64, 16, 4, C)   # (b, w, lm, q, chain of C values)
    p = torch.zeros_like(t[..., 0]) if about_zero else t[..., 0].clone()
    d = t - p[..., None]
    s1 = torch.zeros_like(p); s2 = torch.zeros_like(p)
    for k in range(C):
        s1 = s1 + d[..., k]
        s2 = (s2.double() + d[..., k].double() * d[..., k].double()).float()       # fma
    d1, d2, pd = s1.double(), s2.double(), p.double()
    return torch.stack([(d1 + C * pd).sum((1, 2, 3)), (d2 + pd * (2 * d1 + C * pd)).sum((1, 2, 3))], -1)


def pre_conv3_model(c, defect=None, about_zero=False):
    """(y (B, Cout, L) float64 holding storage values, out_stats (B, 2) float64) of the fp32 model, optionally with one planted defect"""
    x, fmt, B, L = c["x"], c["fmt"], c["B"], c["L"]
    n = c["Cin"] * L
    st = c["in_stats"]
    if defect == "stats_of_previous_sample":
        st = torch.roll(st, 1, 0)
    mean = st[:, 0] / n
    var = torch.clamp(st[:, 1] / n - mean * mean, min=0.0)
    rstd = _f32(1.0 / torch.sqrt(var + float(np.float32(EPS))))
    sc = _f32(c["ga"])[None, :] * rstd[:, None]                           # fp32 product
    mh = _f32(mean); ml = mean - mh.double()                              # mean = mh + ml
    sh = _f32(c["be"][None, :] - ml[:, None] * sc.double())               # fp64, one rounding
    xc = _f32(x) - mh[:, None, None]                                      # fp32 subtraction (exact near the mean)
    z = (xc.double() * sc.double()[:, :, None] + sh.double()[:, :, None]).float()            # fma: one rounding
    a = N.rne((z * (1.0 / (1.0 + torch.exp(-z)))).double(), fmt)          # silu_f in fp32, then the LDS rounding
    pad = torch.zeros(B, c["Cin"], 1, dtype=torch.float64)
    if defect == "act0_in_padding":
        pad = N.rne(torch.nn.functional.silu(_f32(c["be"][None, :] - mean[:, None] * sc.double())).double(), fmt)[:, :, None]      # act(0)
    ap = torch.cat([pad, a, pad], 2)                                      # ap[:, :, l + t] = a[:, :, l + t - 1]
    taps = [ap[:, :, t:t + L].clone() for t in range(3)]
    if defect == "halo_from_neighbour_sample":
        taps[0][1:, :, 0] = a[:-1, :, L - 1]; taps[2][:-1, :, L - 1] = a[1:, :, 0]
    if defect == "zero_halo_at_tile_seam":
        taps[0][:, :, 256] = 0.0; taps[2][:, :, 255] = 0.0
    w = _f32(c["w"])
    order = (2, 1, 0) if defect == "taps_reversed" else (0, 1, 2)
    acc = torch.zeros(B, c["Cout"], L, dtype=torch.float32)
    for t in range(3):
        acc = acc + torch.einsum("oc,bcl->bol", w[:, :, order[t]], _f32(taps[t]))
    v = acc + _f32(c["bias"])[None, :, None]
    if c["resid"] is not None:
        r = _f32(c["resid"]).clone()
        if defect == "resid_dropped_16_31":
            r[:, 16:32] = 0.0
        v = v + r
    y = N.rne(v.double(), fmt)
    out_stats = c["preload"] + _lane_stats(_f32(v if defect == "stats_of_unrounded_y" else y), about_zero)
    return y, out_stats


def judge(c, y, out_stats, tag):
    """every check the GPU test runs on one pre_conv3 launch; returns the list of failures (empty: passed)"""
    fmt, B, L = c["fmt"], c["B"], c["L"]
    fails = []
    y_ref, _mag, d = N.pre_conv3_ref(c["x"], c["in_stats"], c["ga"], c["be"], c["w"], c["bias"], c["resid"], fmt, EPS)
    emul = N.pre_conv3_emul(c["x"], 1, c["ga"], c["be"], c["w"], c["bias"], c["resid"], fmt, EPS)
    try:
        N.check(y, y_ref, d / N.gamma(0), 0, fmt, emul=emul, route=tag)
    except AssertionError as e:
        fails.append(str(e))
    fails += N.check_rows(y, y_ref, d, fmt, SEAM_ROWS, route=tag)
    bounds = N.pivot_sums_bounds(y, N.pre_conv3_pivots(y), N.PRE_CONV3_STATS_DEPTH, n64=64 * 4 * (L // 256), preload=c["preload"])
    for k, vals in enumerate((y, y * y)):
        err = (out_stats[:, k] - c["preload"][:, k] - vals.sum((1, 2))).abs()
        ratio = float((err / bounds[k]).max())
        print(f"[numerics] {tag} out_stats[{k}]: worst {ratio:.3f} x bound")
        if not ratio <= 1:
            fails.append(f"{tag}: out_stats[{k}] is {ratio:.3g} x its bound away from the sums of the stored y")
    return fails


@pytest.mark.parametrize("off", [0.0, 30.0, 100.0])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_model_of_the_kernel_passes(fmt, off):
    for (B, L, Cin, Cout) in ((2, 512, 32, 64), (1, 256, 64, 32)):
        c = make_case(B, L, Cin, Cout, fmt, off=off)
        y, st = pre_conv3_model(c)
        fails = judge(c, y, st, f"model {Cin}->{Cout} B{B} L{L} mean {off:g} std")
        assert not fails, "\n".join(fails)


def test_model_passes_where_var_is_eps_and_on_a_constant_sample():
    c = make_case(2, 256, 32, 32, "bf16", scale=1e-3)
    y, st = pre_conv3_model(c)
    assert not judge(c, y, st, "model |x| 1e-3")
    c = make_case(2, 256, 32, 32, "f16")
    c["x"][1] = 0.75
    xf = c["x"].reshape(2, -1); c["in_stats"] = torch.stack([xf.sum(-1), (xf * xf).sum(-1)], -1)
    _m, var, rstd, _s, _h = N.enc_affine(c["in_stats"], 32 * 256, c["ga"], c["be"], EPS)
    assert float(var[1]) == 0.0 and abs(float(rstd[1]) * math.sqrt(float(np.float32(EPS))) - 1) < 1e-12
    y, st = pre_conv3_model(c)
    assert not judge(c, y, st, "model constant sample")


# defect -> the smallest case that can show it (B, L, Cin, Cout, fmt, keyword arguments of make_case)
DEFECTS = {
    "act0_in_padding": (1, 256, 32, 32, "f16", dict(beta0=2.0)),                  # silu(shift) ~ 1.8: far from the zero padding
    "halo_from_neighbour_sample": (2, 256, 32, 32, "f16", {}),
    "zero_halo_at_tile_seam": (1, 512, 32, 32, "f16", {}),
    "taps_reversed": (1, 256, 32, 32, "f16", {}),
    "resid_dropped_16_31": (1, 256, 32, 32, "f16", {}),
    "stats_of_unrounded_y": (1, 256, 32, 32, "bf16", {}),                         # (the rounding noise of fp16 is below the fp32 bound of the sums)
    "stats_of_previous_sample": (2, 256, 32, 32, "f16", {}),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_fails(defect):
    B, L, Cin, Cout, fmt, kw = DEFECTS[defect]
    c = make_case(B, L, Cin, Cout, fmt, **kw)
    y, st = pre_conv3_model(c)
    assert not judge(c, y, st, f"{defect}: the sound model on this case"), "the case must pass without the defect"
    y, st = pre_conv3_model(c, defect)
    fails = judge(c, y, st, defect)
    print(f"[defect] {defect}: {len(fails)} checks failed; first: {fails[0][:200] if fails else None}")
    assert fails, f"{defect} passed every check"
    if defect in ("act0_in_padding", "halo_from_neighbour_sample"):
        assert any("row 0" in f or f"row {L - 1}" in f for f in fails), fails           # named by its row, not averaged
    if defect == "zero_halo_at_tile_seam":
        assert any("row 255" in f for f in fails) and any("row 256" in f for f in fails), fails
    if defect == "stats_of_unrounded_y":
        assert all("out_stats" in f for f in fails), fails                              # y itself is untouched


def _sample_stats_model(v, about_zero=False):
    """sample_stats_kernel on (B, n) fp32 values: `per` blocks of 256 threads, 8-value chunks grid-strided, fp32 per thread and over the six
    shuffle levels, about the sample's first element, fp64 from the wave partials on"""
    B, n = v.shape
    nch = n // 8
    per = min(64, max(1, (nch + 255) // 256))
    nt = per * 256
    k = -(-nch // nt)
    pv = torch.zeros(B) if about_zero else v[:, 0].clone()
    ch = torch.zeros(B, k * nt, 8, dtype=torch.float32); ch[:, :nch] = v.reshape(B, nch, 8) - pv[:, None, None]
    ch = ch.reshape(B, k, nt, 8)
    s1 = torch.zeros(B, nt); s2 = torch.zeros(B, nt)
    for i in range(k):
        for e in range(0, 8, 2):
            v0, v1 = ch[:, i, :, e], ch[:, i, :, e + 1]
            s1 = s1 + (v0 + v1)
            s2 = s2 + (v0.double() * v0.double() + (v1 * v1).double()).float()
    out = []
    for s in (s1, s2):
        s = s.reshape(B, nt // 64, 64)
        w = 64
        while w > 1:
            w //= 2
            s = s[..., :w] + s[..., w:2 * w]
        out.append(s[..., 0].double().sum(-1))
    d1, d2, pd = out[0], out[1], pv.double()
    return torch.stack([d1 + n * pd, d2 + pd * (2 * d1 + n * pd)], -1)


@pytest.mark.parametrize("n", [8, 2040, 2048, 2056, 98304])
def test_sums_bound_holds_the_sample_stats_model(n):
    for off in (0.0, 30.0, 100.0):
        for fmt in ("bf16", "f16"):
            v = N.to_storage(_randn((3, n), 5) + off, fmt)
            got = _sample_stats_model(v.float())
            bounds = N.pivot_sums_bounds(v, v[:, :1], N.sample_stats_depth(n), n64=4 * 64)
            for k, vals in enumerate((v, v * v)):
                ratio = float(((got[:, k] - vals.sum(-1)).abs() / bounds[k]).max())
                assert ratio <= 1, (n, off, fmt, k, ratio)
    assert N.sample_stats_depth(8) == 16 and N.sample_stats_depth(98304) == 8 * 1 + 8 and N.sample_stats_depth(64 * 256 * 8 * 3) == 8 * 3 + 8


def test_sums_about_zero_carry_the_mean_squared_factor_and_the_pivot_does_not():
    """The statistics a consumer derives from the slots, at a mean of 30 sigma in fp16.  About zero (the kernels before the pivot) the bound of
    var carries 1 + 3 mean^2 / var and the model's variance is off by a relative 1e-6 to 1e-4; about the first element both stay at the
    fp32 level -- what test_gpu_enc_fused_rounding.py::test_statistics_chain found on the device and now holds."""
    out = {}
    for off in (0.0, 30.0):
        v = N.to_storage(_randn((2, 16384), 9) + off, "f16")
        n = v.shape[1]
        for zero in (True, False):
            b = N.enc_stats_bounds(v, N.sample_stats_depth(n), EPS, pivot=None if zero else v[:, :1])
            st = _sample_stats_model(v.float(), about_zero=zero)
            mean = st[:, 0] / n; var = st[:, 1] / n - mean * mean
            assert bool(((mean - b["mean"]).abs() <= b["e_mean"]).all())
            assert bool(((var - b["var"]).abs() <= b["e_var"]).all())
            out[off, zero] = (float((b["e_var"] / b["var"]).max()), float(((var - b["var"]).abs() / b["var"]).max()))
    print(f"[model] e_var / var bound and measured: {out}")
    assert out[30.0, True][0] > 500 * out[0.0, True][0], out          # the amplification, in the bound ...
    assert out[30.0, True][1] > 20 * out[30.0, False][1], out         # ... and in the arithmetic
    assert out[30.0, False][0] < 4 * out[0.0, False][0] and out[30.0, False][1] < 1e-6, out
