"""-m gpu: the fused frozen encoder (csrc/enc_fused.hip: pre_conv3_kernel, sample_stats_kernel; aekl_encode_fused_seq in csrc/aekl.hip) against
float64, kernel by kernel (eegldm_debug_pre_conv3, eegldm_debug_sample_stats) and through eegldm_aekl_encode with the route confirmed from
eegldm_debug_aekl_encode_route.  References and bounds: tests/numerics.py (pre_conv3_ref, sums_bound, enc_stats_bounds); the same checks
are held against an fp32 model of the kernel and seven planted defects in tests/test_enc_fused_numerics_cpu.py.

pre_conv3 (bf16 and fp16; 32->32, 32->64, 64->64, 64->32; (B, L) = (1, 256) one tile, (3, 512) a tile seam, (2, 768) two seams; with and
without the residual; with and without out_stats; x = scale (randn + offset) rounded to storage, offset 0, 30 and 100 sigma):
  check A   every element of y inside [RNE(y_ref - d), RNE(y_ref + d)], y_ref = conv(RNE(a)) + bias + resid in float64 on the values the kernel
            reads, d = gamma(3 Cin) mag + conv(|w|, a_hi - a_lo): the activated operand is rounded to storage inside the kernel, a point no
            test observes, so it is modelled as the interval [RNE(a - d_a), RNE(a + d_a)] with d_a the fp32 bound of the apply.
  check B   share of elements != RNE(y_ref) <= 2 m_emul + 1e-3, m_emul measured at run time on torch fp32 group_norm + SiLU -> RNE -> conv1d.
  rows      check A again on l in {0, 1, 254, 255, 256, 257, L - 2, L - 1} of every sample, one verdict per (sample, row).
  out_stats (out_stats - preload) against the float64 sums of the kernel's own stored y within pivot_sums_bounds (every lane sums its values
            about the first of them in fp32: at most 64 per lane, bounded as 64 + 6; fp64 from the lane on, atomics onto a non-zero preload).
  bits      three launches (with out_stats, without, with again) give bit-equal y.
  One case at scale 1e-3 (var ~ eps), one with a constant sample (var clamps to 0, rstd = 1 / sqrt(eps)), one NaN that must reach exactly
  the three rows that read it and its sample's out_stats.
sample_stats (n in {8, 2040, 2048, 2056, 98304}, B in {1, 3}, 0 / 30 / 100 sigma): float64 sums within sums_bound of the values about the sample's
  first element, onto a preload; n % 8 != 0 refused.
Statistics chain sample_stats -> pre_conv3(out_stats) -> pre_conv3 at (3, 512, 32->32->32), the intermediate tensor at 0 and 30 sigma: the
  (mean, rstd) a consumer derives from the produced slots against float64 within enc_stats_bounds (the hard check: what the arithmetic
  admits), and the final y through check B against the float64 chain.
Whole encoder: eegldm_aekl_encode at [32, 64] (2, 512), [32, 32, 64] (2, 1024) and [32, 32, 64] (1, 1280) (second level 640 rows: no whole
  tiles, the record must say layer-by-layer) against oracle/aekl.py in float64; yardstick the same oracle under bf16 / fp16 storage; bound
  gpu_util.bf16_gap_bound of the measured gap for z_mu and z_sigma, element-wise max and rel-L2; the layer-by-layer run
  (EEGLDM_AEKL_NO_FUSED_ENC=1) under the same bound, both ratios printed side by side; deterministic-mode encodes bit-equal (that mode
  takes the layer-by-layer path: the fp64 atomics of the fused kernels add rounded partials, whose order shows in the last bit).

Every check prints a `[numerics]` line with its worst error / bound ratio, every encoder case a `[route]` line from the record.

Worst error / bound ratios per tensor class over all cases, measured on an MI355X (bf16 | fp16) and the case that gave them.  (Check A's printed
ratio divides by half an ulp of the REFERENCE's binade + d; the verdict is the interval, whose end can lie in the next binade: 1.21 with no
element outside.)
  pre_conv3 y, check A                          1.211 (32->32 B2 L768, 30 sigma)        | 0.979 (32->64 B2 L768, 0 sigma, resid)
  pre_conv3 y, check B share / (2 m_emul + 1e-3) 0.492 (64->32 B1 L256, 0 sigma)          | 0.449 (32->32 B3 L512, 0 sigma)
      at 100 sigma, 32->64 B1 L256 fp16: 3.66e-4 of the elements off RNE(ref) where torch's fp32 emulation has 2.47e-2
  pre_conv3 seam rows                           0.990 (32->32 B1 L256, 30 sigma, resid)  | 0.970 (32->32 B3 L512, 0 sigma, resid)
  pre_conv3 out_stats against the stored y      0.003 (32->64 B1 L256, 100 sigma, resid) | 0.002 (32->32 B3 L512, 0 sigma, resid)
  sample_stats sums                             0.015 (n 2056, B 3, 0 sigma)             | 0.029 (n 8, B 1, 0 sigma)
  chain: (mean, rstd) from the produced slots   0.009 (sample_stats, 0 sigma)            | 0.011 (sample_stats, 0 sigma); at 30 sigma 0.000 | 0.002
  chain: y, check A                             0.998 (y1, 30 sigma)                     | 0.984 (y1, 30 sigma)
  chain: y, check B share / (2 m_emul + 1e-3)   0.774 (y1, 0 sigma)                      | 0.603 (y2, 0 sigma)
      y2 against the float64 chain at 30 sigma: 0.0 of the elements off (emulation 2.0e-5) | 9.8e-3 (emulation 1.75e-2)
  encoder z_mu     fused | layer-by-layer       0.585 | 0.585 ([32, 32, 64] B2 L1024)    | 0.450 | 0.445 ([32, 32, 64] B2 L1024)
  encoder z_sigma  fused | layer-by-layer       0.638 | 0.638 ([32, 32, 64] B1 L1280: both layer-by-layer) | 0.286 | 0.419 ([32, 64] B2 L512)
With the kernels as they were before this file (one-pass sums about zero, the shift beta - mean scale folded into one fp32 value) the hard checks
passed as well, and two cases failed: the chain's y2 against the float64 chain at 30 sigma in bf16 (4.27e-3 of the elements off, bound 1.04e-3:
rstd from the epilogue slots off by a relative 1.0e-5 at mean^2 / var = 992), and check B of pre_conv3 32->64 B1 L256 at 100 sigma in fp16
(5.39e-2, bound 5.04e-2).  profiles/enc_fused_numerics.txt has both sets of figures and the encode time before and after.
"""
import ctypes
import math
import os
import sys

import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

EPS = 1e-6
FMT = {1: "bf16", 2: "f16"}
SEAM_ROWS = (0, 1, 254, 255, 256, 257, -2, -1)
CHANS = [(32, 32), (32, 64), (64, 64), (64, 32)]
SHAPES = [(1, 256), (3, 512), (2, 768)]


def _G():
    import gpu_util as G
    return G


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _sums(t):
    """(B, 2) float64 (sum, sum of squares) per sample of a (B, ...) float64 tensor"""
    f = t.reshape(t.shape[0], -1)
    return torch.stack([f.sum(-1), (f * f).sum(-1)], -1)


def _operands(B, L, Cin, Cout, fmt, off, scale=1.0, seed=11, bias0=0.0):
    x = N.to_storage(scale * (_randn((B, Cin, L), seed) + off), fmt)
    assert bool(torch.isfinite(x).all()), "non-finite input"
    ga = N.rne(1 + 0.2 * _randn((Cin,), seed + 1), "f32"); be = N.rne(0.1 * _randn((Cin,), seed + 2), "f32")
    w = N.to_storage(_randn((Cout, Cin, 3), seed + 3) / math.sqrt(3 * Cin), fmt)
    bias = N.rne(bias0 + 0.1 * _randn((Cout,), seed + 4), "f32")
    resid = N.to_storage(_randn((B, Cout, L), seed + 5), fmt)
    return dict(x=x, ga=ga, be=be, w=w, bias=bias, resid=resid)


def _dev(o, dt):
    G = _G()
    f = lambda t: t.float().to(G.DEV).contiguous()
    return dict(x=G.nlc(o["x"], dt), ga=f(o["ga"]), be=f(o["be"]), w=G.pack_w(o["w"], dt), bias=f(o["bias"]), resid=G.nlc(o["resid"], dt))


def _launch(c, dt, d, in_stats, resid, out_stats, B, L, Cin, Cout):
    """one eegldm_debug_pre_conv3 launch into a NaN-filled y; returns y as (B, Cout, L) float64"""
    G = _G()
    y = torch.full((B * L, Cout), math.nan, device=G.DEV, dtype=G.TDT[dt])
    G.check(G.lib.eegldm_debug_pre_conv3(c.h, dt, G.ptr(d["x"]), G.ptr(in_stats), G.ptr(d["ga"]), G.ptr(d["be"]), G.ptr(d["w"]), G.ptr(d["bias"]),
                                         G.ptr(d["resid"]) if resid else None, G.ptr(y), G.ptr(out_stats), B, L, Cin, Cout, EPS))
    torch.cuda.synchronize()
    return G.ncl(y, B, L).double()


def _preload(B):
    return torch.tensor([[3.0, 7.0]] * B, dtype=torch.float64) * torch.arange(1, B + 1, dtype=torch.float64)[:, None]


def _check_out_stats(tag, y, got, preload, L):
    """(out_stats - preload) against the float64 sums of the stored y"""
    bounds = N.pivot_sums_bounds(y, N.pre_conv3_pivots(y), N.PRE_CONV3_STATS_DEPTH, n64=64 * 4 * (L // 256), preload=preload)
    worst = []
    for k, vals in enumerate((y, y * y)):
        err = (got[:, k] - preload[:, k] - vals.sum((1, 2))).abs()
        worst.append(float((err / bounds[k]).max()))
    print(f"[numerics] {tag} out_stats: sum {worst[0]:.3f} x bound, sum of squares {worst[1]:.3f} x bound")
    assert worst[0] <= 1 and worst[1] <= 1, f"{tag}: out_stats off the sums of the stored y ({worst[0]:.3g} x, {worst[1]:.3g} x their bounds)"


def _judge_y(tag, o, in_stats, resid, fmt, y):
    r = o["resid"] if resid else None
    y_ref, _mag, d = N.pre_conv3_ref(o["x"], in_stats, o["ga"], o["be"], o["w"], o["bias"], r, fmt, EPS)
    emul = N.pre_conv3_emul(o["x"], 1, o["ga"], o["be"], o["w"], o["bias"], r, fmt, EPS)
    fails = N.check_rows(y, y_ref, d, fmt, SEAM_ROWS, route=tag)
    assert not fails, "\n".join(fails)
    N.check(y, y_ref, d / N.gamma(0), 0, fmt, emul=emul, route=tag)


def _run_pre_conv3(tag, c, dt, o, B, L, Cin, Cout, resid):
    """the launches and checks of one operand set, with or without the residual"""
    G = _G(); fmt = FMT[dt]
    d = _dev(o, dt)
    in_stats = _sums(o["x"])
    ind = in_stats.to(G.DEV)
    pre = _preload(B)
    st = pre.to(G.DEV).clone()
    y = _launch(c, dt, d, ind, resid, st, B, L, Cin, Cout)
    y_b = _launch(c, dt, d, ind, resid, None, B, L, Cin, Cout)
    st_c = pre.to(G.DEV).clone()
    y_c = _launch(c, dt, d, ind, resid, st_c, B, L, Cin, Cout)
    assert bool(torch.isfinite(y).all()), f"{tag}: non-finite or unwritten output"
    assert torch.equal(y, y_b), f"{tag}: y differs between a launch with and one without out_stats"
    assert torch.equal(y, y_c), f"{tag}: y differs between two launches"
    _judge_y(tag, o, in_stats, resid, fmt, y)
    _check_out_stats(tag, y, st.cpu(), pre, L)
    _check_out_stats(tag + " (second launch)", y, st_c.cpu(), pre, L)


@pytest.mark.parametrize("B,L", SHAPES, ids=[f"B{b}L{l}" for b, l in SHAPES])
@pytest.mark.parametrize("Cin,Cout", CHANS, ids=[f"{a}to{b}" for a, b in CHANS])
@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_pre_conv3_against_float64(dt, Cin, Cout, B, L):
    G = _G(); c = G.ctx()
    for off in (0.0, 30.0, 100.0):
        o = _operands(B, L, Cin, Cout, FMT[dt], off)
        for resid in (False, True):
            tag = f"pre_conv3 [{FMT[dt]}] {Cin}->{Cout} B{B} L{L} mean {off:g} std{' +resid' if resid else ''}"
            _run_pre_conv3(tag, c, dt, o, B, L, Cin, Cout, resid)


@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_pre_conv3_where_var_is_eps_and_on_a_constant_sample(dt):
    G = _G(); c = G.ctx()
    B, L, Cin, Cout = 3, 512, 32, 64
    o = _operands(B, L, Cin, Cout, FMT[dt], 0.0, scale=1e-3)
    var = N.enc_affine(_sums(o["x"]), Cin * L, o["ga"], o["be"], EPS)[1]
    assert 0.5e-6 < float(var.min()) and float(var.max()) < 2e-6
    _run_pre_conv3(f"pre_conv3 [{FMT[dt]}] |x| 1e-3 (var ~ eps)", c, dt, o, B, L, Cin, Cout, True)
    o = _operands(B, L, Cin, Cout, FMT[dt], 30.0)
    o["x"][1] = 0.75
    _m, var, rstd, _s, _h = N.enc_affine(_sums(o["x"]), Cin * L, o["ga"], o["be"], EPS)
    assert float(var[1]) == 0.0 and abs(float(rstd[1]) * math.sqrt(EPS) - 1) < 1e-6
    _run_pre_conv3(f"pre_conv3 [{FMT[dt]}] constant sample (var = 0)", c, dt, o, B, L, Cin, Cout, True)


@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_pre_conv3_one_nan_reaches_its_three_rows_and_its_sample(dt):
    """in_stats are those of the clean tensor: the NaN travels through the operand alone.  Position 256 of sample 1: its three rows 255,
    256, 257 lie on both sides of a tile seam."""
    G = _G(); c = G.ctx()
    B, L, Cin, Cout = 3, 512, 32, 64
    o = _operands(B, L, Cin, Cout, FMT[dt], 0.0)
    in_stats = _sums(o["x"]).to(G.DEV)
    o["x"][1, 5, 256] = math.nan
    d = _dev(o, dt)
    pre = _preload(B); st = pre.to(G.DEV).clone()
    y = _launch(c, dt, d, in_stats, True, st, B, L, Cin, Cout)
    want = torch.zeros(B, Cout, L, dtype=torch.bool); want[1, :, 255:258] = True
    bad = torch.isnan(y) != want
    assert not bool(bad.any()), f"NaN pattern differs in {int(bad.sum())} elements ({int(torch.isnan(y).sum())} NaN, expected {int(want.sum())})"
    assert bool(torch.isfinite(y[~want]).all())
    st = st.cpu()
    assert bool(torch.isnan(st[1]).all()) and bool(torch.isfinite(st[0]).all()) and bool(torch.isfinite(st[2]).all()), st
    print(f"[nonfinite] pre_conv3 [{FMT[dt]}]: one NaN at (1, 5, 256) -> {int(want.sum())} NaN outputs in rows 255..257 of sample 1, its out_stats NaN, nothing else")


# ---------------------------------------------------------------- sample_stats
def _sample_stats(c, dt, v, preload):
    """v (B, n) float64 storage values -> the slots after one launch onto `preload`"""
    G = _G()
    B, n = v.shape
    vd = v.to(G.DEV).to(G.TDT[dt]).contiguous()
    st = preload.to(G.DEV).clone()
    G.check(G.lib.eegldm_debug_sample_stats(c.h, dt, G.ptr(vd), n, B, G.ptr(st)))
    torch.cuda.synchronize()
    return st.cpu()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [8, 2040, 2048, 2056, 98304])
def test_sample_stats_against_float64(n, B):
    G = _G(); c = G.ctx()
    depth = N.sample_stats_depth(n)
    for dt in (1, 2):
        for off in (0.0, 30.0, 100.0):
            v = N.to_storage(_randn((B, n), 21) + off, FMT[dt])
            assert bool(torch.isfinite(v).all())
            pre = _preload(B)
            got = _sample_stats(c, dt, v, pre)
            bounds = N.pivot_sums_bounds(v, v[:, :1], depth, n64=4 * 64, preload=pre)
            worst = []
            for k, vals in enumerate((v, v * v)):
                err = (got[:, k] - pre[:, k] - vals.sum(-1)).abs()
                worst.append(float((err / bounds[k]).max()))
            print(f"[numerics] sample_stats n={n} B={B} [{FMT[dt]}] mean {off:g} std: sum {worst[0]:.3f} x bound, sum of squares {worst[1]:.3f} x bound "
                  f"(depth {depth})")
            assert worst[0] <= 1 and worst[1] <= 1, (n, B, FMT[dt], off, worst)


def test_sample_stats_refuses_partial_chunks():
    G = _G(); c = G.ctx()
    v = torch.zeros(2, 2048, device=G.DEV, dtype=torch.bfloat16)
    st = torch.zeros(2, 2, device=G.DEV, dtype=torch.float64)
    for n in (2044, 7, 2041):
        assert G.lib.eegldm_debug_sample_stats(c.h, 1, G.ptr(v), n, 2, G.ptr(st)) != 0, n
    torch.cuda.synchronize()
    assert float(st.abs().sum()) == 0.0


def test_pre_conv3_refuses_what_its_eligibility_check_refuses():
    G = _G(); c = G.ctx()
    x = torch.zeros(512 * 64, device=G.DEV, dtype=torch.bfloat16); f = torch.zeros(64, device=G.DEV); st = torch.zeros(2, device=G.DEV, dtype=torch.float64)
    w = torch.zeros(3 * 64 * 64, device=G.DEV, dtype=torch.bfloat16)
    for dt, L, Cin, Cout in ((1, 128, 32, 32), (1, 384, 32, 32), (1, 256, 16, 32), (1, 256, 32, 128), (0, 256, 32, 32)):
        rc = G.lib.eegldm_debug_pre_conv3(c.h, dt, G.ptr(x), G.ptr(st), G.ptr(f), G.ptr(f), G.ptr(w), G.ptr(f), None, G.ptr(x), None, 1, L, Cin, Cout, EPS)
        assert rc == -3, (dt, L, Cin, Cout, rc)


# ---------------------------------------------------------------- the statistics chain
@pytest.mark.parametrize("off", [0.0, 30.0], ids=["mean0", "mean30"])
@pytest.mark.parametrize("dt", [1, 2], ids=["bf16", "f16"])
def test_statistics_chain(dt, off):
    """sample_stats -> pre_conv3 (out_stats) -> pre_conv3 on the produced statistics.  x and, through the first conv's bias, the intermediate
    tensor y1 sit `off` standard deviations from zero: the epilogue sums of pre_conv3 then carry the mean^2 / var amplification."""
    G = _G(); c = G.ctx(); fmt = FMT[dt]
    B, L, C = 3, 512, 32
    n = C * L
    o1 = _operands(B, L, C, C, fmt, off, seed=31, bias0=0.6 * off)          # (the conv of a unit-variance activated tensor has a deviation of ~0.6)
    o2 = _operands(B, L, C, C, fmt, 0.0, seed=41)
    d1, d2 = _dev(o1, dt), _dev(o2, dt)
    tag = f"chain [{fmt}] mean {off:g} std"
    # ---- sample_stats
    xs = o1["x"].permute(0, 2, 1).reshape(B, n)
    s0 = _sample_stats(c, dt, xs, torch.zeros(B, 2, dtype=torch.float64))
    b0 = N.enc_stats_bounds(xs, N.sample_stats_depth(n), EPS, n64=4 * 64, pivot=xs[:, :1])
    m0, _v0, r0, _sc, _sh = N.enc_affine(s0, n, o1["ga"], o1["be"], EPS)
    e_m, e_r = float(((m0 - b0["mean"]).abs() / b0["e_mean"]).max()), float(((r0 / b0["rstd"] - 1).abs() / b0["e_rstd"]).max())
    print(f"[numerics] {tag} sample_stats slots: mean {e_m:.3f} x bound, rstd {e_r:.3f} x bound (rstd bound {float(b0['e_rstd'].max()):.2e}, "
          f"measured {float((r0 / b0['rstd'] - 1).abs().max()):.2e}, mean^2 / var {float((b0['mean'] ** 2 / b0['var']).max()):.3g})")
    assert e_m <= 1 and e_r <= 1, f"{tag}: statistics of sample_stats outside their bound"
    # ---- first pre_conv3: reads the slots sample_stats produced, leaves the slots of y1
    s0d = s0.to(G.DEV); s1d = torch.zeros(B, 2, device=G.DEV, dtype=torch.float64)
    y1 = _launch(c, dt, d1, s0d, False, s1d, B, L, C, C)
    s1 = s1d.cpu()
    _judge_y(tag + " y1 (kernel's slots)", o1, s0, False, fmt, y1)
    b1 = N.enc_stats_bounds(y1, N.PRE_CONV3_STATS_DEPTH, EPS, n64=64 * 4 * (L // 256), pivot=N.pre_conv3_pivots(y1))
    m1, _v1, r1, _sc, _sh = N.enc_affine(s1, n, o2["ga"], o2["be"], EPS)
    e_m, e_r = float(((m1 - b1["mean"]).abs() / b1["e_mean"]).max()), float(((r1 / b1["rstd"] - 1).abs() / b1["e_rstd"]).max())
    print(f"[numerics] {tag} pre_conv3 slots: mean {e_m:.3f} x bound, rstd {e_r:.3f} x bound (rstd bound {float(b1['e_rstd'].max()):.2e}, "
          f"measured {float((r1 / b1['rstd'] - 1).abs().max()):.2e}, mean^2 / var {float((b1['mean'] ** 2 / b1['var']).max()):.3g})")
    assert e_m <= 1 and e_r <= 1, f"{tag}: statistics from the pre_conv3 epilogue outside their bound"
    if off:
        assert float((b1["mean"] ** 2 / b1["var"]).min()) > 0.25 * off ** 2, "the intermediate tensor does not sit where the case wants it"
    # ---- second pre_conv3 on the produced statistics
    o2["x"] = y1
    d2["x"] = G.nlc(y1, dt)
    y2 = _launch(c, dt, d2, s1d, True, None, B, L, C, C)
    _judge_y(tag + " y2 (kernel's slots)", o2, s1, True, fmt, y2)                    # hard: float64 on the slots the kernel read
    exact = _sums(y1)
    y_ref, _mag, _d = N.pre_conv3_ref(y1, exact, o2["ga"], o2["be"], o2["w"], o2["bias"], o2["resid"], fmt, EPS)
    emul = N.pre_conv3_emul(y1, 1, o2["ga"], o2["be"], o2["w"], o2["bias"], o2["resid"], fmt, EPS)
    N.check_b(y2, y_ref, emul, fmt, route=tag + " y2 against the float64 chain")


# ---------------------------------------------------------------- the whole encoder
ENCODERS = [([32, 64], 2, 512, True), ([32, 32, 64], 2, 1024, True), ([32, 32, 64], 1, 1280, False)]
_ORACLE = {}


def _net(channels, dtype, seed=0):
    from eegldm.models import AutoencoderKL
    ae = AutoencoderKL(spatial_dims=1, in_channels=1, out_channels=1, num_channels=channels, latent_channels=1, num_res_blocks=2,
                       norm_num_groups=1, attention_levels=[False] * len(channels), dtype=dtype)
    g = torch.Generator().manual_seed(seed)
    new = {}
    for k, v in ae.state_dict().items():
        if v.dim() == 1 and k.endswith(".weight"):
            new[k] = 1.0 + 0.2 * torch.randn(v.shape, generator=g)
        elif v.dim() == 1:
            new[k] = 0.1 * torch.randn(v.shape, generator=g)
        else:
            new[k] = torch.randn(v.shape, generator=g) / (v.shape[1] * v.shape[2]) ** 0.5
    ae.load_state_dict(new)
    return ae


def _oracle(channels, B, L, dtype, sd):
    """(x, (mu, sigma) float64, (mu, sigma) of the same oracle with `dtype` storage), computed once per case and left unchanged"""
    key = (tuple(channels), B, L, dtype)
    if key not in _ORACLE:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from oracle import aekl as O
        from oracle import quant as Q
        cfg = dict(num_channels=channels, num_res_blocks=2, norm_num_groups=1)
        x = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(9))
        with torch.no_grad():
            ref = O.encode({k: v.double() for k, v in sd.items()}, cfg, x.double())
            with (Q.bf16_storage(True) if dtype == "bfloat16" else Q.f16_storage(True)):
                yard = O.encode(sd, cfg, x)
        _ORACLE[key] = (x, ref, tuple(t.double() for t in yard))
    return _ORACLE[key]


def _enc_route(ae):
    G = _G()
    out = (ctypes.c_int * 3)()
    G.check(G.lib.eegldm_debug_aekl_encode_route(ae.h, out))
    return dict(fused=out[0], pre_conv3=out[1], sample_stats=out[2])


def _errs(got, ref):
    return float((got - ref).abs().max() / ref.abs().max()), float((got - ref).norm() / ref.norm())


@pytest.mark.parametrize("channels,B,L,fused", ENCODERS, ids=["32_64-L512", "32_32_64-L1024", "32_32_64-L1280-not-eligible"])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_encoder_against_float64_oracle(dtype, channels, B, L, fused, env_switches):
    G = _G()
    ae = _net(channels, dtype)
    sd = {k: v.detach().cpu().float() for k, v in ae.state_dict().items()}
    x, ref, yard = _oracle(channels, B, L, dtype, sd)
    floor = G.BF16_FLOOR if dtype == "bfloat16" else G.F16_FLOOR
    tag = f"encoder {channels} B{B} L{L} [{dtype}]"
    runs = {}
    for mode in ("fused", "layerwise"):
        env_switches(EEGLDM_AEKL_NO_FUSED_ENC="1" if mode == "layerwise" else None)
        mu, sg = ae.encode(x.to(G.DEV))
        torch.cuda.synchronize()
        r = _enc_route(ae)
        print(f"[route] {tag} {mode}: {'fused' if r['fused'] else 'layer-by-layer'} pre_conv3 launches {r['pre_conv3']} sample_stats launches {r['sample_stats']}")
        if mode == "fused" and fused:
            nres = 2 * len(channels)
            assert r == dict(fused=1, pre_conv3=2 * nres, sample_stats=len(channels)), f"{tag}: the fused path did not run as planned: {r}"
        else:
            assert r == dict(fused=0, pre_conv3=0, sample_stats=0), f"{tag}: expected the layer-by-layer path, got {r}"
        runs[mode] = (mu.double().cpu(), sg.double().cpu())
    env_switches(EEGLDM_AEKL_NO_FUSED_ENC=None)
    bad = []
    for i, name in enumerate(("z_mu", "z_sigma")):
        gap = _errs(yard[i], ref[i])
        ratios = {}
        for mode in runs:
            e = _errs(runs[mode][i], ref[i])
            ratios[mode] = tuple(e[k] / G.bf16_gap_bound(gap[k], floor=floor) for k in range(2))
            for k, what in enumerate(("max", "rel-L2")):
                if not ratios[mode][k] <= 1:
                    bad.append(f"{name} {mode} {what}: error {e[k]:.3e}, storage gap {gap[k]:.3e}, bound {G.bf16_gap_bound(gap[k], floor=floor):.3e}")
        print(f"[numerics] {tag} {name}: error / bound  max fused {ratios['fused'][0]:.3f} | layer-by-layer {ratios['layerwise'][0]:.3f}   "
              f"rel-L2 fused {ratios['fused'][1]:.3f} | layer-by-layer {ratios['layerwise'][1]:.3f}   (storage gap max {gap[0]:.2e} rel-L2 {gap[1]:.2e})")
    assert not bad, f"{tag}:\n  " + "\n  ".join(bad)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_deterministic_mode_fused_encodes_are_bit_equal(dtype, env_switches):
    G = _G()
    env_switches(EEGLDM_DETERMINISTIC="1")
    ae = _net([32, 32, 64], dtype)
    x = torch.randn(2, 1, 1024, generator=torch.Generator().manual_seed(9)).to(G.DEV)
    outs = []
    for _ in range(3):
        mu, sg = ae.encode(x)
        torch.cuda.synchronize()
        r = _enc_route(ae)
        outs.append((mu.cpu(), sg.cpu(), r))
    print(f"[route] deterministic mode [{dtype}]: {outs[0][2]}")
    for mu, sg, r in outs[1:]:
        assert r == outs[0][2]
        assert torch.equal(mu, outs[0][0]) and torch.equal(sg, outs[0][1]), f"deterministic mode: two encodes differ ({r})"
