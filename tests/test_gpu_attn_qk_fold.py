"""The K projection of single-head AttentionBlocks folded into Q (16-bit storage; csrc/attn_fold.hip), on top of the proj_out
fold of DESIGN.md 11.

    S_ij = Q_i . K_j = xn_i Wq^T Wk xn_j^T + (Wq xn_i) . bk + bq . (Wk xn_j) + bq . bk
    softmax_j(S_ij) = softmax_j(Q'_i . xn_j),   Q' = xn W'^T + c,  W' = Wk^T Wq,  c = Wk^T bq      (terms of the row i alone cancel)

The stand-alone block takes the route only under EEGLDM_ATTN_QK_FOLD=1 (networks built by eegldm_unet_create take it by default at C >= 512).
References are plain torch in float64 from the block's formulas (the unfolded ones: q, k, v, softmax, proj_out), computed once per shape and
shared by both formats.  Tolerances: gpu_util.TOL for y, GTOL for dx and every parameter gradient, and for y and dx the format bound of
test_gpu_attn_fold.py's docstring, rel-L2 <= 2^-6 (bf16) / 2^-9 (f16): the route has fewer roundings between the inputs and either tensor than
the eight counted there (K is no longer rounded as an activation; W' is rounded once as a weight).  Gradients are taken for
dy ~ N(0, 1) / sqrt(B T) as in that file.
"""
import pytest
import torch
import torch.nn.functional as F

from param_gen import normal
from test_gpu_attn_fold import RELL2, _Block, _G, _dt, _inputs, _load_all, _params, _prof_rows, _unet, _unet_inputs

pytestmark = pytest.mark.gpu


def _half_cus():
    return (torch.cuda.get_device_properties(0).multi_processor_count + 1) // 2


def _B(B):
    """"half": the smallest batch the attention kernels serve with whole-sample blocks (B >= num_cu / 2: fused dK / dV); 128 on the MI355X"""
    return _half_cus() if B == "half" else B


_REF = {}


def _reference(B, Cc, T):
    """float64 AttentionBlock (one head, unfolded formulas) forward + backward; matmul form, computed once per shape and left unchanged"""
    key = (B, Cc, T)
    if key not in _REF:
        x, dy = _inputs(B, Cc, T)
        sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in _params(Cc).items()}
        xr = x.double().requires_grad_(True)
        xn = F.group_norm(xr, 32, sd["norm.weight"], sd["norm.bias"], eps=1e-6).transpose(1, 2)        # [B][T][C]
        q, k, v = (xn @ sd["qkv.weight"][:, :, 0].t() + sd["qkv.bias"]).split(Cc, dim=2)
        p = torch.softmax((q @ k.transpose(1, 2)) * float(Cc) ** -0.5, dim=-1)
        o = p @ v
        y = xr + (o @ sd["proj_out.weight"][:, :, 0].t() + sd["proj_out.bias"]).transpose(1, 2)
        y.backward(dy.double())
        _REF[key] = (y.detach(), xr.grad.detach(), {k: v.grad.detach() for k, v in sd.items()})
    return _REF[key]


@pytest.mark.parametrize("B,Cc,T", [(2, 256, 64), (3, 512, 192), ("half", 256, 192), (2, 256, 768), (2, 512, 768)])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_block_parity_with_float64(fmt, B, Cc, T, env_switches):
    """64-row-block route (two shapes, more than one block of every kernel), whole-sample route with fused dK / dV, long variant (T = 768)
    with one and with two 256-column passes (C = 512: the pixel-space model's attention level)"""
    G = _G()
    B = _B(B)
    dt = _dt(G, fmt)
    y64, dx64, g64 = _reference(B, Cc, T)
    x, dy = _inputs(B, Cc, T)
    env_switches(EEGLDM_ATTN_QK_FOLD="1")
    blk = _Block(Cc, 1, dt)
    try:
        blk.load(_params(Cc))
        y, dx, gr = blk.run(x.to(G.DEV), dy.to(G.DEV))      # (run zeroes the gradient buffer first)
        ey, edx = G.rel_l2(y, y64), G.rel_l2(dx, dx64)
        eg = {k: G.rel_l2(gr[k], g64[k]) for k in gr if k != "qkv.bias"}
        eg["qkv.bias (q, v)"] = G.rel_l2(torch.cat([gr["qkv.bias"][:Cc], gr["qkv.bias"][2 * Cc:]]), torch.cat([g64["qkv.bias"][:Cc], g64["qkv.bias"][2 * Cc:]]))
        print(f"[numerics] attention QK fold [{fmt}] B={B} C={Cc} T={T}: rel-L2 vs float64: y {ey:.3e}, dx {edx:.3e}, "
              + ", ".join(f"{k} {v:.3e}" for k, v in eg.items()) + f"; float64 |dbk| max {float(g64['qkv.bias'][Cc:2 * Cc].abs().max()):.1e}")
        G.assert_close(y, y64.float(), **G.TOL[dt], name="y")
        G.assert_close(dx, dx64.float(), **G.GTOL[dt], name="dx")
        for k in gr:
            G.assert_close(gr[k], g64[k].float(), **G.GTOL[dt], name=f"grad {k}")
        assert ey <= RELL2[fmt] and edx <= RELL2[fmt], (ey, edx)
        # the K third of qkv.bias gets no gradient on this route (the exact gradient; the unfolded route leaves rounding noise there)
        assert torch.equal(gr["qkv.bias"][Cc:2 * Cc], torch.zeros(Cc)), float(gr["qkv.bias"][Cc:2 * Cc].abs().max())
        assert float(gr["qkv.bias"][:Cc].abs().max()) > 0.0 and float(gr["qkv.weight"][Cc:2 * Cc].abs().max()) > 0.0
    finally:
        blk.close()


def test_launch_rows_of_the_route(env_switches):
    """1-tap GEMM launches that touch the B T activation rows.  QK route: one forward row (B T) x 2C x C, backward (B T) x C x 2C (data) and
    2C x C x (B T) (weight), no row with 3C.  EEGLDM_ATTN_QK_FOLD=0: the rows of the proj_out fold alone, 3C wide."""
    G = _G()
    B, Cc, T = 4, 512, 192
    R = B * T
    x, dy = _inputs(B, Cc, T)
    xd, dyd = x.to(G.DEV), dy.to(G.DEV)
    blk = _Block(Cc, 1, G.BF16)
    c = G.ctx()
    try:
        blk.load(_params(Cc))
        for switch, W in (("1", 2 * Cc), ("0", 3 * Cc), (None, 3 * Cc)):      # (None: a stand-alone block keeps the 3C route by default)
            env_switches(EEGLDM_ATTN_QK_FOLD=switch)
            y = torch.empty(B, Cc, T, device=G.DEV); dx = torch.empty(B, Cc, T, device=G.DEV)
            try:
                c.prof_enable(True)
                G.check(G.lib.eegldm_block_forward(blk.h, G.ptr(xd), None, G.ptr(y), B, T))
                torch.cuda.synchronize()
                fwd = _prof_rows(G, c)
                c.prof_enable(True)
                G.check(G.lib.eegldm_block_backward(blk.h, G.ptr(dyd), G.ptr(dx), None))
                torch.cuda.synchronize()
                bwd = _prof_rows(G, c)
            finally:
                c.prof_enable(False)
            print(f"[route] EEGLDM_ATTN_QK_FOLD={switch}: forward rows {fwd}, backward rows {bwd}")
            rows_b = [r for r in bwd if R in r[:3]]
            assert fwd == [(R, W, Cc, 1)], fwd
            assert sorted(rows_b) == sorted([(R, Cc, W, 1), (W, Cc, R, 1)]), bwd
            if switch == "1":
                assert not any(3 * Cc in r[:3] for r in fwd + bwd), (fwd, bwd)
    finally:
        blk.close()


def test_two_backwards_accumulate(env_switches):
    """gradients accumulate across backward passes without zero_grad (the back-transform ADDS into the real slots), zeros stay zeros"""
    G = _G()
    B, Cc, T = 2, 256, 64
    x, dy = _inputs(B, Cc, T)
    x2 = torch.from_numpy(normal((B, Cc, T), seed=84)); dy2 = torch.from_numpy(normal((B, Cc, T), seed=85)) / float(B * T) ** 0.5
    env_switches(EEGLDM_ATTN_QK_FOLD="1")
    blk = _Block(Cc, 1, G.BF16)
    try:
        blk.load(_params(Cc))
        _, _, g1 = blk.run(x.to(G.DEV), dy.to(G.DEV))
        _, _, g2 = blk.run(x2.to(G.DEV), dy2.to(G.DEV))
        blk.run(x.to(G.DEV), dy.to(G.DEV))
        _, _, g12 = blk.run(x2.to(G.DEV), dy2.to(G.DEV), zero=False)
        for k in g12:
            want = g1[k].double() + g2[k].double()
            e = G.rel_l2(g12[k], want)
            print(f"[numerics] QK fold accumulation {k}: rel-L2 {e:.3e}")
            assert e <= 1e-5, (k, e)
            assert torch.equal(g12[k] == 0, want == 0), k
        assert torch.equal(g12["qkv.bias"][Cc:2 * Cc], torch.zeros(Cc))
    finally:
        blk.close()


def _rows(G, net, x, t):
    c = net.ctx
    try:
        c.prof_enable(True)
        net(x, timesteps=t); torch.cuda.synchronize()
        return _prof_rows(G, c)
    finally:
        c.prof_enable(False)


def test_no_stale_effective_weights(env_switches):
    """after an Adam step, a load_state_dict and an EMA swap-in / swap-out the forward on the QK route equals, bit for bit, the forward of a
    freshly built model given the same flat parameters (256 channels at the attention level: the route by the switch, not by default)"""
    G = _G()
    from eegldm.training import Adam, EMA
    env_switches(EEGLDM_ATTN_QK_FOLD="1")
    net = _unet(); _load_all(net, 7)
    x, dy, t = _unet_inputs(G)

    def same_as_fresh(what):
        y = net(x, timesteps=t).cpu()
        fresh = _unet(); fresh.flat.copy_(net.flat); fresh.sync_weights()
        yf = fresh(x, timesteps=t).cpu()
        assert torch.isfinite(y).all() and torch.equal(y, yf), what
        return y

    rows = _rows(G, net, x, t)
    assert sum(r == (128, 512, 256, 1) for r in rows) == 4 and sum(r == (128, 768, 256, 1) for r in rows) == 0, rows
    y0 = same_as_fresh("initial")
    ema = EMA(net, decay=0.5, warmup=False)
    opt = Adam(net, lr=1e-2, ema=ema)
    net.zero_grad(); net(x, timesteps=t); net.backward(dy); opt.step()
    y1 = same_as_fresh("Adam step")
    assert not torch.equal(y0, y1)
    with ema.applied():
        y2 = same_as_fresh("EMA swapped in")
        assert not torch.equal(y1, y2)
    assert torch.equal(same_as_fresh("EMA swapped out"), y1)
    _load_all(net, 8)
    y3 = same_as_fresh("load_state_dict")
    assert not torch.equal(y3, y1)


def test_unet_default_route(env_switches):
    """networks built by eegldm_unet_create: the QK route by default at 512 channels, the 3C route at 256; the switch decides for both"""
    G = _G()
    from eegldm.models import UNetModel
    x, _dy, t = _unet_inputs(G)
    for mc, Cc in ((128, 512), (64, 256)):
        net = UNetModel(image_size=128, in_channels=1, model_channels=mc, out_channels=1, num_res_blocks=1, attention_resolutions=[2],
                        channel_mult=[1, 4], num_heads=1, resblock_updown=True, dtype="bfloat16")
        _load_all(net, 7)
        for switch, W in ((None, 2 * Cc if Cc >= 512 else 3 * Cc), ("1", 2 * Cc), ("0", 3 * Cc)):
            env_switches(EEGLDM_ATTN_QK_FOLD=switch)
            rows = _rows(G, net, x, t)
            assert sum(r == (128, W, Cc, 1) for r in rows) == 4 and sum(r == (128, 5 * Cc - W, Cc, 1) for r in rows) == 0, (Cc, switch, rows)


def test_other_routes_are_untouched(env_switches):
    """fp32 storage, two heads and the few-row (B = 1) eval forward do not take the route: bit-identical with the switch at 1 and at 0
    (under EEGLDM_DETERMINISTIC=1: without it the bias gradients are fp32 atomics, which differ run to run in the last bit)"""
    G = _G()
    env_switches(EEGLDM_DETERMINISTIC="1")
    for Cc, heads, dt in ((256, 1, G.F32), (512, 2, G.BF16)):
        B, T = 2, 64
        x, dy = _inputs(B, Cc, T)
        blk = _Block(Cc, heads, dt)
        try:
            blk.load(_params(Cc))
            got = []
            for switch in ("1", "0"):
                env_switches(EEGLDM_ATTN_QK_FOLD=switch)
                got.append(blk.run(x.to(G.DEV), dy.to(G.DEV)))
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), (Cc, heads)
            for k in got[0][2]:
                assert torch.equal(got[0][2][k], got[1][2][k]), (Cc, heads, k)
        finally:
            blk.close()
    net = _unet(); _load_all(net, 7)
    x, _dy, t = _unet_inputs(G, B=1)
    net.eval()
    out = []
    for switch in ("1", "0"):
        env_switches(EEGLDM_ATTN_QK_FOLD=switch)
        out.append(net(x, timesteps=t).cpu())
    assert torch.equal(out[0], out[1])


def test_deterministic_mode_is_bit_reproducible(env_switches):
    """EEGLDM_DETERMINISTIC=1: two runs of the backward on the QK route give bit-equal qkv.weight and qkv.bias gradients"""
    G = _G()
    env_switches(EEGLDM_DETERMINISTIC="1", EEGLDM_ATTN_QK_FOLD="1")
    B, Cc, T = 3, 512, 192
    x, dy = _inputs(B, Cc, T)
    blk = _Block(Cc, 1, G.BF16)
    try:
        blk.load(_params(Cc))
        runs = [blk.run(x.to(G.DEV), dy.to(G.DEV))[2] for _ in range(2)]
        for k in ("qkv.weight", "qkv.bias", "proj_out.weight"):
            assert torch.equal(runs[0][k], runs[1][k]), k
        assert float(runs[0]["qkv.weight"][Cc:2 * Cc].abs().max()) > 0.0 and torch.equal(runs[0]["qkv.bias"][Cc:2 * Cc], torch.zeros(Cc))
    finally:
        blk.close()
