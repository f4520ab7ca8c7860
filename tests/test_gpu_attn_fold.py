"""proj_out folded into the V projection of single-head AttentionBlocks (16-bit storage; csrc/attn_fold.hip).

    out = x + (P V) Wp^T + bp = x + P (xn Wvp^T + bv'),   Wvp = Wp Wv,  bv' = Wp bv + bp        (softmax rows of P sum to 1)

References are plain torch in float64 from the block's formulas, computed once per shape.  Shapes: C = 256 and 512 (the fused attention
kernel, which the fold needs, takes head widths that are multiples of 256), T = 64 and 192, B = 2-4: more than one block of every kernel.
Gradients are taken for dy ~ N(0, 1) / sqrt(B T), so that the weight gradients (sums over B T rows) are O(1) like the activations and
gpu_util.GTOL's absolute term means the same for them; dx is then small against that term, so y and dx are also held to a rel-L2 bound
from the format alone: at most 8 roundings to 16 bits lie between the inputs and either tensor (x, xn, qkv, P, out / dout, dqkv, dS, dxn),
each of relative size <= 2^-9 (bf16) or 2^-12 (f16), and rounding errors add at most linearly: 8 x 2^-9 = 2^-6, 8 x 2^-12 = 2^-9.
"""
import csv
import ctypes as C
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

from param_gen import gen_param, normal

pytestmark = pytest.mark.gpu

RELL2 = {"bf16": 2.0 ** -6, "f16": 2.0 ** -9}


def _G():
    import gpu_util as G
    return G


def _dt(G, fmt):
    return {"bf16": G.BF16, "f16": G.F16, "f32": G.F32}[fmt]


class _Block:
    """one eegldm_block (AttentionBlock): entry table, flat parameter / gradient buffers"""

    def __init__(self, channels, heads, dt):
        G = _G()
        h = C.c_void_p()
        G.check(G.lib.eegldm_attnblock_create(G.ctx().h, channels, heads, dt, C.byref(h)))
        self.h = h
        n = int(G.lib.eegldm_block_num_params(h))
        name = C.create_string_buffer(256)
        off, numel, ndim, shape = C.c_long(), C.c_long(), C.c_int(), (C.c_int * 3)()
        self.entries = {}
        for i in range(G.lib.eegldm_block_num_entries(h)):
            G.check(G.lib.eegldm_block_entry(h, i, name, 256, C.byref(off), C.byref(numel), C.byref(ndim), shape))
            self.entries[name.value.decode()] = (off.value, numel.value, tuple(shape[k] for k in range(ndim.value)))
        self.flat = torch.zeros(n, device=G.DEV)
        self.grad = torch.zeros(n, device=G.DEV)

    def load(self, sd):
        G = _G()
        for k, (o, n, shape) in self.entries.items():
            v = torch.as_tensor(sd[k]).float()
            if len(shape) == 3:
                v = v.permute(2, 0, 1)
            self.flat[o:o + n].copy_(v.reshape(-1).to(G.DEV))
        G.check(G.lib.eegldm_block_bind(self.h, G.ptr(self.flat), G.ptr(self.grad)))

    def grads(self):
        out = {}
        for k, (o, n, shape) in self.entries.items():
            t = self.grad[o:o + n]
            if len(shape) == 3:
                t = t.reshape(shape[2], shape[0], shape[1]).permute(1, 2, 0)
            out[k] = t.reshape(shape).cpu().clone()
        return out

    def run(self, x, dy, zero=True):
        """forward + backward; returns (y, dx, parameter gradients) on the host"""
        G = _G()
        B, Cc, T = x.shape
        y = torch.empty(B, Cc, T, device=G.DEV); dx = torch.empty(B, Cc, T, device=G.DEV)
        if zero:
            self.grad.zero_()
        G.check(G.lib.eegldm_block_forward(self.h, G.ptr(x), None, G.ptr(y), B, T))
        G.check(G.lib.eegldm_block_backward(self.h, G.ptr(dy), G.ptr(dx), None))
        return y.cpu(), dx.cpu(), self.grads()

    def close(self):
        _G().lib.eegldm_block_destroy(self.h)


def _params(channels, seed=81):
    shapes = {"norm.weight": (channels,), "norm.bias": (channels,), "qkv.weight": (3 * channels, channels, 1), "qkv.bias": (3 * channels,),
              "proj_out.weight": (channels, channels, 1), "proj_out.bias": (channels,)}
    return {k: gen_param(seed, k, s) for k, s in shapes.items()}      # (every bias non-zero: 0.1 N(0, 1))


def _inputs(B, Cc, T):
    x = torch.from_numpy(normal((B, Cc, T), seed=82))
    dy = torch.from_numpy(normal((B, Cc, T), seed=83)) / float(B * T) ** 0.5
    return x, dy


_REF = {}


def _reference(B, Cc, T):
    """float64 AttentionBlock (one head) forward + backward from the formulas; computed once per shape and left unchanged"""
    key = (B, Cc, T)
    if key not in _REF:
        x, dy = _inputs(B, Cc, T)
        sd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in _params(Cc).items()}
        xr = x.double().requires_grad_(True)
        xn = F.group_norm(xr, 32, sd["norm.weight"], sd["norm.bias"], eps=1e-6)
        q, k, v = F.conv1d(xn, sd["qkv.weight"], sd["qkv.bias"]).split(Cc, dim=1)
        s = float(Cc) ** -0.25
        p = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
        o = torch.einsum("bts,bcs->bct", p, v)
        y = xr + F.conv1d(o, sd["proj_out.weight"], sd["proj_out.bias"])
        y.backward(dy.double())
        _REF[key] = (y.detach(), xr.grad.detach(), {k: v.grad.detach() for k, v in sd.items()})
    return _REF[key]


def _prof_rows(G, c):
    path = os.path.join(tempfile.gettempdir(), f"eegldm_fold_rows_{os.getpid()}.csv")
    G.check(G.lib.eegldm_prof_dump(c.h, path.encode()))
    try:
        with open(path) as fh:
            return [(int(r["M"]), int(r["N"]), int(r["K"]), int(r["taps"])) for r in csv.DictReader(fh)]
    finally:
        os.unlink(path)


@pytest.mark.parametrize("B,Cc,T", [(2, 256, 64), (3, 512, 192)])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_block_parity_with_float64(fmt, B, Cc, T, env_switches):
    G = _G()
    dt = _dt(G, fmt)
    y64, dx64, g64 = _reference(B, Cc, T)
    x, dy = _inputs(B, Cc, T)
    blk = _Block(Cc, 1, dt)
    try:
        blk.load(_params(Cc))
        for label, switch in (("folded", None), ("unfolded", "1")):
            env_switches(EEGLDM_NO_ATTN_FOLD=switch)
            y, dx, gr = blk.run(x.to(G.DEV), dy.to(G.DEV))
            ey, edx = G.rel_l2(y, y64), G.rel_l2(dx, dx64)
            eg = {k: G.rel_l2(gr[k], g64[k]) for k in gr}
            print(f"[numerics] attention fold [{fmt}] B={B} C={Cc} T={T} {label}: rel-L2 vs float64: y {ey:.3e}, dx {edx:.3e}, "
                  + ", ".join(f"{k} {v:.3e}" for k, v in eg.items()))
            G.assert_close(y, y64.float(), **G.TOL[dt], name=f"{label} y")
            G.assert_close(dx, dx64.float(), **G.GTOL[dt], name=f"{label} dx")
            for k in gr:
                G.assert_close(gr[k], g64[k].float(), **G.GTOL[dt], name=f"{label} grad {k}")
            assert ey <= RELL2[fmt] and edx <= RELL2[fmt], (label, ey, edx)
    finally:
        blk.close()


def test_launch_counts_of_a_folded_block(env_switches):
    """1-tap GEMM launches that touch the B T activation rows: folded 1 forward (qkv) + 2 backward (qkv data and weight gradient), none of
    M x N x K = (B T) x C x C; unfolded 2 + 4.  A forward row count of exactly 1 also shows that the fused attention kernel served the block
    (the composition adds two batched GEMM rows)."""
    G = _G()
    B, Cc, T = 4, 512, 192
    R = B * T
    x, dy = _inputs(B, Cc, T)
    xd, dyd = x.to(G.DEV), dy.to(G.DEV)
    blk = _Block(Cc, 1, G.BF16)
    c = G.ctx()
    try:
        blk.load(_params(Cc))
        for switch, nf, nb in ((None, 1, 2), ("1", 2, 4)):
            env_switches(EEGLDM_NO_ATTN_FOLD=switch)
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
            print(f"[route] fold {'off' if switch else 'on'}: forward rows {fwd}, backward rows {bwd}")
            rows_f = [r for r in fwd if R in r[:3]]; rows_b = [r for r in bwd if R in r[:3]]
            assert all(r[3] == 1 for r in rows_f + rows_b)
            assert len(fwd) == nf and len(rows_f) == nf, fwd
            assert len(rows_b) == nb, bwd
            assert (R, 3 * Cc, Cc, 1) in rows_f and (R, Cc, 3 * Cc, 1) in rows_b and (3 * Cc, Cc, R, 1) in rows_b
            square = [r for r in fwd + bwd if sorted(r[:3]) == sorted((R, Cc, Cc))]
            assert (len(square) == 0) if switch is None else (len(square) == 3), square
    finally:
        blk.close()


def test_two_backwards_accumulate(env_switches):
    """gradients accumulate across backward passes without zero_grad: the back-transform ADDS into the real slots"""
    G = _G()
    B, Cc, T = 2, 256, 64
    x, dy = _inputs(B, Cc, T)
    x2 = torch.from_numpy(normal((B, Cc, T), seed=84)); dy2 = torch.from_numpy(normal((B, Cc, T), seed=85)) / float(B * T) ** 0.5
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
            print(f"[numerics] accumulation {k}: rel-L2 {e:.3e}")
            assert e <= 1e-5, (k, e)
            assert torch.equal(g12[k] == 0, want == 0), k
    finally:
        blk.close()


def _unet(dtype="bfloat16"):
    """smallest UNet whose AttentionBlocks fold: 256 channels at the attention level (T = L / 2 = 64), four such blocks"""
    from eegldm.models import UNetModel
    return UNetModel(image_size=128, in_channels=1, model_channels=64, out_channels=1, num_res_blocks=1, attention_resolutions=[2],
                     channel_mult=[1, 4], num_heads=1, resblock_updown=True, dtype=dtype)


def _unet_inputs(G, B=2, L=128):
    x = torch.from_numpy(normal((B, 1, L), seed=91)).to(G.DEV)
    dy = torch.from_numpy(normal((B, 1, L), seed=92)).to(G.DEV) / float(B * L) ** 0.5
    t = torch.tensor([17, 640][:B], dtype=torch.int64, device=G.DEV)
    return x, dy, t


def _load_all(net, seed):
    net.load_state_dict({k: torch.from_numpy(gen_param(seed, k, shape)) for k, (_o, _n, shape) in net.entries.items()})


def test_unfolded_routes_are_untouched(env_switches):
    """fp32 storage, two heads and the few-row eval forward do not fold: bit-identical with the switch on and off.  (The blocks run under
    EEGLDM_DETERMINISTIC=1: without it the bias gradients are fp32 atomics, which differ run to run in the last bit on the parent too.)"""
    G = _G()
    env_switches(EEGLDM_DETERMINISTIC="1")
    for Cc, heads, dt in ((256, 1, G.F32), (512, 2, G.BF16)):
        B, T = 2, 64
        x, dy = _inputs(B, Cc, T)
        blk = _Block(Cc, heads, dt)
        try:
            blk.load(_params(Cc))
            got = []
            for switch in (None, "1"):
                env_switches(EEGLDM_NO_ATTN_FOLD=switch)
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
    for switch in (None, "1"):
        env_switches(EEGLDM_NO_ATTN_FOLD=switch)
        out.append(net(x, timesteps=t).cpu())
    assert torch.equal(out[0], out[1])


def test_no_stale_effective_weights():
    """after an Adam step, a load_state_dict and an EMA swap-in / swap-out the folded forward equals, bit for bit, the forward of a freshly
    built model given the same flat parameters"""
    G = _G()
    from eegldm.training import Adam, EMA
    net = _unet(); _load_all(net, 7)
    x, dy, t = _unet_inputs(G)
    c = net.ctx

    def same_as_fresh(what):
        y = net(x, timesteps=t).cpu()
        fresh = _unet(); fresh.flat.copy_(net.flat); fresh.sync_weights()
        yf = fresh(x, timesteps=t).cpu()
        assert torch.isfinite(y).all() and torch.equal(y, yf), what
        return y

    # the route: no 1-tap launch of proj_out's shape (B T) x C x C at the attention level, one qkv launch per block
    try:
        c.prof_enable(True)
        net(x, timesteps=t); torch.cuda.synchronize()
        rows = _prof_rows(G, c)
    finally:
        c.prof_enable(False)
    assert sum(r == (128, 768, 256, 1) for r in rows) == 4 and sum(r == (128, 256, 256, 1) for r in rows) == 0, rows
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


def test_deterministic_mode_is_bit_reproducible(env_switches):
    """EEGLDM_DETERMINISTIC=1: two runs of forward + backward give bit-identical gradients (grouped flush + back-transform included)"""
    G = _G()
    env_switches(EEGLDM_DETERMINISTIC="1")
    net = _unet(); _load_all(net, 7)
    x, dy, t = _unet_inputs(G)
    runs = []
    for _ in range(2):
        net.zero_grad(); net(x, timesteps=t); dx = net.backward(dy, need_dx=True)
        runs.append((net.flat_grad.cpu().clone(), dx.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    o, n, _s = net.entries["middle_block.1.proj_out.weight"]
    assert float(runs[0][0][o:o + n].abs().max()) > 0.0
