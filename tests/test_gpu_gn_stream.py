"""-m gpu: the full-slab (straight-line) body of the resident GroupNorm backward against the predicated body it stands in for
(csrc/norm.hip: gn_bwd_resident_full_kernel, switch EEGLDM_GN_NO_STREAM=1).  The forward has one body (a straight-line form measured no
faster and was not kept); its outputs are compared all the same, so that the switch is seen to leave it alone.

The full-slab body keeps the arithmetic, the thread-to-data mapping and the launch geometry of the predicated one; what changes is the
order and the counting of the memory operations.  So the check is bit identity, not a bound: every output of eegldm_groupnorm_fwd /
eegldm_groupnorm_bwd with the switch unset equals the output with EEGLDM_GN_NO_STREAM=1 bit for bit, under EEGLDM_DETERMINISTIC=1 (one writer
per dgamma / dbeta partial; the default mode folds them with fp32 atomics whose order is the hardware's), and both runs report the same
route (eegldm_debug_gn_last_route).  The float64 bounds of these routes are tests/test_gpu_groupnorm_rounding.py's.

Shapes (B, L, C, G) -- the smallest that reach each instantiation at 1024 threads and 256-channel chunks (16 row lanes):
  (3, 192, 256, 32)  full slab at 12 rows per thread;   (3, 96, 256, 32)  full slab at 6;
  (3, 160, 256, 32)  10 rows of the 12-row instantiation: NOT a full slab, the predicated body with or without the switch.
Three samples put more than one block on a slot of the partial sums (b % nslot).  fp32 runs the first shape only (two-pass forward; its
backward takes 128-channel chunks, 6 rows of the 8-row instantiation, i.e. the predicated body).
The public entry points have no second addend and no per-sample column sums: those instantiations are reached by the UNet test at the end
(ResBlocks pass the skip gradient as the second addend and take the bias gradient of the preceding convolution from the column sums)."""
import ctypes
import itertools
import math

import pytest
import torch

from param_gen import gen_param, normal

pytestmark = pytest.mark.gpu

EPS = 1e-6
RESIDENT = 2
ENV = {"EEGLDM_GN_NO_FEW_SLAB_NARROW": "1", "EEGLDM_DETERMINISTIC": "1"}     # B = 3 would take the 256-thread forward otherwise
SHAPES = {"full R12": ((3, 192, 256, 32), 12), "full R6": ((3, 96, 256, 32), 6), "row tail L160": ((3, 160, 256, 32), 12)}
CASES = [(name, dt) for name in SHAPES for dt in (1, 2)] + [("full R12", 0)]
COMBOS = list(itertools.product((0, 1), (0, 1, 2), (False, True)))      # silu, resample, first addend


def _G():
    import gpu_util as G
    return G


def _route(G, backward):
    out = (ctypes.c_int * 6)()
    G.check(G.lib.eegldm_debug_gn_last_route(backward, out))
    return tuple(out)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


_INPUTS = {}


def _inputs(shape, rs):
    """(x, dy, dxr, gamma, beta) as float32 NCL / per-channel CPU tensors, made once per (shape, resample)"""
    if (shape, rs) not in _INPUTS:
        B, L, C, _g = shape
        Lo = L // 2 if rs == 1 else (2 * L if rs == 2 else L)
        g = torch.Generator().manual_seed(1000 + L + rs)
        r = lambda *s: torch.randn(*s, generator=g)
        _INPUTS[(shape, rs)] = (0.5 + r(B, C, L), r(B, C, Lo), r(B, C, Lo), 1 + 0.1 * r(C), 0.1 * r(C))
    return _INPUTS[(shape, rs)]


def _run(G, c, shape, dt, silu, rs, addend, poison=False):
    """one forward and one backward through the public entry points; every output as raw bits, plus the two route records"""
    B, L, C, Gr = shape
    Lo = L // 2 if rs == 1 else (2 * L if rs == 2 else L)
    x, dy, dxr, ga, be = _inputs(shape, rs)
    if poison:
        x = x.clone(); dy = dy.clone()
        x[0, C // Gr + 1, 5] = math.nan      # inside group 1 of sample 0, off its pivot element
        dy[B - 1, C - 3, 7] = math.inf       # last group of the last sample
    xd, dyd = G.nlc(x, dt), G.nlc(dy, dt)
    dxrd = G.nlc(dxr, dt) if addend else None
    gad, bed = ga.to(G.DEV), be.to(G.DEV)
    nan = lambda rows: torch.full((rows, C), math.nan, device=G.DEV, dtype=G.TDT[dt])      # an unwritten element shows
    y, xr, dx = nan(B * Lo), (nan(B * Lo) if rs else None), nan(B * L)
    st = torch.full((B * Gr * 2,), math.nan, device=G.DEV)
    G.check(G.lib.eegldm_groupnorm_fwd(c.h, G.ptr(xd), C, G.ptr(gad), G.ptr(bed), G.ptr(y), C, G.ptr(st), B, L, C, Gr, EPS, silu, rs,
                                       G.ptr(xr) if rs else None, C if rs else 0, dt))
    dga = torch.zeros(C, device=G.DEV); dbe = torch.zeros(C, device=G.DEV)
    G.check(G.lib.eegldm_groupnorm_bwd(c.h, G.ptr(xd), C, G.ptr(gad), G.ptr(bed), G.ptr(st), G.ptr(dyd), C, G.ptr(dx), C,
                                       G.ptr(dga), G.ptr(dbe), B, L, C, Gr, silu, rs, G.ptr(dxrd) if addend else None, C if addend else 0, dt))
    torch.cuda.synchronize()
    out = dict(y=y, stats=st, dx=dx, dgamma=dga, dbeta=dbe)
    if rs:
        out["xr"] = xr
    return {k: _bits(v) for k, v in out.items()}, _route(G, 0), _route(G, 1)


@pytest.mark.parametrize("name,dt", CASES, ids=[f"{n} {('f32', 'bf16', 'f16')[d]}" for n, d in CASES])
def test_full_slab_bodies_are_bit_identical(name, dt, env_switches):
    G = _G(); c = G.ctx()
    shape, rpt = SHAPES[name]
    for silu, rs, addend in COMBOS:
        tag = f"{name} dt{dt} silu{silu} resample{rs} addend{int(addend)}"
        got = []
        for switch in (None, "1"):
            env_switches(**ENV, EEGLDM_GN_NO_STREAM=switch)
            got.append(_run(G, c, shape, dt, silu, rs, addend))
        (new, rf_new, rb_new), (old, rf_old, rb_old) = got
        assert rf_new == rf_old and rb_new == rb_old, f"{tag}: route differs with the switch: {rf_new} {rb_new} vs {rf_old} {rb_old}"
        for r in (rf_new, rb_new):
            assert r[0] == RESIDENT and r[2] == 1024, f"{tag}: not the resident family at 1024 threads: {r}"
        assert rf_new[3] == rpt, f"{tag}: forward rows per thread {rf_new[3]}, expected {rpt}"
        if dt != 0:
            assert rb_new[3] == rpt and rb_new[4] == 256, f"{tag}: backward route {rb_new}, expected {rpt} rows per thread and 256-channel chunks"
        for k in new:
            assert torch.equal(new[k], old[k]), f"{tag}: {k} differs in {int((new[k] != old[k]).sum())} of {new[k].numel()} elements"
            vals = new[k].view({0: torch.float32, 1: torch.bfloat16, 2: torch.float16}[dt] if k in ("y", "dx", "xr") else torch.float32)
            assert bool(torch.isfinite(vals.float()).all()), f"{tag}: {k} has an unwritten or non-finite element"


@pytest.mark.parametrize("dt", (1, 2), ids=("bf16", "f16"))
def test_nonfinite_reaches_the_same_elements(dt, env_switches):
    """a NaN in x and an inf in dy make the same output elements non-finite in both bodies (raw bits equal, NaN payloads included),
    and stay inside their (sample, group): some elements are non-finite, not all"""
    G = _G(); c = G.ctx()
    shape, _rpt = SHAPES["full R12"]
    tdt = torch.bfloat16 if dt == 1 else torch.float16
    for silu, rs, addend in ((1, 0, True), (0, 0, False), (1, 2, True), (1, 1, False)):
        got = []
        for switch in (None, "1"):
            env_switches(**ENV, EEGLDM_GN_NO_STREAM=switch)
            got.append(_run(G, c, shape, dt, silu, rs, addend, poison=True)[0])
        for k in got[0]:
            assert torch.equal(got[0][k], got[1][k]), f"silu{silu} resample{rs}: {k} differs between the bodies on non-finite input"
        for k in ("y", "dx"):
            bad = ~torch.isfinite(got[0][k].view(tdt).float())
            assert bool(bad.any()) and not bool(bad.all()), f"silu{silu} resample{rs}: {k} has {int(bad.sum())} of {bad.numel()} non-finite elements"


@pytest.mark.parametrize("L", (128, 192))
def test_unet_level_is_bit_identical(L, env_switches):
    """one forward and backward of the 256-channel toy UNet (tests/test_gpu_attn_fold.py::_unet), deterministic mode: the parameter
    gradients and dx are bit-equal with the switch on and off.  Its ResBlocks hand the backward the second addend and the column sums.
    L = 128 is that test's size (64 rows at the 256-channel level: 4 rows of the 6-row instantiation, the predicated body either way);
    at L = 192 the level has 96 rows = 6 x 16, full slabs, so the two-addend and column-sum instantiations of the new body run."""
    from eegldm.models import UNetModel
    G = _G()
    env_switches(EEGLDM_DETERMINISTIC="1")
    net = UNetModel(image_size=L, in_channels=1, model_channels=64, out_channels=1, num_res_blocks=1, attention_resolutions=[2],
                    channel_mult=[1, 4], num_heads=1, resblock_updown=True, dtype="bfloat16")
    net.load_state_dict({k: torch.from_numpy(gen_param(7, k, shape)) for k, (_o, _n, shape) in net.entries.items()})
    B = 2
    x = torch.from_numpy(normal((B, 1, L), seed=91)).to(G.DEV)
    dy = torch.from_numpy(normal((B, 1, L), seed=92)).to(G.DEV) / float(B * L) ** 0.5
    t = torch.tensor([17, 640], dtype=torch.int64, device=G.DEV)
    runs = []
    for switch in (None, "1"):
        env_switches(EEGLDM_GN_NO_STREAM=switch)
        net.zero_grad(); net(x, timesteps=t); dx = net.backward(dy, need_dx=True)
        runs.append((net.flat_grad.cpu().clone(), dx.cpu().clone()))
    assert torch.equal(runs[0][0], runs[1][0]), f"flat_grad differs in {int((runs[0][0] != runs[1][0]).sum())} elements"
    assert torch.equal(runs[0][1], runs[1][1]), "dx differs"
    assert float(runs[0][0].abs().max()) > 0.0
