"""CPU: the float64 ResBlock reference of tests/resblock_reference.py and the checks of tests/test_gpu_resblock_rounding.py, judged
without a device.

1. The reference is pinned to tests/golden/resblocks.npz and blocks_r6.npz (the imported reference's own numbers) at those files' inputs,
   and its float32 yardstick to a direct call of oracle.unet.resblock.
2. A stand-in engine -- the storage-emulating float32 oracle (the plain float32 oracle for an fp32 engine) evaluated in another summation
   order: batch and channel order reversed, then undone, its parameter gradients added onto the preloaded contents in fp32 -- passes
   every check A to D, and E with a NaN in dy.
3. Planted faults: each must fail at least one check, and the test says which.
   (a) out_layers.3.bias gradient doubled                                        -> B (and A)
   (b) one sample's per-sample sums zeroed                                       -> C
   (c) channels [64, 128) of the in_layers.2.bias gradient dropped               -> D
   (d) scale and shift halves of the emb_layers.1 gradients swapped (ssn)        -> A and C
   (e) dx of a down block doubled (the 1/2 of the average-pool backward lost)    -> A
   (f) skip_connection.bias gradient left at zero                                -> B and D
   and, for E, a NaN that spreads from one sample's dx to every sample's."""
import math
import os

import numpy as np
import pytest
import torch

import resblock_reference as R
from oracle import unet as U
from param_gen import gen_param, normal

FWD = dict(rtol=1e-4, atol=1e-5)
GRAD = dict(rtol=1e-3, atol=1e-5)
PGRAD = dict(rtol=1e-3, atol=1e-4)

RES = {"plain": (32, 32, 0), "skip": (32, 64, 0), "wide_in": (96, 32, 0), "down": (32, 32, 1), "up": (64, 64, 2)}
RES_R6 = {"ssn_plain": (32, 32, 0), "ssn_skip": (32, 64, 0), "ssn_down": (32, 32, 1), "ssn_up": (64, 64, 2)}
GOLDEN = [("resblocks.npz", n, 0) for n in RES] + [("blocks_r6.npz", n, 1) for n in RES_R6]


def _golden_inputs(g, name, ci, co, updown, ssn):
    """the golden files' own inputs (B = 2, L = 32, a dense embedding) in the form resblock_reference.make_inputs returns"""
    sw, sx, se, sdy = [int(v) for v in g[name + ":seeds"]]
    shapes = R.param_shapes(ci, co, ssn)
    B, L = 2, 32
    return dict(B=B, cin=ci, cout=co, L=L, Lo=R.lout(L, updown), updown=updown, ssn=ssn,
                params={k: torch.from_numpy(gen_param(sw, k, s)) for k, s in shapes.items()},
                preload={k: torch.zeros(s) for k, s in shapes.items()},
                x=torch.from_numpy(normal((B, ci, L), seed=sx)), dy=torch.from_numpy(normal((B, co, R.lout(L, updown)), seed=sdy)),
                emb=torch.from_numpy(normal((B, R.EMB), seed=se)))


@pytest.mark.parametrize("fname,name,ssn", GOLDEN, ids=[n for _f, n, _s in GOLDEN])
def test_reference_pinned_to_goldens_and_float32_oracle(golden_dir, fname, name, ssn):
    g = np.load(os.path.join(golden_dir, fname), allow_pickle=False)
    ci, co, updown = (RES_R6 if ssn else RES)[name]
    inp = _golden_inputs(g, name, ci, co, updown, ssn)
    ref = R.reference(inp, "f32")
    np.testing.assert_allclose(ref["y"].numpy(), g[name + ":y"], **FWD)
    np.testing.assert_allclose(ref["dx"].numpy(), g[name + ":dx"], **GRAD)
    np.testing.assert_allclose(ref["demb"].numpy(), g[name + ":demb"], **GRAD)
    for k, v in ref["g"].items():
        np.testing.assert_allclose(v.numpy(), g[name + ":g:" + k], **PGRAD, err_msg=k)
    assert ref["dh1"].shape == (2, co, inp["Lo"]) and ref["dout"].shape == ref["y"].shape
    assert ref["ps"].shape == (2, 2 * co if ssn else co) and ref["abs_c"].shape == (co,)
    # the float32 yardstick = oracle.unet.resblock called directly in float32 on the same values, bit for bit
    o32 = R.run_oracle(inp, "f32", torch.float32)
    sd = {k: v.clone().requires_grad_(True) for k, v in inp["params"].items()}
    x = inp["x"].clone().requires_grad_(True); e = inp["emb"].clone().requires_grad_(True)
    y = U.resblock(sd, "", x, e, up=updown == 2, down=updown == 1, scale_shift=bool(ssn))
    y.backward(inp["dy"])
    assert torch.equal(o32["y"], y.detach().double()) and torch.equal(o32["dx"], x.grad.double()) and torch.equal(o32["demb"], e.grad.double())
    for k in sd:
        assert torch.equal(o32["g"][k], sd[k].grad.double()), k
    # and the float64 reference is closer to it than the SURVEY tolerances by orders of magnitude
    assert R.rel_l2(o32["y"], ref["y"]) < 1e-5 and R.rel_l2(o32["dx"], ref["dx"]) < 1e-5


def test_gap_constants_are_the_projects():
    import gpu_util as G
    assert (R.BF16_GAP_FACTOR, R.BF16_FLOOR, R.F16_FLOOR) == (G.BF16_GAP_FACTOR, G.BF16_FLOOR, G.F16_FLOOR)
    floor = {"bf16": G.BF16_FLOOR, "f16": G.F16_FLOOR}
    for fmt, gap in (("bf16", 3e-3), ("bf16", 1e-4), ("f16", 3e-4), ("f16", 1e-5)):
        assert max(R.BF16_GAP_FACTOR * gap, floor[fmt]) == G.bf16_gap_bound(gap, floor=floor[fmt])


def test_one_hot_embedding_reads_the_per_sample_sums():
    """the claim the GPU test rests on, on the float64 reference: ps = g_w[:, :B]^T / silu(1), columns >= B exactly 0, rows add up to the bias"""
    inp = R.make_inputs(8, 128, 256, 96, 0, 0)
    ref = R.reference(inp, "bf16")
    ps = R.per_sample_sums(ref["g"]["emb_layers.1.weight"], 8, silu1=float(torch.nn.functional.silu(torch.ones((), dtype=torch.float64))))
    assert float((ps - ref["ps"]).abs().max()) <= 1e-12 * float(ref["ps"].abs().max())
    assert float((ps.sum(0) - ref["g"]["emb_layers.1.bias"]).abs().max()) <= 1e-12 * float(ref["ps_mag"].max())
    assert float((ref["g"]["in_layers.2.bias"] - ref["g"]["emb_layers.1.bias"]).abs().max()) <= 1e-12 * float(ref["abs_c"].max())


# ---------------------------------------------------------------- the stand-in engine
def _flip_inputs(inp):
    """batch and channel order reversed (a use_scale_shift_norm projection within its [scale | shift] halves)"""
    co, ssn = inp["cout"], inp["ssn"]

    def fp(k, v):
        if k.startswith("emb_layers.1") and ssn:
            return v.reshape(2, co, *v.shape[1:]).flip(1).reshape(v.shape)
        if v.dim() == 3:
            return v.flip(0, 1)
        return v.flip(0)
    out = dict(inp)
    out["params"] = {k: fp(k, v).contiguous() for k, v in inp["params"].items()}
    out["x"], out["dy"], out["emb"] = inp["x"].flip(0, 1).contiguous(), inp["dy"].flip(0, 1).contiguous(), inp["emb"].flip(0).contiguous()
    out["_unflip_param"] = fp
    return out


def stand_in(inp, fmt):
    fl = _flip_inputs(inp)
    o = R.run_oracle(fl, fmt, torch.float32, storage=None if fmt == "f32" else R.storage_dtype(fmt))
    pre = inp["preload"]
    g = {k: fl["_unflip_param"](k, v) for k, v in o["g"].items()}
    raw = {k: (pre[k].float() + g[k].float()) for k in g}                     # the engine's fp32 `+=`
    return dict(y=o["y"].flip(0, 1), dx=o["dx"].flip(0, 1), demb=o["demb"].flip(0), raw={k: v.double() for k, v in raw.items()},
                g={k: (raw[k] - pre[k].float()).double() for k in raw})


STAND_IN_ROUTE = dict(b_c1=R.B_COLSUM)       # the oracle sums the stored dh1 for both biases
CASES = {"skip bf16": ((8, 128, 256, 96, 0, 0), "bf16"), "skip f16": ((8, 128, 256, 96, 0, 0), "f16"), "skip f32": ((3, 64, 128, 96, 0, 0), "f32"),
         "ssn bf16": ((8, 128, 128, 192, 0, 1), "bf16"), "ssn f32": ((8, 128, 128, 192, 0, 1), "f32"),
         "down bf16": ((8, 64, 64, 64, 1, 0), "bf16"), "down f32": ((8, 64, 64, 64, 1, 0), "f32"), "up bf16": ((8, 64, 64, 32, 2, 0), "bf16"),
         "down skip f32": ((8, 64, 128, 64, 1, 0), "f32"), "odd groups bf16": ((3, 96, 160, 40, 0, 0), "bf16"), "golden plain f32": ((2, 32, 32, 32, 0, 0), "f32")}
_CACHE = {}


def _case(name):
    """(inputs, float64 reference, yardsticks, the stand-in's outputs), computed once and never modified"""
    if name not in _CACHE:
        shape, fmt = CASES[name]
        inp = R.make_inputs(*shape)
        o32, oq = R.yardsticks(inp, fmt)
        _CACHE[name] = (inp, fmt, R.reference(inp, fmt), o32, oq, stand_in(inp, fmt))
    return _CACHE[name]


def _copy(got):
    return {k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v.clone()) for k, v in got.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_stand_in_engine_passes_every_check(name):
    inp, fmt, ref, o32, oq, got = _case(name)
    rep = R.run_checks(got, ref, o32, oq, inp, fmt, STAND_IN_ROUTE)
    print(R.report_line(name, fmt, "stand-in", rep))
    assert not rep["failed"]
    for k in "ABCD":
        assert rep[k] <= 1.0
    assert R.check_producers_agree(rep["ps"], R.per_sample_sums(_case(name)[4 if oq is not None else 3]["g"]["emb_layers.1.weight"], inp["B"]), ref, fmt) <= 1.0


def _set_grad(got, inp, k, new):
    """a fault in one parameter gradient: what the engine would have added, and the buffer contents that go with it"""
    got["g"][k] = new
    got["raw"][k] = inp["preload"][k].double() + new


def _fault(got, inp, which):
    co = inp["cout"]
    if which == "a":
        _set_grad(got, inp, "out_layers.3.bias", 2 * got["g"]["out_layers.3.bias"])
    elif which == "b":
        w = got["g"]["emb_layers.1.weight"].clone(); w[:, inp["B"] - 2] = 0
        _set_grad(got, inp, "emb_layers.1.weight", w)
    elif which == "c":
        v = got["g"]["in_layers.2.bias"].clone(); v[64:128] = 0
        _set_grad(got, inp, "in_layers.2.bias", v)
    elif which == "d":
        for k in ("emb_layers.1.weight", "emb_layers.1.bias"):
            v = got["g"][k]
            _set_grad(got, inp, k, torch.cat([v[co:], v[:co]], dim=0))
    elif which == "e":
        got["dx"] = 2 * got["dx"]
    elif which == "f":
        _set_grad(got, inp, "skip_connection.bias", torch.zeros_like(got["g"]["skip_connection.bias"]))
    return got


FAULTS = [("a", "skip bf16", "AB"), ("a", "skip f32", "AB"), ("b", "skip bf16", "C"), ("b", "skip f32", "C"), ("b", "skip f16", "C"),
          ("c", "skip bf16", "D"), ("c", "skip f32", "D"), ("d", "ssn bf16", "AC"), ("d", "ssn f32", "AC"),
          ("e", "down bf16", "A"), ("e", "down f32", "A"), ("f", "skip bf16", "BD"), ("f", "skip f32", "BD"), ("f", "down skip f32", "BD")]


@pytest.mark.parametrize("which,name,must_fail", FAULTS, ids=[f"{w} {n}" for w, n, _m in FAULTS])
def test_planted_fault_is_caught(which, name, must_fail):
    inp, fmt, ref, o32, oq, got = _case(name)
    rep = R.run_checks(_fault(_copy(got), inp, which), ref, o32, oq, inp, fmt, STAND_IN_ROUTE, collect=True)
    print(f"fault ({which}) on {name}: caught by {sorted(rep['failed'])}")
    for letter in must_fail:
        assert letter in rep["failed"], f"fault ({which}) on {name}: check {letter} did not fail; failed: {rep['failed']}"
        assert rep["failed"][letter].startswith(f"check {letter}")


def test_total_of_per_sample_sums_identity_bound():
    """D on the route 'total of the per-sample sums': a c1 bias that IS the fp32 total of the stand-in's sums passes the 2 gamma(B) bound;
    one that lost a sample does not"""
    inp, fmt, ref, o32, oq, got = _case("skip bf16")
    ps = R.per_sample_sums(got["g"]["emb_layers.1.weight"], inp["B"]).float()
    ok = _copy(got); _set_grad(ok, inp, "in_layers.2.bias", ps.sum(0).double()); _set_grad(ok, inp, "emb_layers.1.bias", ps.flip(0).sum(0).double())
    assert max(R.check_identities(ok, ref, inp, fmt, dict(b_c1=R.B_TOTAL)).values()) <= 1.0
    _set_grad(ok, inp, "in_layers.2.bias", ps[1:].sum(0).double())
    with pytest.raises(AssertionError, match="check D"):
        R.check_identities(ok, ref, inp, fmt, dict(b_c1=R.B_TOTAL))


@pytest.mark.parametrize("name", ["skip bf16", "skip f32"])
def test_nan_masks(name):
    """E: a NaN at dy[b0, c0, l0] reaches sample b0's dx and demb row and every bias gradient's... exactly the reference's elements"""
    inp0, fmt, *_ = _case(name)
    inp = dict(inp0); inp["dy"] = inp0["dy"].clone(); inp["dy"][1, 5, 7] = math.nan
    ref = R.run_oracle(inp, fmt, torch.float64)
    got = stand_in(inp, fmt)
    assert bool(torch.isnan(ref["dx"][1]).any()) and not bool(torch.isnan(ref["dx"][0]).any()) and not bool(torch.isnan(ref["demb"][0]).any())
    R.check_nan_masks(got, ref)
    bad = _copy(got); bad["dx"][0, 0, 0] = math.nan              # the NaN leaks into another sample
    with pytest.raises(AssertionError, match="check E"):
        R.check_nan_masks(bad, ref)
    bad = _copy(got); bad["raw"]["out_layers.3.bias"] = torch.zeros_like(bad["raw"]["out_layers.3.bias"])      # a NaN swallowed
    with pytest.raises(AssertionError, match="check E"):
        R.check_nan_masks(bad, ref)
