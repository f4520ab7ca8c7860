"""CPU: the staged attention checks of tests/numerics.py (attention_stages: every stage of softmax(alpha q k^T) v and its backward judged on
the stored operands the next stage read, the way the attention kernels of csrc/attn.hip and the GEMM + softmax composition expose them)
accept correct kernels and reject subtly wrong ones.

Correct kernels: two fp32 emulations of the whole forward + backward (fp32 accumulation in two different orders, every 16-bit store
rounded once, torch's exp) must pass every stage at the (T, C) at which the kernels change variant (SHAPES), both orders in both formats.  The emulation has
no path that depends on the batch size or on the number of query rows, so the batch is cut to 2 and, at T >= 768, to one sample of 192
query rows against all T keys (the row operations and the reductions over the keys keep their length) to keep the file under a minute.
Defect models: each must fail the stage named for it (DEFECTS).  For the record the test prints which of them the old assert_close
tolerances of test_gpu_primitives.py / test_gpu_fp16.py (bf16 3e-2 forward, 5e-2 backward; f16 4e-3 / 8e-3) would have accepted.

The row-maximum defect comes twice.  A maximum taken over one quarter of the keys and used for the WHOLE row is the same softmax
mathematically (any row constant cancels) until exp overflows, which needs s - m > 88: `max_one_quarter` runs at q, k scaled by 16
(logits of standard deviation ~256), where it does.  What a missing reduction across the column waves does at the sharp scale of the
device tests (4) is give every column wave its OWN quarter's maximum while the sum runs over all of them: `max_per_wave`.
The P defects are run with the CPU's exp accuracy and with the device figures of numerics.py, so that stage P is shown to stay sharp
with the constants the device tests use.  Non-finite operands: the emulation must reproduce the float64 pattern, a kernel that loses NaN
logits must not; fp16 subnormal probabilities flushed to zero must fail stage P."""
import math

import numpy as np
import pytest
import torch

import numerics as N

E_EXP = 4 * N.U32          # torch's CPU exp: at most 1 ulp = 2u (SLEEF's u10 routines), doubled as the device figures are


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def make_inputs(B, T, C, fmt, scale=1.0, seed=0):
    q = N.to_storage(_randn((B, T, C), 101 + seed, scale), fmt); k = N.to_storage(_randn((B, T, C), 102 + seed, scale), fmt)
    v = N.to_storage(_randn((B, T, C), 103 + seed), fmt); do = N.to_storage(_randn((B, T, C), 104 + seed), fmt)
    return q, k, v, do


def mm32(a, b, order):
    """a (B, M, K) @ b (B, K, N) with fp32 accumulation: torch's order, or 32-wide K chunks added last to first"""
    a, b = a.float(), b.float()
    if order == 0:
        return a @ b
    acc = None
    for k0 in reversed(range(0, a.shape[-1], 32)):
        part = a[..., k0:k0 + 32] @ b[:, k0:k0 + 32]
        acc = part if acc is None else acc + part
    return acc


def _quarters(x, order):
    """row sums as the column waves form them: one partial per quarter of the keys, then added"""
    parts = [c.sum(-1, keepdim=True) for c in x.chunk(4, dim=-1)]
    if order:
        parts = parts[::-1]
    return parts


def emulate(q, k, v, do, fmt, order=0, defect=None):
    """the kernels' arithmetic in fp32 on the CPU; every stored 16-bit tensor rounded ONCE; returns the buffers a caller could read back"""
    B, T, C = q.shape
    al = np.float32(1.0) / np.sqrt(np.float32(C))
    rnd = (lambda t: N.rne(t.double(), fmt)) if fmt != "f32" else (lambda t: t.double())
    s = mm32(q, k.transpose(1, 2), order) * float(al)
    if defect == "nan_masked":                                 # NaN logits lost (an fmaxf-style clamp somewhere before the exponential)
        s = torch.where(torch.isnan(s), torch.zeros_like(s), s)
    m = s.amax(-1, keepdim=True)
    if defect == "max_one_quarter":
        m = s[..., :T // 4].amax(-1, keepdim=True)
    if defect == "max_per_wave":
        m = torch.cat([c.amax(-1, keepdim=True).expand_as(c) for c in s.chunk(4, dim=-1)], dim=-1)
    e = torch.exp(s - m)
    parts = _quarters(e, order)
    S = sum(parts[1:], parts[0]) if order else e.sum(-1, keepdim=True)
    if defect == "norm_per_wave":
        S = torch.cat([c.sum(-1, keepdim=True).expand_as(c) for c in e.chunk(4, dim=-1)], dim=-1)
    p32 = e * (1.0 / S)
    P = N.rtz(p32.double(), fmt) if defect == "p_trunc" else rnd(p32)
    if defect == "p_f16_flush":
        P = torch.where(P.abs() < 2.0 ** -14, torch.zeros_like(P), P)
    if defect == "xcd_perm":                                   # the second query tile of every sample computed from another sample
        P[:, 64:128] = P.roll(1, 0)[:, 64:128].clone()
    Pd = P.clone()
    if defect == "drop_slice":
        Pd[:, 0:32, 32:64] = 0
    if defect == "stale_slice":                                # T = 768: column wave 1 owns keys 96 .. 191 = slices 3, 4, 5
        Pd[:, :, 128:160] = P[:, :, 96:128]
    o32 = mm32(Pd, v, order)
    if defect == "v_tile_reuse":
        o32[..., 256:] = mm32(Pd, v[..., :256], order)
    if defect == "partial16":
        h = T // 2
        o32 = rnd(mm32(P[:, :, :h], v[:, :h], order)).float() + rnd(mm32(P[:, :, h:], v[:, h:], order)).float()
    O = rnd(o32)
    dP = mm32(do, v.transpose(1, 2), order)
    pf = P.float()
    parts = _quarters(dP * pf, order)
    dl = parts[0] if defect == "dot_one_wave" else sum(parts[1:], parts[0])
    a_ds = {"alpha_missing": 1.0, "alpha_twice": float(al * al)}.get(defect, float(al))
    dS = rnd(a_ds * pf * (dP - dl))
    dQ = rnd(mm32(dS, k, order))
    dK = rnd(mm32(dS if defect == "dk_untransposed" else dS.transpose(1, 2), q, order))
    dV = rnd(mm32((dS if defect == "dv_from_ds" else P).transpose(1, 2), do, order))
    return dict(S=s.double(), P=P, O=O, dP=dP.double(), dS=dS, dQ=dQ, dK=dK, dV=dV)


# (T, C): fused 64-row blocks T = 64 .. 256, two 256-column passes (C = 512), the long variant T = 768; composition with the K = 1 .. 4 register
# softmax (T <= 256, 384, 768, 1024) and the three-pass softmax (T = 1280)
SHAPES = [(64, 256), (128, 256), (256, 256), (192, 512), (192, 256), (768, 256), (768, 512), (24, 32), (72, 64), (384, 128), (1024, 32), (1280, 32)]


@pytest.mark.parametrize("T,C", SHAPES)
def test_correct_emulations_pass_every_stage(T, C):
    B = 1 if T >= 768 else 2
    for fmt in ("bf16", "f16"):
        q, k, v, do = make_inputs(B, T, C, fmt)
        if T >= 768:
            q, do = q[:, :192], do[:, :192]
        shared = {}
        for order in (0, 1):
            fails, stats = N.attention_stages(q, k, v, do, emulate(q, k, v, do, fmt, order), fmt, E_EXP, route=f"emulation {order} ({B},{T},{C})",
                                              shared=shared)
            assert not fails, fails
            assert set(stats) == {"S", "P", "O", "dP", "dS", "dQ", "dK", "dV"}


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_correct_emulations_pass_sharp_softmax(fmt):
    """q, k scaled by 4: logits of standard deviation ~16, s - m down to about -90: the stability the maximum subtraction exists for"""
    q, k, v, do = make_inputs(2, 192, 256, fmt, scale=4.0)
    sl = N.attn_logits(q, k, N.attn_alpha(256))
    p = N.attn_softmax(sl)
    assert float((sl - sl.amax(-1, keepdim=True)).min()) < -85, "s - m does not reach the range the maximum subtraction exists for"
    assert float((p.amax(-1) > 0.99).double().mean()) > 0.05
    p16 = N.rne(p, "f16")
    assert bool(((p16.abs() < 2.0 ** -14).double().mean(-1) > 0.5).any()), "no row with more than half of RNE(p) zero or subnormal in fp16"
    shared = {}
    for order in (0, 1):
        fails, _ = N.attention_stages(q, k, v, do, emulate(q, k, v, do, fmt, order), fmt, E_EXP, route=f"emulation {order} sharp", shared=shared)
        assert not fails, fails


# defect, the stage that must reject it, (B, T, C), q / k scale, formats, e_exp values
CPU_AND_DEVICE = (E_EXP, N.E_EXP_FUSED, N.E_EXP_COMPOSITION)
DEFECTS = [
    ("p_trunc", "P", (2, 192, 256), 1.0, ("bf16", "f16"), CPU_AND_DEVICE),
    ("max_per_wave", "P", (2, 192, 256), 4.0, ("bf16", "f16"), CPU_AND_DEVICE),
    ("max_one_quarter", "P", (2, 192, 256), 16.0, ("bf16", "f16"), CPU_AND_DEVICE),
    ("norm_per_wave", "P", (2, 192, 256), 1.0, ("bf16", "f16"), CPU_AND_DEVICE),
    ("p_f16_flush", "P", (2, 192, 256), 4.0, ("f16",), CPU_AND_DEVICE),
    ("drop_slice", "O", (2, 192, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("stale_slice", "O", (1, 768, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("v_tile_reuse", "O", (2, 192, 512), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("dot_one_wave", "dS", (2, 192, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("alpha_missing", "dS", (2, 192, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("alpha_twice", "dS", (2, 192, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("dk_untransposed", "dK", (2, 192, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("dv_from_ds", "dV", (2, 192, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("xcd_perm", "P", (2, 192, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
    ("partial16", "O", (2, 192, 256), 1.0, ("bf16", "f16"), (E_EXP,)),
]
OLD_TOL = {"bf16": (3e-2, 5e-2), "f16": (4e-3, 8e-3)}


def _old_accepts(got, want, tol):
    return bool(((got - want).abs() <= tol + tol * want.abs()).all())


@pytest.mark.parametrize("defect,stage,shape,scale,fmts,e_exps", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_defect_is_rejected_by_its_stage(defect, stage, shape, scale, fmts, e_exps):
    B, T, C = shape
    for fmt in fmts:
        q, k, v, do = make_inputs(B, T, C, fmt, scale=scale)
        got = emulate(q, k, v, do, fmt, 0, defect)
        for e_exp in e_exps:
            fails, _ = N.attention_stages(q, k, v, do, got, fmt, e_exp, route=f"{defect} {fmt}", report=False)
            assert stage in fails, f"{defect} [{fmt}, e_exp {e_exp:.2e}]: stage {stage} accepted it (failed stages: {sorted(fails)})"
            # the stages up-stream of the defect see a correct kernel and must not complain
            order = ["S", "P", "O", "dP", "dS", "dQ", "dK", "dV"]
            early = [s for s in order[:order.index(stage)] if s in fails]
            assert not early, f"{defect} [{fmt}]: up-stream stages {early} failed too: {fails}"
        # for the record: the old whole-tensor tolerances on the end-to-end result
        a = N.attn_alpha(C)
        p = N.attn_softmax(N.attn_logits(q, k, a)); dp = N.attn_dprobs(do, v); ds = N.attn_dscores(p, dp, a)
        f, b = OLD_TOL[fmt]
        acc = {"out": _old_accepts(got["O"], N.attn_out(p, v), f), "dq": _old_accepts(got["dQ"], N.attn_dq(ds, k), b),
               "dk": _old_accepts(got["dK"], N.attn_dk(ds, q), b), "dv": _old_accepts(got["dV"], N.attn_dv(p, do), b)}
        verdict = "ACCEPTED by the old assert_close tolerances" if all(acc.values()) else "rejected by the old tolerances on " + ", ".join(
            k_ for k_, ok in acc.items() if not ok)
        print(f"[defect] {defect:<16s} {fmt:>4s}: rejected by stage {stage} ({fails[stage][:110]}...); {verdict}")


def _poisoned(fmt):
    q, k, v, do = (t.clone() for t in make_inputs(3, 128, 256, fmt))
    q[0, 5, 7] = math.nan; k[1, 125, 255] = math.inf; v[2, 9, 100] = math.nan
    do[0, 127, 3] = math.nan; do[1, 17, 128] = -math.inf
    return q, k, v, do


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_nonfinite_pattern_stage(fmt):
    """one NaN in a q row, one inf in a k row, one NaN in v, one NaN and one -inf in dO: both emulations reproduce the float64 pattern in
    every stage (0 x inf = NaN in dS included); a kernel that loses NaN logits is rejected at P"""
    q, k, v, do = _poisoned(fmt)
    for order in (0, 1):
        got = emulate(q, k, v, do, fmt, order)
        fails = N.attention_nonfinite(q, k, v, do, {s: got[s] for s in ("P", "O", "dS", "dQ", "dK", "dV")}, route=f"emulation {order} {fmt}")
        assert not fails, fails
    assert "P" in N.attention_nonfinite(q, k, v, do, emulate(q, k, v, do, fmt, 0, "nan_masked"), route="nan_masked", report=False)
    with pytest.raises(AssertionError, match="no non-finite element"):
        clean = make_inputs(3, 128, 256, fmt)
        N.attention_nonfinite(*clean, emulate(*clean, fmt, 0), report=False)
