"""-m gpu: the attention kernels, variant by variant, against staged float64 references (tests/numerics.py: attention_stages).

Both the fused chain kernel (csrc/attn.hip) and the GEMM + softmax composition (ops.hip, elementwise.hip) store their 16-bit intermediates
in caller-owned buffers (P in `probs`, dS in `scratch_dlogits`; the composition also its fp32 logits and dP in the fp32 scratch), and the
later stages read those very values.  So every stage is judged on the operands the next stage read:
  S  = alpha q k^T           check A, n = C                         (composition only: the fp32 logits are visible)
  P  = softmax(S)            numerics.softmax_bound (derived), check B
  O  = P_stored V            check A, n = T, check B
  dP = dO V^T                check A, n = C                         (composition only)
  dS = alpha P (dP - dl)     numerics.dscores_bound (derived), check B
  dQ = dS_stored K, dK = dS_stored^T Q, dV = P_stored^T dO           check A, n = T, check B (fused pass or batched TN GEMM alike)
Each case names the variant that must serve it, forces it with the library's switches, and confirms it: the launch profiler counts the
GEMM launches of each pass (fused forward 0, composition 2; fused backward 0 with dK and dV fused, 1 with dK fused, 2 on 64-row blocks,
composition 4) and, for the fused variants, EEGLDM_ATTN_STAMPS=1 makes the launcher print its instantiation (T, mode, NQ, NCW) on stderr.
Output buffers are pre-filled with NaN; the column-view cases also demand that every column outside the view keeps its bits.

exp accuracy (the one figure of softmax_bound that is not derived from this repository's source): `__expf` in attn.hip compiles to
v_mul_f32 by fp32(log2 e) followed by v_exp_f32 (read from the gfx950 assembly), expf in elementwise.hip to the device library's routine.
numerics.py derives both figures from the stated accuracy of the instruction and of the library routine (E_EXP_FUSED, E_EXP_COMPOSITION).

Every stage prints one `[numerics]` line (worst error in units of its bound, mismatch share against the fp32 CPU emulation, mean signed
ulp error), every case a `[route]` line and a report-only `[numerics] end to end` line: rel-L2 of O and dqkv against
oracle.unet.qkv_attention on float64 operands, beside the same figure for a float64 computation that rounds P, O, dS and the gradients to
the storage type once each (what the storage format alone costs)."""
import csv
import math
import os
import re
import sys
import tempfile

import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

FMT = {0: "f32", 1: "bf16", 2: "f16"}
E_EXP = {"fused": N.E_EXP_FUSED, "composition": N.E_EXP_COMPOSITION}


def _G():
    import gpu_util as G
    return G


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _half_cus():
    return (torch.cuda.get_device_properties(0).multi_processor_count + 1) // 2


def _batch(B):
    """symbolic batch sizes around the whole-sample threshold B >= num_cu / 2 (attn.hip launch_chain)"""
    return {"half": _half_cus(), "half+2": _half_cus() + 2}.get(B, B)


def _prof_rows(G, c):
    path = os.path.join(tempfile.gettempdir(), f"eegldm_attn_rows_{os.getpid()}.csv")
    G.check(G.lib.eegldm_prof_dump(c.h, path.encode()))
    try:
        with open(path) as fh:
            return list(csv.DictReader(fh))
    finally:
        os.unlink(path)


_INPUTS = {}


def _inputs(B, T, C, fmt, scale):
    """seeded float64 normals rounded to storage (q and k scaled by `scale`); kept for the other tests of the same case"""
    key = (B, T, C, fmt, scale)
    if key not in _INPUTS:
        if len(_INPUTS) > 2:
            _INPUTS.clear()
        _INPUTS[key] = [N.to_storage(_randn((B, T, C), 201 + i, sc), fmt) for i, sc in enumerate((scale, scale, 1.0, 1.0))]
    return _INPUTS[key]


def _judged_samples(B, T):
    """Every sample runs, and every output element of every sample must have been written with a finite value (NaN pre-fill); the staged
    float64 checks run on at most ~6e5 score elements per case so that a case stays within seconds: evenly spaced samples, always the
    first and the last; every other sample is held to check A of O and dQ from its own stored P / dS (_check_other_samples), which a sample
    served by another sample's block cannot meet"""
    n = max(2, min(B, 600_000 // (T * T)))
    return sorted({round(i * (B - 1) / (n - 1)) for i in range(n)}) if B > 1 else [0]


def _check_other_samples(name, fmt, rest, k, v, got):
    """the samples outside _judged_samples: check A of O = P_stored V and dQ = dS_stored K on every 8th channel (two float64 products, no
    row-operation bounds): a sample served by another sample's block, or by another sample's K / V, fails on every channel"""
    if not rest:
        return
    T = k.shape[1]
    for stage, fn, a, b in (("O", N.attn_out, got["P"][rest], v[rest][..., ::8]), ("dQ", N.attn_dq, got["dS"][rest], k[rest][..., ::8])):
        ref, mag, _ = N.evaluate(fn, a, b)
        nbad, worst, i = N.check_a(got[stage][rest][..., ::8], ref, mag, T, fmt)
        assert nbad == 0, f"{name} [{fmt}]: {stage} of the samples outside the judged set: {nbad} elements outside check A (worst {worst:.3g} x bound at {i})"
    print(f"[numerics] {name} [{fmt}]: {len(rest)} further samples: O and dQ within check A on every 8th channel")


def _launch(G, c, q, k, v, do, dt, view, capfd, stamps):
    """forward + backward through the C ABI on NaN-filled buffers; returns the read-back stages, the GEMM launch counts and the stamp lines"""
    B, T, C = q.shape
    td = G.TDT[dt]
    heads, h = view if view else (1, 0)
    Ct = heads * C
    ldq, ldo, off3, off1 = 3 * Ct, Ct, 3 * h * C, h * C
    qkv = _randn((B * T, ldq), 299).to(td) if view else torch.empty(B * T, ldq, dtype=td)
    qkv[:, off3:off3 + 3 * C] = torch.cat([q, k, v], dim=-1).reshape(B * T, 3 * C).to(td)
    dof = torch.zeros(B * T, ldo, dtype=td); dof[:, off1:off1 + C] = do.reshape(B * T, C).to(td)
    qd, dod = qkv.to(G.DEV), dof.to(G.DEV)
    nan = float("nan")
    od = torch.full((B * T, ldo), nan, device=G.DEV, dtype=td); pr = torch.full((B, T, T), nan, device=G.DEV, dtype=td)
    s1 = torch.full((B, T, T), nan, device=G.DEV); s2 = torch.full((B, T, T), nan, device=G.DEV, dtype=td)
    dq = torch.full((B * T, ldq), nan, device=G.DEV, dtype=td)
    es = qd.element_size()
    at = lambda t, o: G.ptr(t) if o == 0 else type(G.ptr(t))(t.data_ptr() + o * es)
    capfd.readouterr()
    got = {}
    try:
        c.prof_enable(True)
        G.check(G.lib.eegldm_attention_fwd(c.h, at(qd, off3), ldq, at(od, off1), ldo, G.ptr(pr), G.ptr(s1), B, T, C, dt))
        torch.cuda.synchronize()
        nf = len(_prof_rows(G, c))
        if nf:
            got["S"] = s1.double().cpu()
        c.prof_enable(True)
        G.check(G.lib.eegldm_attention_bwd(c.h, at(qd, off3), ldq, G.ptr(pr), at(dod, off1), ldo, at(dq, off3), ldq, G.ptr(s1), G.ptr(s2), B, T, C, dt))
        torch.cuda.synchronize()
        nb = len(_prof_rows(G, c))
        if nb == 4:
            got["dP"] = s1.double().cpu()
    finally:
        c.prof_enable(False)
    cap = capfd.readouterr()
    sys.stdout.write(cap.out)
    lines = re.findall(r"attn_chain<T=(\d+), mode (\d), NQ (\d+), NCW (\d+)>", cap.err) if stamps else []
    o_all, dq_all = od.cpu(), dq.cpu()
    got.update(P=pr.double().cpu(), dS=s2.double().cpu(), O=o_all[:, off1:off1 + C].double().reshape(B, T, C),
               dQ=dq_all[:, off3:off3 + C].double().reshape(B, T, C), dK=dq_all[:, off3 + C:off3 + 2 * C].double().reshape(B, T, C),
               dV=dq_all[:, off3 + 2 * C:off3 + 3 * C].double().reshape(B, T, C))
    if view:        # nothing outside the view may be written: those columns still hold the NaN they were filled with, bit for bit
        fill = torch.full((1,), nan, dtype=td).view(torch.int16)
        mo = torch.ones(ldo, dtype=torch.bool); mo[off1:off1 + C] = False
        mq = torch.ones(ldq, dtype=torch.bool); mq[off3:off3 + 3 * C] = False
        assert bool((o_all.view(torch.int16)[:, mo] == fill).all()), "out: columns outside the view were written"
        assert bool((dq_all.view(torch.int16)[:, mq] == fill).all()), "dqkv: columns outside the view were written"
    return got, nf, nb, [tuple(int(x) for x in ln) for ln in lines]


def _confirm(name, fmt, want, nf, nb, lines, T):
    """want: ("composition",) or ("fused", NQ, NCW, backward GEMM launches)"""
    if want[0] == "composition":
        assert (nf, nb) == (2, 4), f"{name} [{fmt}]: expected the composition (2 + 4 GEMM launches), profiler saw {nf} + {nb}"
        assert not lines, f"{name} [{fmt}]: composition expected, but the fused kernel ran: {lines}"
        print(f"[route] {name} [{fmt}]: composition, GEMM launches fwd {nf} bwd {nb}")
        return "composition"
    _, nq, ncw, nbw = want
    assert (nf, nb) == (0, nbw), f"{name} [{fmt}]: expected fused (0 forward, {nbw} backward GEMM launches), profiler saw {nf} + {nb}"
    assert sorted(lines) == [(T, 0, nq, ncw), (T, 1, nq, ncw)], f"{name} [{fmt}]: expected attn_chain<T={T}, NQ {nq}, NCW {ncw}> forward and backward, saw {lines}"
    print(f"[route] {name} [{fmt}]: fused attn_chain<T={T}, NQ {nq}, NCW {ncw}>, GEMM launches fwd {nf} bwd {nb}")
    return "fused"


def _end_to_end(q, k, v, do, got, fmt, name):
    from oracle.unet import qkv_attention
    B, T, C = q.shape
    qkv = torch.cat([q, k, v], dim=-1).permute(0, 2, 1).contiguous().requires_grad_(True)
    o = qkv_attention(qkv)
    (g,) = torch.autograd.grad(o, qkv, do.permute(0, 2, 1))
    o = o.detach().permute(0, 2, 1); g = g.permute(0, 2, 1)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    a = N.attn_alpha(C)
    r = (lambda t: N.rne(t, fmt)) if fmt != "f32" else (lambda t: t)
    P = r(N.attn_softmax(N.attn_logits(q, k, a))); dS = r(N.attn_dscores(P, N.attn_dprobs(do, v), a))
    eo = r(N.attn_out(P, v)); eg = torch.cat([r(N.attn_dq(dS, k)), r(N.attn_dk(dS, q)), r(N.attn_dv(P, do))], dim=-1)
    gg = torch.cat([got["dQ"], got["dK"], got["dV"]], dim=-1)
    print(f"[numerics] end to end {name} [{fmt}] vs oracle.unet.qkv_attention: O rel-L2 {rel(got['O'], o):.3e} (storage emulation {rel(eo, o):.3e}), "
          f"dqkv rel-L2 {rel(gg, g):.3e} (storage emulation {rel(eg, g):.3e})")


def _case(name, B, T, C, dts, env, want, env_switches, capfd, view=None, scale=1.0):
    G = _G(); c = G.ctx()
    B = _batch(B)
    fused = want[0] == "fused"
    env_switches(EEGLDM_ATTN_STAMPS="1" if fused else None, **env)
    worst = {}
    for dt in dts:
        fmt = FMT[dt]
        q, k, v, do = _inputs(B, T, C, fmt, scale)
        got, nf, nb, lines = _launch(G, c, q, k, v, do, dt, view, capfd, fused)
        path = _confirm(name, fmt, want, nf, nb, lines, T)
        for s, t in got.items():
            assert bool(torch.isfinite(t).all()), f"{name} [{fmt}]: {s} holds non-finite values (an element that was not written, or a kernel fault)"
        sel = _judged_samples(B, T)
        _check_other_samples(name, fmt, [b for b in range(B) if b not in sel], k, v, got)
        q, k, v, do = (t[sel] for t in (q, k, v, do)); got = {s: t[sel] for s, t in got.items()}
        fails, stats = N.attention_stages(q, k, v, do, got, fmt, E_EXP[path], route=name)
        _end_to_end(q, k, v, do, got, fmt, name)
        assert not fails, f"{name} [{fmt}]: " + " | ".join(f"{s}: {m}" for s, m in fails.items())
        for s, st in stats.items():
            worst[s] = max(worst.get(s, 0.0), st["worst"])
    print(f"[numerics] {name}: worst error in units of the bound per stage: " + ", ".join(f"{s} {w:.3f}" for s, w in worst.items()))


B64 = ("fused", 1, 4, 2)         # 64-row blocks: dK, dV by batched TN GEMMs
LONG = ("fused", 1, 8, 2)        # T = 768: 8 column waves
COMP = ("composition",)
# name, B, T, C, dtypes, switches, expected route
CASES = [
    ("64-row blocks (2, 64, 256)", 2, 64, 256, (1, 2), {}, B64),
    ("64-row blocks (3, 128, 256)", 3, 128, 256, (1, 2), {}, B64),
    ("64-row blocks XCD order (8, 128, 256)", 8, 128, 256, (1, 2), {}, B64),
    ("64-row blocks (2, 256, 256)", 2, 256, 256, (1, 2), {}, B64),
    ("64-row blocks XCD order (8, 256, 256)", 8, 256, 256, (1, 2), {}, B64),
    ("64-row blocks two column passes (3, 192, 512)", 3, 192, 512, (1, 2), {}, B64),
    ("64-row blocks XCD order two column passes (8, 192, 512)", 8, 192, 512, (1, 2), {}, B64),
    ("64-row blocks (2, 192, 256)", 2, 192, 256, (1, 2), {}, B64),
    ("whole-sample (half+2, 192, 256) dK dV fused", "half+2", 192, 256, (1, 2), {}, ("fused", 3, 4, 0)),
    ("whole-sample (half, 192, 512) dK dV fused", "half", 192, 512, (1, 2), {}, ("fused", 3, 4, 0)),
    ("whole-sample (half+2, 192, 256) NO_FUSED_DV", "half+2", 192, 256, (1, 2), {"EEGLDM_ATTN_NO_FUSED_DV": "1"}, ("fused", 3, 4, 1)),
    ("whole-sample (half+2, 192, 256) NO_FUSED_KV", "half+2", 192, 256, (1, 2), {"EEGLDM_ATTN_NO_FUSED_KV": "1"}, ("fused", 3, 4, 2)),
    ("(half+2, 192, 256) NO_WHOLE: 64-row blocks", "half+2", 192, 256, (1, 2), {"EEGLDM_ATTN_NO_WHOLE": "1"}, B64),
    ("long (2, 768, 256)", 2, 768, 256, (1, 2), {}, LONG),
    ("long XCD order (8, 768, 256)", 8, 768, 256, (1, 2), {}, LONG),
    ("long two column passes (2, 768, 512)", 2, 768, 512, (1, 2), {}, LONG),
    ("(2, 768, 256) NO_LONG: composition, K = 3 register softmax", 2, 768, 256, (1, 2), {"EEGLDM_ATTN_NO_LONG": "1"}, COMP),
    ("composition (2, 24, 32)", 2, 24, 32, (0, 1, 2), {}, COMP),
    ("composition (2, 72, 64)", 2, 72, 64, (0, 1, 2), {}, COMP),
    ("composition (2, 384, 128) K = 2 register softmax", 2, 384, 128, (0, 1, 2), {}, COMP),
    ("composition (1, 1024, 32) K = 4 register softmax", 1, 1024, 32, (0, 1), {}, COMP),
    ("composition (1, 1280, 32) three-pass softmax", 1, 1280, 32, (0, 1), {}, COMP),
    ("composition forced (2, 192, 256)", 2, 192, 256, (1, 2), {"EEGLDM_NO_FUSED_ATTENTION": "1"}, COMP),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_attention_variant(case, env_switches, capfd):
    name, B, T, C, dts, env, want = case
    _case(name, B, T, C, dts, env, want, env_switches, capfd)


@pytest.mark.parametrize("T", [192, 768])
@pytest.mark.parametrize("head", [0, 1])
def test_attention_column_views(T, head, env_switches, capfd):
    """two heads of 256 channels in C_total = 512: pointer offsets 3 h ch (qkv, dqkv) and h ch (out, dO), ldq = lddq = 1536, ldo = 512"""
    _case(f"column view head {head} of 2 (2, {T}, 256 in 512)", 2, T, 256, (1, 2), {}, B64 if T == 192 else LONG, env_switches, capfd, view=(2, head))


# one case per fused kernel shape: NJT = 1, 2, 3, 4, the long variant with one and two column passes, whole-sample blocks
FAMILY = [c for c in CASES if c[0] in ("64-row blocks (2, 64, 256)", "64-row blocks (3, 128, 256)", "64-row blocks (2, 192, 256)", "64-row blocks (2, 256, 256)",
                                       "long (2, 768, 256)", "long two column passes (2, 768, 512)", "whole-sample (half+2, 192, 256) dK dV fused")]


@pytest.mark.parametrize("case", FAMILY, ids=[c[0] for c in FAMILY])
def test_sharp_softmax(case, env_switches, capfd):
    """q and k scaled by 4: logits of standard deviation ~16, s - m down to about -90.  The reference must reach that range (rows whose largest
    p exceeds 0.99; rows where more than half of RNE(p) are zero or subnormal in fp16), then every stage must hold, and every fp16 P whose RNE(ref) is subnormal must equal
    RNE(ref) (numerics._check_row_op: except where ref is within the derived bound of a rounding midpoint)."""
    name, B, T, C, dts, env, want = case
    Bn = _batch(B)
    q, k = (t[_judged_samples(Bn, T)] for t in _inputs(Bn, T, C, "f16", 4.0)[:2])
    s = N.attn_logits(q, k, N.attn_alpha(C))
    p = N.attn_softmax(s)
    p16 = N.rne(p, "f16")
    assert float((s - s.amax(-1, keepdim=True)).min()) < -80, "the logits do not reach s - m < -80"
    assert bool((p.amax(-1) > 0.99).any()), "no row with a probability above 0.99"
    assert bool(((p16.abs() < 2.0 ** -14).double().mean(-1) > 0.5).any()), "no row with more than half of its fp16 probabilities zero or subnormal"
    _case(name + " [sharp softmax]", B, T, C, dts, env, want, env_switches, capfd, scale=4.0)


@pytest.mark.parametrize("case", FAMILY, ids=[c[0] for c in FAMILY])
def test_nonfinite_operands_through_the_fused_kernel(case, env_switches, capfd):
    """one NaN in a q row (sample 0), one inf in a k row (sample 1), one NaN in v (last sample), one NaN and one -inf in dO: the non-finite
    pattern of P, O, dS, dQ, dK and dV must be the float64 reference's"""
    name, B, T, C, dts, env, want = case
    G = _G(); c = G.ctx()
    B = _batch(B)
    env_switches(EEGLDM_ATTN_STAMPS="1", **env)
    for dt in dts:
        fmt = FMT[dt]
        q, k, v, do = (t.clone() for t in _inputs(B, T, C, fmt, 1.0))
        q[0, 5, 7] = math.nan; k[1, T - 3, C - 1] = math.inf; v[B - 1, 9, 100] = math.nan
        do[0, T - 1, 3] = math.nan; do[1, 17, C // 2] = -math.inf
        got, nf, nb, lines = _launch(G, c, q, k, v, do, dt, None, capfd, True)
        _confirm(name + " [non-finite]", fmt, want, nf, nb, lines, T)
        fails = N.attention_nonfinite(q, k, v, do, got, route=f"{name} [{fmt}]")
        assert not fails, " | ".join(fails.values())
