"""CPU: the arithmetic of the BatchNorm + LeakyReLU kernels (csrc/losses.hip), of the from-parts fold and of the fused tail's forward
(csrc/disc_tail.hip) restated in numpy float32 / float64, held to the very checks of tests/test_gpu_batchnorm_rounding.py on the very inputs
of its cases (same seeds), so that without a GPU it is known that
  - the derived bounds admit the intended arithmetic at channel means of 0, 30 and 100 sigma,
  - the mask-uncertain share of every GPU case is within its cap (computed from the reference alone), and
  - the checks reject each of a list of planted defects.

The models
  4-wide route   a block owns rows_per_block rows; thread (tx, ty) the 4 channels of column tx and the rows ty, ty + TY, ... of the block
                 (bnmap / bn_split): fp32 s1 += t, s2 = fma(a, b, s2) in row order, fp64 across the TY lanes, ONE fp32 rounding of the block
                 partial, fp64 over the blocks.  Apply: sc = gamma rstd, sh = fma(-mean, sc, beta), z = fma(x, sc, sh), mask z > 0.
  scalar route   4 row lanes per block of the row split, their fp32 sums added in fp32, fp64 over the splits.  Apply:
                 z = fma((x - mean) rstd, gamma, beta); backward mask  fma(gamma, xhat, beta) <= 0  (the other spelling).
  statistics     `fp32`: the sums of x and x^2 by the mapping above -- the forward statistics as they were; inside every hard bound, but
                 outside check B for fp16 at 30 and 100 sigma (test_fp32_statistics_sums_fail_check_b_at_30_sigma pins the figures the device gave).
                 `fp64` (the kernels now): fp64 per thread and across lanes, the block partial as two fp32 rows: exact sums up to 2^-48.
  backward       the reduce kernels keep the fp32 mapping (sums of dz and dz xhat: no common offset to amplify) and use the second mask
                 spelling with xhat = (x - mean) rstd on either route; the 4-wide apply the first.
  finalize       mean = S1 / n, var = max(S2 / n - mean^2, 0) in fp64, two casts; the running update in fp32.
(fma where the compiler contracts a * b + c; either choice is inside the bounds, which count a rounding for the product.)"""
import math

import numpy as np
import pytest
import torch

import numerics as N
import test_gpu_batchnorm_rounding as GB

f32 = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _lane_sums(t1, a, b, rows, rpb, TY, drop_last=False):
    """per (block, lane, channel) fp32 sums s1 += t1[row], s2 = fma(a[row], b[row], s2) over the lane's rows in order"""
    nb = -(-rows // rpb)
    l0 = np.arange(nb) * rpb
    l1 = np.minimum(rows - (1 if drop_last else 0), l0 + rpb)
    C = t1.shape[1]
    s1 = np.zeros((nb, TY, C), f32); s2 = np.zeros_like(s1)
    for k in range(-(-rpb // TY)):
        l = l0[:, None] + np.arange(TY)[None, :] + k * TY
        live = (l < l1[:, None])[:, :, None]
        lc = np.minimum(l, rows - 1)
        s1 = np.where(live, (s1 + t1[lc]).astype(f32), s1)
        s2 = np.where(live, _fma(a[lc], b[lc], s2), s2)
    return s1, s2


def _column_sums(t1, a, b, rows, route, defect=None, wide=False):
    """(S1, S2) float64 per channel as the statistics / reduce launch and its fold leave them"""
    drop = defect == "last row dropped"
    if wide:
        n = rows - (1 if drop else 0)
        return t1[:n].astype(np.float64).sum(0), (a[:n].astype(np.float64) * b[:n].astype(np.float64)).sum(0)
    if route["stats"] in (GB.VEC_FF, GB.VEC_FOLD):
        s1, s2 = _lane_sums(t1, a, b, rows, route["rpb"], route["ty"], drop)
        p1 = s1.astype(np.float64).sum(1).astype(f32); p2 = s2.astype(np.float64).sum(1).astype(f32)      # the block partial, rounded to fp32
    else:
        s1, s2 = _lane_sums(t1, a, b, rows, route["rpb"], 4, drop)
        add4 = lambda s: (((s[:, 0] + s[:, 1]).astype(f32) + s[:, 2]).astype(f32) + s[:, 3]).astype(f32)
        p1, p2 = add4(s1), add4(s2)
    return p1.astype(np.float64).sum(0), p2.astype(np.float64).sum(0)


def _finalize(S1, S2, n, rm, rv, nbt, defect=None):
    mean = S1 / n
    var = np.maximum(S2 / n - mean * mean, 0.0)
    st = np.stack([mean.astype(f32), (1.0 / np.sqrt(var + np.float64(f32(GB.EPS)))).astype(f32)], 1)
    ub = (var * n / (n if defect == "biased variance in the running update" else max(n - 1, 1))).astype(f32)
    mom = f32(0.1)
    rm2 = ((f32(1) - mom) * rm + mom * mean.astype(f32)).astype(f32); rv2 = ((f32(1) - mom) * rv + mom * ub).astype(f32)
    return st, rm2, rv2, nbt + 1.0


def bn_model(case, inp, defect=None, stats="fp64"):
    """the `got` dict of GB.bn_judge from the fp32 model of the route the case must take"""
    _name, (B, L, C), _ld, _dts, _offs, _scale, mode, opts = case
    rows, fmt = B * L, inp["fmt"]
    ld_ok = GB.case_ld(case) % 4 == 0
    det = "det" in opts
    rf = GB.expected_route(rows, C, ld_ok, det, mode, 0)
    x = inp["x"].numpy().astype(f32); ga = inp["ga"].numpy().astype(f32); be = inp["be"].numpy().astype(f32)
    dy = inp["dy"].numpy().astype(f32)
    rm, rv = inp["rm"].numpy().astype(f32), inp["rv"].numpy().astype(f32)
    slope = f32(GB.SLOPE)
    out = lambda z: N.rtz(torch.from_numpy(z.astype(np.float64)), fmt) if (defect == "truncated output" and fmt != "f32") else \
        N.rne(torch.from_numpy(z.astype(np.float64)), fmt)
    if mode == "plain":
        return dict(y=out(np.where(x > 0, x, (slope * x).astype(f32))), dx=out(np.where(x > 0, dy, (slope * dy).astype(f32))))
    if mode == "eval":
        st = np.stack([rm, (1.0 / np.sqrt((rv + f32(GB.EPS)).astype(f32).astype(np.float64))).astype(f32)], 1)
        rm2, rv2, nbt = rm, rv, inp["nbt"]
    else:
        S1, S2 = _column_sums(x, x, x, rows, rf, defect, wide=stats == "fp64")
        st, rm2, rv2, nbt = _finalize(S1, S2, float(rows), rm, rv, inp["nbt"], defect)
    mean, rstd = st[:, 0], st[:, 1]
    sc = (ga * rstd).astype(f32); sh = _fma(-mean, sc, be)
    xh = ((x - mean).astype(f32) * rstd).astype(f32)
    z4 = _fma(x, sc, sh)                      # the 4-wide apply's spelling
    zs = _fma(xh, ga, be)                     # the scalar kernels' and the reduce kernels' spelling
    z = z4 if rf["apply"] else zs
    got = dict(st=torch.from_numpy(st.astype(np.float64)), y=out(np.where(z > 0, z, (slope * z).astype(f32))),
               rm=torch.from_numpy(rm2.astype(np.float64)), rv=torch.from_numpy(rv2.astype(np.float64)), nbt=nbt)
    if mode == "eval":
        return got
    rb = GB.expected_route(rows, C, ld_ok, det, mode, 1)
    neg_r = (x <= 0) if defect == "mask from x > 0" else (zs <= 0)
    dz_r = np.where(neg_r, (dy * slope).astype(f32), dy)
    S1, S2 = _column_sums(dz_r, dz_r, x if defect == "S2 with x in place of xhat" else xh, rows, rb, defect)
    n = f32(rows - 1) if defect == "inv_n = 1 / (n - 1)" else f32(rows)
    inv_n = f32(1) / n
    k1 = (S1.astype(f32) * inv_n).astype(f32); k2 = (S2.astype(f32) * inv_n).astype(f32)
    if rb["apply"]:
        pos = (x > 0) if defect == "mask from x > 0" else (z4 > 0)
        dz = np.where(pos, dy, (slope * dy).astype(f32))
        dx = (sc * ((dz - k1).astype(f32) - (xh * k2).astype(f32)).astype(f32)).astype(f32)
    else:
        dz = dz_r
        dx = ((ga * rstd).astype(f32) * ((dz - k1).astype(f32) - (xh * k2).astype(f32)).astype(f32)).astype(f32)
    got.update(dx=out(dx), dbe=torch.from_numpy((inp["db0"].numpy().astype(f32) + S1.astype(f32)).astype(np.float64)),
               dga=torch.from_numpy((inp["dg0"].numpy().astype(f32) + S2.astype(f32)).astype(np.float64)))
    return got


def _judge_case(case, dt, off, defect=None, stats="fp64"):
    tag = f"model: {case[0]} [{GB.FMT[dt]}, mean {off:g} sigma]" + (f" defect: {defect}" if defect else "") + (" fp32 statistics sums" if stats == "fp32" else "")
    inp = GB.bn_inputs(case, dt, off)
    _n, (B, L, C), _ld, _dts, _offs, _scale, mode, opts = case
    ref = GB.bn_reference(inp, GB.expected_route(B * L, C, GB.case_ld(case) % 4 == 0, "det" in opts, mode, 0))
    return GB.bn_judge(bn_model(case, inp, defect, stats), inp, ref, tag)


@pytest.mark.parametrize("case", GB.BN_CASES, ids=GB._ids(GB.BN_CASES))
def test_models_pass_the_checks_of_every_gpu_case(case):
    """every (type, offset) run of every GPU case: the U cap holds (asserted inside bn_reference) and the model of its route is inside every bound"""
    fails = []
    for dt, off in GB.case_runs(case):
        fails += _judge_case(case, dt, off)
    GB._raise(fails)


def test_fp32_statistics_sums_fail_check_b_at_30_sigma():
    """The forward statistics with fp32 per-thread sums and fp32 block partials (the kernels before this file existed): every hard bound holds,
    and check B fails exactly where the device failed it -- fp16 dx at 30 sigma with 2.969e-3 of the elements off RNE(ref) against 4.3e-4 for
    torch's fp32, at 100 sigma 4.5e-2 (and the forward 5.3e-2); with sixteen rows per thread (C 516, TY 1) 1.0e-1 at 30 sigma."""
    for name, off, want in (("4-wide fold_finalize", 30.0, {"dx B"}), ("4-wide fold_finalize", 100.0, {"y B", "dx B"}), ("4-wide C516 (TX 129, TY 1)", 30.0, {"y B", "dx B"})):
        names = {n for n, _m in _judge_case(_case(name), 2, off, stats="fp32")}
        assert names == want, (name, off, names)
        for dt in (0, 1) if off < 100 else (0,):       # fp32 has no check B; bf16 squares and block sums of a few rows are exact in fp32
            assert not _judge_case(_case(name), dt, off, stats="fp32")


def _case(name):
    return next(c for c in GB.BN_CASES if c[0] == name)


DEFECTS = [
    # defect, case, dtype, offset, checks of which at least one must fail
    ("last row dropped", "4-wide fold_finalize", 0, 0.0, {"stats", "y A"}),
    ("last row dropped", "scalar odd C6", 0, 30.0, {"stats", "dbeta", "dgamma"}),
    ("inv_n = 1 / (n - 1)", "4-wide fold_finalize", 0, 0.0, {"dx A"}),
    ("inv_n = 1 / (n - 1)", "scalar odd C6", 0, 30.0, {"dx A"}),
    ("biased variance in the running update", "4-wide fold_finalize", 0, 0.0, {"running var"}),
    ("S2 with x in place of xhat", "4-wide fold_finalize", 0, 30.0, {"dgamma", "dx A"}),
    ("mask from x > 0", "4-wide fold_finalize", 0, 0.0, {"dx A", "dbeta", "dgamma"}),
    ("mask from x > 0", "scalar odd C6", 1, 30.0, {"dx A", "dbeta", "dgamma"}),
    ("truncated output", "4-wide fold_finalize", 1, 30.0, {"y A", "y B", "dx A", "dx B"}),
    ("truncated output", "4-wide fold_finalize", 2, 100.0, {"y A", "y B", "dx A", "dx B"}),
]


@pytest.mark.parametrize("defect,name,dt,off,expect", DEFECTS, ids=[f"{d} ({n}, {GB.FMT[t]})" for d, n, t, _o, _e in DEFECTS])
def test_planted_defects_are_rejected(defect, name, dt, off, expect):
    fails = _judge_case(_case(name), dt, off, defect)
    names = {n for n, _m in fails}
    print(f"[defect] {defect}: rejected by {sorted(names)}")
    assert names & expect, f"{defect}: not rejected by any of {sorted(expect)} (failed: {sorted(names)})"


# ---------------------------------------------------------------- from-parts fold
def parts_model(pi, fold32=False):
    p = pi["parts"].numpy().astype(f32)
    nparts, C = pi["nparts"], pi["C"]
    if fold32:      # the defect: the 16 row lanes and their meeting in fp32
        lanes = np.zeros((16, 2 * C), f32)
        for r in range(nparts):
            lanes[r % 16] = (lanes[r % 16] + p[r]).astype(f32)
        S = np.zeros(2 * C, f32)
        for k in range(16):
            S = (S + lanes[k]).astype(f32)
        S = S.astype(np.float64)
    else:
        lanes = np.zeros((16, 2 * C), np.float64)
        for r in range(nparts):
            lanes[r % 16] += p[r]
        S = np.zeros(2 * C)
        for k in range(16):
            S = S + lanes[k]
    S = S.reshape(C, 2)
    st, rm, rv, nbt = _finalize(S[:, 0], S[:, 1], float(pi["n"]), pi["rm"].numpy().astype(f32), pi["rv"].numpy().astype(f32), pi["nbt"])
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    return dict(st=t(st), rm=t(rm), rv=t(rv), nbt=nbt)


@pytest.mark.parametrize("size", GB.PARTS_SIZES, ids=[f"{n}x{c}" for n, c in GB.PARTS_SIZES])
def test_from_parts_fold_fp64_passes_fp32_is_rejected(size):
    pi = GB.parts_inputs(*size)
    ref = GB.parts_reference(pi)
    if size[1] >= 2:
        assert float((ref["st"]["mean"] ** 2 / ref["st"]["var"]).max()) > 5e3            # the channels where fp64 matters
    GB._raise(GB.parts_judge(parts_model(pi), pi, ref, f"model: from parts {size[0]} x {size[1]}"))
    if size[0] >= 2048:
        fails = GB.parts_judge(parts_model(pi, fold32=True), pi, ref, f"model: from parts {size[0]} x {size[1]} defect: fp32 fold")
        assert "stats" in {n for n, _m in fails}, "an fp32 fold at mean^2 / var = 1e4 was not rejected"


# ---------------------------------------------------------------- fused tail and head: the U cap of every GPU case; the tail forward's model
def tail_model_logits(ti, boundary_defect=False):
    """tail_fwd_kernel: a = lrelu(fma(y, sc, sh)) in fp32, three per-row dot products (float64 here: better than any fp32 order), the taps
    of a row outside the sample zero -- or, the defect, taken from the neighbouring sample's rows of the flat [B L] buffer"""
    y = ti["y"].numpy().astype(f32); B, L, C = y.shape
    st = N.bn_stats(ti["y"].reshape(B * L, C), GB.EPS)
    mean, rstd = st["mean"].numpy().astype(f32), st["rstd"].numpy().astype(f32)
    ga, be, w = ti["ga"].numpy().astype(f32), ti["be"].numpy().astype(f32), ti["w3"].numpy().astype(f32)
    sc = (ga * rstd).astype(f32); sh = _fma(-mean, sc, be)
    z = _fma(y, sc, sh)
    a = np.where(z > 0, z, (f32(GB.SLOPE) * z).astype(f32)).astype(np.float64)
    p = np.stack([(a * w[t].astype(np.float64)).sum(-1) for t in range(3)])           # (3, B, L)
    flat = p.reshape(3, B * L)
    out = np.zeros(B * L)
    for r in range(B * L):
        l = r % L
        s = flat[1, r]
        if r > 0 and (l > 0 or boundary_defect):
            s += flat[0, r - 1]
        if r + 1 < B * L and (l + 1 < L or boundary_defect):
            s += flat[2, r + 1]
        out[r] = s + (float(ti["bias"]) if ti["bias"] is not None else 0.0)
    return torch.from_numpy(out.astype(f32).astype(np.float64)).reshape(B, L)


def test_tail_forward_model_passes_and_an_unzeroed_boundary_tap_is_rejected():
    ti = GB.tail_inputs(3, 37, 64, 1)
    ref = GB.tail_reference(ti)
    GB._raise(GB.tail_judge(dict(logits=tail_model_logits(ti)), ti, ref, "model: tail C64 L37 [bf16]"))
    fails = GB.tail_judge(dict(logits=tail_model_logits(ti, boundary_defect=True)), ti, ref, "model: tail C64 L37 [bf16] defect: boundary tap")
    assert fails and fails[0][0] == "logits", "a sample-boundary tap that is not zeroed was not rejected"
    assert "4 of" in fails[0][1] or "outside the bound" in fails[0][1]


def test_tail_reference_matches_autograd():
    """tail_logits / tail_bwd (explicit formulas) against torch autograd of the layer-wise composition in float64"""
    import torch.nn.functional as F
    ti = GB.tail_inputs(2, 9, 16, 0)
    y, ga, be, w3, dl = ti["y"], ti["ga"], ti["be"], ti["w3"], ti["dl"]
    B, L, C = y.shape
    st = N.bn_stats(y.reshape(B * L, C), GB.EPS)
    yr = y.permute(0, 2, 1).contiguous().requires_grad_(True); gr = ga.clone().requires_grad_(True); br = be.clone().requires_grad_(True)
    wr = w3.t().reshape(1, C, 3).contiguous().requires_grad_(True); bb = ti["bias"].clone().requires_grad_(True)
    lg = F.conv1d(F.leaky_relu(F.batch_norm(yr, None, None, gr, br, True, 0.1, GB.EPS), GB.SLOPE), wr, bb, padding=1)
    lg.backward(dl.reshape(B, 1, L))
    assert torch.allclose(N.tail_logits(y, ga, be, st, w3, ti["bias"], GB.SLOPE), lg.detach().reshape(B, L), rtol=1e-12, atol=1e-12)
    dy, dga, dbe, dw3, dbias = N.tail_bwd(y, ga, be, st, w3, GB.SLOPE, dl)
    for a, b in ((dy, yr.grad.permute(0, 2, 1)), (dga, gr.grad), (dbe, br.grad), (dw3, wr.grad[0].t()), (dbias, bb.grad[0])):
        assert torch.allclose(a, b, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("stride,L", [(2, 16), (1, 37)])
def test_head_reference_matches_autograd(stride, L):
    import torch.nn.functional as F
    hi = GB.head_inputs(3, L, 16, stride, 0)
    x, w, b, da = hi["x"], hi["w"], hi["bias"], hi["da"]
    xr = x.reshape(3, 1, L).clone().requires_grad_(True); wr = w.t().reshape(16, 1, 3).contiguous().requires_grad_(True); br = b.clone().requires_grad_(True)
    a0 = F.leaky_relu(F.conv1d(xr, wr, br, stride=stride, padding=1), GB.SLOPE)
    a0.backward(da.permute(0, 2, 1))
    dw, db, dx = N.head_bwd(da, x, w, b, GB.SLOPE, stride)
    for a, c in ((dw, wr.grad[:, 0].t()), (db, br.grad), (dx, xr.grad[:, 0])):
        assert torch.allclose(a, c, rtol=1e-10, atol=1e-12)


def test_mask_uncertain_share_of_every_tail_and_head_case():
    """the references of the GPU file's tail, head and sequence cases, built from the same seeds: each asserts its U cap"""
    worst = 0.0
    for dt in (0, 1, 2):
        for L in (37, 8):
            for C in GB.TAIL_C[dt]:
                worst = max(worst, GB.tail_reference(GB.tail_inputs(3, L, C, dt))["share"])
        worst = max(worst, GB.tail_reference(GB.tail_inputs(3, 37, 64, dt, bias=False, acc=False))["share"])
        for s, B, L in GB.HEAD_GEOM:
            for i, C0 in enumerate(GB.TAIL_C[dt]):
                worst = max(worst, GB.head_reference(GB.head_inputs(B, L, C0, s, dt, bias=i % 2 == 0))["share"])
    print(f"[model] largest mask-uncertain share over the tail and head cases: {worst:.2e}")
    assert worst <= GB.U_CAP
