"""Float64 reference of ONE ResBlock, forward and backward, and the checks that hold the ResBlock executor (csrc/net.hip res_forward /
res_backward) to it (imported by tests/test_resblock_numerics_cpu.py and tests/test_gpu_resblock_rounding.py; not a conftest).

Reference: oracle.unet.resblock in float64 under torch autograd (oracle/quant.py's `q` is the identity outside float32).  Its inputs are
what the engine holds: x and dy rounded once to the storage format, the three conv weights rounded to it (the GEMMs read the 16-bit copy),
every other parameter and the embedding in fp32.  The intermediates the executor's side products are sums of -- dh1, the gradient at the
input of the second GroupNorm, and with use_scale_shift_norm the FiLM rows -- come from a restated backward built from tests/numerics.py
(gn_fwd, gn_bwd, conv1d_fwd, conv1d_dgrad); `reference` asserts that the restated backward agrees with autograd.

Two yardsticks come from the same function: the float32 oracle, and the float32 oracle inside oracle.quant.bf16_storage(True, fmt).

The embedding of every case is one-hot, emb[b, b] = 1: SiLU(emb) has one non-zero per row, so column b of the emb_layers.1.weight gradient
is silu(1) times sample b's per-sample column sums and the side product of the fused GroupNorm backward can be read off the ABI:
ps[b, :] = g_w[:, b] / silu_f32(1) (`per_sample_sums`).

Preloaded gradients: the engine adds every parameter gradient onto what the buffer held.  `preload` gives those contents, and the
yardsticks go through the same fp32 addition and subtraction (`through_preload`) as the engine's figures do, so that its rounding is part
of the yardstick and not of the engine's error.

The checks (A to E of the GPU test's docstring) take a `got` dict -- y, dx, demb, g (parameter gradients minus the preload), raw (with
it), ps -- and a `route` dict; they return (name, worst error / bound) pairs and raise AssertionError naming the check."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import numerics as N
from oracle import quant as Q
from oracle import unet as U
from param_gen import gen_param, normal

EMB = 128
GROUPS = U.GN_GROUPS
U_S = {"f32": 0.0, "bf16": 2.0 ** -9, "f16": 2.0 ** -12}            # unit roundoff of the storage format
CONVS = ("in_layers.2.weight", "out_layers.3.weight", "skip_connection.weight")
BIASES = ("in_layers.2.bias", "emb_layers.1.bias", "out_layers.3.bias", "skip_connection.bias")
# factor and floors of gpu_util.bf16_gap_bound, restated because gpu_util opens the library; test_resblock_numerics_cpu.py pins them equal
BF16_GAP_FACTOR, BF16_FLOOR, F16_FLOOR = 2.0, 2.0 ** -7, 2.0 ** -9
SILU1_F32 = float(F.silu(torch.ones((), dtype=torch.float32)))     # what the engine's fp32 SiLU makes of emb = 1 (to an ulp)


def param_shapes(cin, cout, ssn):
    ew = 2 * cout if ssn else cout
    s = {"in_layers.0.weight": (cin,), "in_layers.0.bias": (cin,), "in_layers.2.weight": (cout, cin, 3), "in_layers.2.bias": (cout,),
         "emb_layers.1.weight": (ew, EMB), "emb_layers.1.bias": (ew,), "out_layers.0.weight": (cout,), "out_layers.0.bias": (cout,),
         "out_layers.3.weight": (cout, cout, 3), "out_layers.3.bias": (cout,)}
    if cin != cout:
        s["skip_connection.weight"] = (cout, cin, 1); s["skip_connection.bias"] = (cout,)
    return s


def lout(L, updown):
    return L // 2 if updown == 1 else (2 * L if updown == 2 else L)


def one_hot_emb(B):
    assert B <= EMB
    e = torch.zeros(B, EMB)
    e[torch.arange(B), torch.arange(B)] = 1.0
    return e


def make_inputs(B, cin, cout, L, updown, ssn, seed=11):
    """fp32 master values, as a caller hands them to the engine: params, x, dy, emb (one-hot), preload (gradient buffer contents)"""
    shapes = param_shapes(cin, cout, ssn)
    params = {k: torch.from_numpy(gen_param(seed, k, s)) for k, s in shapes.items()}
    pre = {k: 0.25 * torch.from_numpy(normal(s, seed=seed + 100 + i)) for i, (k, s) in enumerate(shapes.items())}
    return dict(B=B, cin=cin, cout=cout, L=L, Lo=lout(L, updown), updown=updown, ssn=ssn, params=params, preload=pre,
                x=torch.from_numpy(normal((B, cin, L), seed=seed + 1)), dy=torch.from_numpy(normal((B, cout, lout(L, updown)), seed=seed + 2)),
                emb=one_hot_emb(B))


def held(inp, fmt):
    """float64 copies of what the engine of storage format `fmt` holds: x, dy and the conv weights rounded once, the rest unchanged"""
    p = {k: (N.to_storage(v, fmt) if k in CONVS else v.double()) for k, v in inp["params"].items()}
    return p, N.to_storage(inp["x"], fmt), N.to_storage(inp["dy"], fmt), inp["emb"].double()


def run_oracle(inp, fmt, dtype, storage=None):
    """oracle.unet.resblock on the engine-held values in `dtype`; storage: None, or the torch dtype whose storage the float32 oracle emulates.
    Returns y, dx, demb, g (parameter gradients) as float64 CPU tensors."""
    p, x, dy, emb = held(inp, fmt)
    sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    xr = x.to(dtype).clone().requires_grad_(True); er = emb.to(dtype).clone().requires_grad_(True)
    with Q.bf16_storage(storage is not None, storage if storage is not None else torch.bfloat16):
        y = U.resblock(sd, "", xr, er, up=inp["updown"] == 2, down=inp["updown"] == 1, scale_shift=bool(inp["ssn"]))
        y.backward(dy.to(dtype))
    return dict(y=y.detach().double(), dx=xr.grad.double(), demb=er.grad.double(), g={k: v.grad.double() for k, v in sd.items()})


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def reference(inp, fmt):
    """The float64 reference: run_oracle's outputs plus dout, dh1, the per-sample sums ps (B, W) the executor hands to the embedding
    projection (W = cout: column sums of dh1; 2 cout with use_scale_shift_norm: the [scale | shift] rows of the FiLM backward) with their
    magnitudes ps_mag = the same sums over absolute values, and abs_c = sum over (b, l) of |dh1| per channel."""
    R = run_oracle(inp, fmt, torch.float64)
    p, x, dy, emb = held(inp, fmt)
    ud, G = inp["updown"], GROUPS
    a1 = N.gn_fwd(x, G, p["in_layers.0.weight"], p["in_layers.0.bias"], U.GN_EPS, silu=True, resample=ud)
    e = F.linear(F.silu(emb), p["emb_layers.1.weight"], p["emb_layers.1.bias"])
    da2 = N.conv1d_dgrad(dy, p["out_layers.3.weight"], inp["Lo"], 1, 1, 1)
    g2, b2 = p["out_layers.0.weight"], p["out_layers.0.bias"]
    if inp["ssn"]:
        h1 = N.conv1d_fwd(a1, p["in_layers.2.weight"], p["in_layers.2.bias"], 1, 1, 1)
        scale, shift = torch.chunk(e[:, :, None], 2, dim=1)
        hn = N.gn_fwd(h1, G, g2, b2, U.GN_EPS, silu=False)
        dz = da2 * _silu_grad(hn * (1 + scale) + shift)
        dh1, _, _ = N.gn_bwd(h1, G, g2, b2, dz * (1 + scale), U.GN_EPS, silu=False)
        ps = torch.cat([(dz * hn).sum(2), dz.sum(2)], dim=1)
        ps_mag = torch.cat([(dz * hn).abs().sum(2), dz.abs().sum(2)], dim=1)
    else:
        h1 = N.conv1d_fwd(a1, p["in_layers.2.weight"], p["in_layers.2.bias"], 1, 1, 1, row=e)
        dh1, _, _ = N.gn_bwd(h1, G, g2, b2, da2, U.GN_EPS, silu=True)
        ps, ps_mag = dh1.sum(2), dh1.abs().sum(2)
    R.update(dout=dy, dh1=dh1, ps=ps, ps_mag=ps_mag, abs_c=dh1.abs().sum(dim=(0, 2)))
    # the restated backward against autograd: the same float64 arithmetic up to the order of a few operations
    tol = lambda ref: 1e-11 * (1.0 + float(ref.abs().max()))
    assert float((dh1.sum(dim=(0, 2)) - R["g"]["in_layers.2.bias"]).abs().max()) <= tol(R["g"]["in_layers.2.bias"])
    assert float((ps.sum(0) - R["g"]["emb_layers.1.bias"]).abs().max()) <= tol(R["g"]["emb_layers.1.bias"])
    da1 = N.conv1d_dgrad(dh1, p["in_layers.2.weight"], inp["Lo"], 1, 1, 1)
    dxr = N.conv1d_dgrad(dy, p["skip_connection.weight"], inp["Lo"]) if "skip_connection.weight" in p else dy
    dx, _, _ = N.gn_bwd(x, G, p["in_layers.0.weight"], p["in_layers.0.bias"], da1, U.GN_EPS, silu=True, resample=ud, dxr=dxr)
    assert float((dx - R["dx"]).abs().max()) <= tol(R["dx"])
    return R


def storage_dtype(fmt):
    return {"bf16": torch.bfloat16, "f16": torch.float16}[fmt]


def through_preload(g, pre):
    """the fp32 `+=` onto the preloaded contents and the fp32 subtraction that takes them off again"""
    return {k: ((pre[k].float() + v.float()) - pre[k].float()).double() for k, v in g.items()}


def yardsticks(inp, fmt):
    """(float32 oracle, storage-emulating float32 oracle or None for fmt = f32), parameter gradients through the preload"""
    o32 = run_oracle(inp, fmt, torch.float32)
    o32["g"] = through_preload(o32["g"], inp["preload"])
    oq = None
    if fmt != "f32":
        oq = run_oracle(inp, fmt, torch.float32, storage=storage_dtype(fmt))
        oq["g"] = through_preload(oq["g"], inp["preload"])
    return o32, oq


def per_sample_sums(g_emb_w, B, silu1=SILU1_F32):
    """ps[b, :] = g_w[:, b] / silu(1) from the emb_layers.1.weight gradient of a one-hot embedding; the columns >= B must be exactly 0.
    silu1: the fp32 value for an engine (its SiLU is within an ulp or two of it: 4 u32 |ps|, far inside every bound that judges ps);
    math-exact float64 for the float64 reference."""
    g = g_emb_w.double()
    assert g.shape[1] == B or float(g[:, B:].abs().max()) == 0.0, "emb_layers.1.weight gradient: a column of an all-zero SiLU(emb) column is not 0"
    return (g[:, :B] / silu1).t().contiguous()


def tensors(out):
    """flat view of a result dict: y, dx, demb and every parameter gradient under 'g:<key>'"""
    t = {k: out[k] for k in ("y", "dx", "demb")}
    t.update({"g:" + k: v for k, v in out["g"].items()})
    return t


def _l2(a, b):
    return float((a.double() - b.double()).norm())


def rel_l2(a, b):
    return _l2(a, b) / (float(b.double().norm()) + 1e-300)


# ---------------------------------------------------------------- check A: the whole block against float64
def whole_block_bounds(ref, o32, oq, fmt):
    """per tensor: (absolute L2 bound, its description).  16-bit: gpu_util.bf16_gap_bound of the storage-emulating oracle's own distance
    from float64 (relative L2; the project's factor and floors).  fp32: 4 max(e32, r ||ref||), e32 the float32 oracle's own distance from
    float64 and r the median of e32 / ||ref|| over the tensors (assert_grad_bound of tests/test_gpu_usleep_train.py)."""
    tr = tensors(ref)
    if fmt == "f32":
        t32 = tensors(o32)
        e32 = {k: _l2(t32[k], tr[k]) for k in tr}
        n64 = {k: float(tr[k].norm()) for k in tr}
        r = float(np.median([e32[k] / n64[k] for k in tr if n64[k] > 0]))
        return {k: 4 * max(e32[k], r * n64[k]) for k in tr}, {k: e32[k] for k in tr}
    tq = tensors(oq)
    floor = BF16_FLOOR if fmt == "bf16" else F16_FLOOR
    gap = {k: rel_l2(tq[k], tr[k]) for k in tr}
    return {k: max(BF16_GAP_FACTOR * gap[k], floor) * float(tr[k].norm()) for k in tr}, {k: gap[k] * float(tr[k].norm()) for k in tr}


def check_whole_block(got, ref, o32, oq, fmt):
    """A.  Returns {tensor: (error / bound, error / yardstick)}; raises on a tensor outside its bound or with a NaN."""
    bounds, yard = whole_block_bounds(ref, o32, oq, fmt)
    tr, tg = tensors(ref), tensors(got)
    out, bad = {}, []
    for k in tr:
        e = _l2(tg[k], tr[k])
        out[k] = (e / bounds[k] if bounds[k] > 0 else (0.0 if e == 0 else math.inf), e / yard[k] if yard[k] > 0 else math.nan)
        if not e <= bounds[k]:
            bad.append(f"{k}: |got - ref| {e:.3e} > bound {bounds[k]:.3e} (yardstick {yard[k]:.3e}, |ref| {float(tr[k].norm()):.3e})")
    assert not bad, "check A (whole block against float64): " + "; ".join(bad)
    return out


# ---------------------------------------------------------------- check B: outputs whose operands are known exactly
def skip_input(inp, fmt):
    """xr, the operand of the skip conv's weight gradient, as the engine stores it: x itself, or its resampled copy rounded to storage"""
    x = N.to_storage(inp["x"], fmt)
    return x if inp["updown"] == 0 else N.to_storage(N.gn_xr(x, inp["updown"]), fmt)


def check_exact_operands(got_raw, inp, fmt, report=False, route=""):
    """B.  out_layers.3.bias and skip_connection.bias against bias_grad(rne(dy)), skip_connection.weight against conv1d_wgrad(xr, rne(dy)),
    each ON TOP of the preloaded contents, by the one-rounding-per-accumulation bound gamma(B Lout) * mag (numerics.check, fp32 outputs)."""
    dy = N.to_storage(inp["dy"], fmt); n = inp["B"] * inp["Lo"]; pre = inp["preload"]
    out, bad = {}, []

    def one(k, ref, mag):
        try:
            out[k] = N.check(got_raw[k], ref, mag, n, "f32", route=f"{route} B {k}", report=report)["worst"]
        except AssertionError as e:
            bad.append(str(e))
    for k in ("out_layers.3.bias", "skip_connection.bias"):
        if k in pre:
            one(k, N.bias_grad(dy, acc=pre[k].double()), N.bias_grad(dy.abs(), acc=pre[k].double().abs()))
    k = "skip_connection.weight"
    if k in pre:
        xr = skip_input(inp, fmt)
        one(k, N.conv1d_wgrad(xr, dy, 1, acc=pre[k].double()), N.conv1d_wgrad(xr.abs(), dy.abs(), 1, acc=pre[k].double().abs()))
    assert not bad, "check B (exactly known operands, numerics.check's hard bound): " + "; ".join(bad)
    return out


# ---------------------------------------------------------------- check C: per-sample sums
def _ratio(err, bound):
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(torch.nan_to_num(r, nan=math.inf).max())


def check_per_sample(ps, ref, a_bound_emb_w, fmt):
    """C.  per (b, c): |ps - ref| <= 2 (2 u_s + gamma(Lout)) sum_l |dh1_ref| + the whole-block bound of A for the emb_layers.1.weight
    gradient (an L2 bound: no element's error exceeds it), taken back through the division by silu(1)."""
    Lo = ref["dh1"].shape[2]
    bound = 2 * (2 * U_S[fmt] + N.gamma(Lo)) * ref["ps_mag"] + a_bound_emb_w / SILU1_F32
    err = (ps.double() - ref["ps"]).abs()
    r = _ratio(err, bound)
    assert r <= 1.0, (f"check C (per-sample sums against float64): worst {r:.3g} x bound at (b, c) = "
                      f"{tuple(int(v) for v in np.unravel_index(int(torch.argmax(torch.nan_to_num(err / bound, nan=math.inf))), err.shape))}")
    return r


def check_producers_agree(ps_a, ps_b, ref, fmt):
    """C, between two producers on the same inputs: |ps_A - ps_B| <= 2 (2 u_s + 2 gamma(Lout)) sum_l |dh1_ref|"""
    Lo = ref["dh1"].shape[2]
    bound = 2 * (2 * U_S[fmt] + 2 * N.gamma(Lo)) * ref["ps_mag"]
    r = _ratio((ps_a.double() - ps_b.double()).abs(), bound)
    assert r <= 1.0, f"check C (two producers of the per-sample sums): worst {r:.3g} x bound"
    return r


# ---------------------------------------------------------------- check D: the identities
B_TOTAL, B_GEMM, B_COLSUM, B_STAGED, B_NONE = 3, 2, 1, 4, 0          # eegldm_debug_res_last_route's producer codes


def check_identities(got, ref, inp, fmt, route):
    """D.  Without use_scale_shift_norm in_layers.2.bias and emb_layers.1.bias both hold the total of dh1; out_layers.3.bias and
    skip_connection.bias both hold the column sums of dy.  `got['g']` has the preload taken off, which costs each side one fp32 rounding of
    (preload + gradient) and one of the difference: 2 u32 (|preload| + |ref|) per side is added to every bound."""
    B, Lo = inp["B"], inp["Lo"]; out = {}
    pre = {k: v.double().abs() for k, v in inp["preload"].items()}
    off = lambda k, r: 2 * N.U32 * (2 * pre[k] + r.abs())      # the sum rounds at up to |preload| + |gradient|, the difference at up to |preload|
    if not inp["ssn"]:
        k1, k2 = "in_layers.2.bias", "emb_layers.1.bias"
        d = (got["g"][k1].double() - got["g"][k2].double()).abs()
        if route["b_c1"] == B_TOTAL:
            bound = 2 * N.gamma(B) * got_ps_abs(ref)
        else:
            bound = 2 * (2 * U_S[fmt] + N.gamma(B * Lo)) * ref["abs_c"]
        bound = bound + off(k1, ref["g"][k1]) + off(k2, ref["g"][k2])
        out["c1 bias = emb bias"] = _ratio(d, bound)
    if "skip_connection.bias" in got["g"]:
        k1, k2 = "out_layers.3.bias", "skip_connection.bias"
        d = (got["g"][k1].double() - got["g"][k2].double()).abs()
        dy = N.to_storage(inp["dy"], fmt)
        bound = 2 * N.gamma(B * Lo) * N.bias_grad(dy.abs()) + off(k1, ref["g"][k1]) + off(k2, ref["g"][k2])      # each within B's bound of the same sum
        out["c2 bias = skip bias"] = _ratio(d, bound)
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, f"check D (identities): {bad}"
    return out


def got_ps_abs(ref):
    """sum_b |ps| per channel, from the reference (no bound takes a magnitude from an engine output)"""
    return ref["ps"].abs().sum(0)


# ---------------------------------------------------------------- check E: a NaN in dy
def check_nan_masks(got, ref):
    """E.  dx, demb and the bias gradients: NaN exactly where the float64 reference has one (numerics._nonfinite_agree), finite elsewhere"""
    bad = []
    pairs = [("dx", got["dx"], ref["dx"]), ("demb", got["demb"], ref["demb"])] + [(k, got["raw"][k], ref["g"][k]) for k in BIASES if k in ref["g"]]
    for name, g, r in pairs:
        g = g.double(); fin, bad_nan, bad_inf = N._nonfinite_agree(g, r)
        extra = fin & ~torch.isfinite(g)
        if bool(bad_nan.any()) or bool(bad_inf.any()) or bool(extra.any()):
            bad.append(f"{name}: {int(bad_nan.sum())} NaNs of the reference missing, {int(extra.sum())} non-finite values where the reference is finite")
    assert not bad, "check E (NaN masks): " + "; ".join(bad)


# ---------------------------------------------------------------- all of A to D on one result
def run_checks(got, ref, o32, oq, inp, fmt, route, collect=False):
    """A, B, C (against the reference), D on one result; every check runs whatever the others found.  `got`: y, dx, demb, g (preload taken
    off), raw (with it).  Returns the report fields, with `failed` = {check letter: message}; raises on a failure unless `collect`."""
    failed, rep = {}, dict(A=math.nan, A_at="", A_yard=math.nan, B=math.nan, C=math.nan, D=math.nan)

    def attempt(letter, fn):
        try:
            return fn()
        except AssertionError as e:
            failed[letter] = str(e)
            return None
    a = attempt("A", lambda: check_whole_block(got, ref, o32, oq, fmt))
    if a is not None:
        ka = max(a, key=lambda k: a[k][0])
        rep.update(A=a[ka][0], A_at=ka, A_yard=max(v[1] for v in a.values() if not math.isnan(v[1])))
    b = attempt("B", lambda: check_exact_operands(got["raw"], inp, fmt))
    if b is not None:
        rep["B"] = max(b.values()) if b else 0.0
    bounds, _ = whole_block_bounds(ref, o32, oq, fmt)
    rep["ps"] = attempt("C", lambda: per_sample_sums(got["g"]["emb_layers.1.weight"], inp["B"]))
    if rep["ps"] is not None:
        c = attempt("C", lambda: check_per_sample(rep["ps"], ref, bounds["g:emb_layers.1.weight"], fmt))
        if c is not None:
            rep["C"] = c
    d = attempt("D", lambda: check_identities(got, ref, inp, fmt, route))
    if d is not None:
        rep["D"] = max(d.values()) if d else 0.0
    rep["failed"] = failed
    assert collect or not failed, " | ".join(failed.values())
    return rep


def report_line(name, fmt, route_txt, rep):
    return (f"[numerics] resblock {name:<26s} {fmt:>4s} route[{route_txt}] A={rep['A']:.3f}xbound ({rep['A_at']}; worst {rep['A_yard']:.2f}x yardstick) "
            f"B={rep['B']:.3f} C={rep['C']:.3f} D={rep['D']:.3f}")
