"""float64 references of the U-Sleep forward (csrc/usleep.hip, the taped forward of csrc/usleep_train.hip) and the bounds its kernels are held
to.  Shared by tests/test_gpu_usleep_fwd.py, tests/test_gpu_usleep_train.py and tests/test_usleep_fwd_numerics_cpu.py; not a conftest.

Every reference is evaluated in float64 on the exact fp32 operands, and every bound from the reference alone.  u = 2^-24, gamma(n) = (n + 4) u
(tests/numerics.py), `mag` = the same operation on the operands' magnitudes.  Bounds are first-order sums, doubled for the higher-order terms
(as the backward tests do), and absolute: a result near 0 needs no special case.

conv + ELU      s = bias + sum w x over the virtual input [a (nearest x2 when ups) | b2], both cropped to L, 'same' padding with `left` zeros on
                the left and K - 1 - left on the right.  A chain of Cin K fmaf and one add:  |ds| <= gamma(Cin K) mag.
                z = ELU(s):  d_z = gamma(Cin K) mag + 8 u |z| where the device may take the expm1f branch (s <= gamma mag): 4 ulp of expm1f, an
                ulp being at most 2 u of the value.  ELU is continuous with slope <= 1, so within gamma mag of 0 either branch is inside d_z.
BatchNorm eval  sc = gamma / sqrtf(rv + eps) (3 roundings: |dsc| <= 3 u |sc|), sh = beta - rm sc (2 roundings), y = fmaf(z, sc, sh).  The same
                rounded sc multiplies z and rm, so  y^ = (z - rm) sc^ + beta + roundings:
                d_y = 2 (3 u |(z - rm) sc| + u |rm sc| + u |sh| + u |y| + |sc| d_z).
BatchNorm train judged on the STORED z (itself judged by d_z): mean, var = fp64 sums (order free: dmean, dvar below), n = B L.
                dvar = (n + 4) 2^-53 * 2 mean(z^2) (the cancellation in E z^2 - mean^2), dmean = (n + 4) 2^-53 mean|z|.
   training path stat = (float) mean, (float)(1 / sqrt(var + eps)) in double:  dm = u |mean| + dmean,  rel. drstd = u + dvar / (2 (var + eps));
   (mode 2)      y = fmaf((z - mean^) rstd^, gamma, beta):  d_y = 2 (|gamma| (rstd (dm + u |z - mean|) + |zhat| (drstd + u)) + u |y|).
   inference     sc = gamma / sqrtf((float) var + eps): rel. dsc = 3 u + dvar / (2 (var + eps));  sh = beta - (float) mean * sc;  y = fmaf(z, sc, sh),
   path (mode 1) again with one sc for z and mean:  d_y = 2 (|zhat gamma| dsc + |sc| dm + u |mean sc| + u |sh| + u |y|).
   running       rm' = keep rm + mom (float) mean, rv' = keep rv + mom (float) unb, unb = var n / (n - 1), with the fp32 values mom = 0.1f and
   statistics    keep = 1.f - 0.1f:  d = 2 (u |keep r| + mom (2 u |new| + dnew) + u |r'|).  The counter goes up by exactly 1.
MaxPool         pad 0 on both sides at odd L, the zeros take part in the max; a NaN wins its pair.  Exact (torch.equal with torch on the stored y).
classifier      h = b0 + W0 x (C1 fmaf), t = tanhf(h) (4 ulp), m = (float) mean over the window in fp64, g = b3 + W3 m, e = ELU(g) (4 ulp of expm1f),
                y = b5 + W5 e:  d_t = gamma(C1) mag_h + 8 u |t|,  d_m = mean(d_t) + u |m|,  d_e = |W3| d_m + gamma(C1) mag_g + 8 u |e|,
                d_y = 2 (|W5| d_e + gamma(ncls) mag_y).  Positions past S win are not read."""
import numpy as np
import torch
import torch.nn.functional as F

import numerics as N
from param_gen import normal

U = 2.0 ** -24
U64 = 2.0 ** -53
EPS = float(np.float32(1e-5))                              # the kernels' 1e-5f
MOM = float(np.float32(0.1))                               # 0.1f
KEEP = float(np.float32(1.0) - np.float32(0.1))            # 1.f - 0.1f as the kernels form it
ELU_ULPS = 4                                               # expm1f / tanhf on the device, as tests/test_gpu_usleep_train.py grants them


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(normal(tuple(shape), seed=seed)).float() * scale


# ---------------------------------------------------------------------------------------------------- the virtual input and the convolution
def virtual_input(a, b2, ups, L):
    """[a (nearest x2 when ups) | b2], both cropped to L."""
    v = F.interpolate(a, scale_factor=2, mode="nearest") if ups else a
    v = v[..., :L]
    if b2 is not None:
        v = torch.cat([v, b2[..., :L]], 1)
    return v


def conv_same(v, w, bias, left=None):
    K = w.shape[-1]
    left = (K - 1) // 2 if left is None else left
    return F.conv1d(F.pad(v, (left, K - 1 - left)), w, bias)


def conv_ref(a, b2, w, bias, ups, L):
    """The forward's virtual input [a (nearest x2 when ups) | b2], both cropped to L, through conv1d 'same' (even K: extra zero on the right)."""
    return conv_same(virtual_input(a, b2, ups, L), w, bias)


ROWS = {1: (1, 1), 63: (3, 21), 64: (2, 32), 65: (5, 13), 130: (5, 26)}     # B * L -> (B, L): odd and even lengths, tiles ending inside samples


def conv_case(form, rows, Cout, Cin, K, seed):
    B, L = ROWS[rows]
    if form == "plain":
        Ca, La, ups, Cb, Lb = Cin, L + (seed % 2), 0, 0, 0           # (every other case: one cropped-off position at the end of a)
    elif form == "ups":
        Ca, La, ups, Cb, Lb = Cin, (L + 1) // 2, 1, 0, 0             # L = 2 La (even) or 2 La - 1 (odd: the last doubled sample is cropped)
    else:                                                            # upsampled + concatenated skip; odd L: the skip is one sample shorter than 2 La
        Ca = max(1, Cin // 2); Cb = Cin - Ca; ups = 1               # even L: the skip is one sample longer and is the one cropped
        La, Lb = (L + 1) // 2, (L if L % 2 else L + 1)
    a = rnd((B, Ca, La), seed)
    b2 = rnd((B, Cb, Lb), seed + 1) if Cb else None
    w = rnd((Cout, Cin, K), seed + 2, 1.0 / np.sqrt(Cin * K))
    dz = rnd((B, Cout, L), seed + 3)
    return dict(B=B, L=L, Ca=Ca, La=La, ups=ups, Cb=Cb, Lb=Lb, a=a, b2=b2, w=w, dz=dz, Cout=Cout, K=K)


# ---------------------------------------------------------------------------------------------------- layer cases
BASE = dict(rows=65, Cout=17, Cin=33, K=7)
LAYER_SWEEP = [dict(BASE, rows=r) for r in ROWS] + [dict(BASE, Cout=c) for c in (1, 4, 15, 16, 17, 33)] + [dict(BASE, Cin=c) for c in (1, 31, 32, 33, 65)] + \
              [dict(BASE, K=k) for k in (1, 2, 3, 5, 7, 9, 11, 13, 15)] + \
              [dict(rows=130, Cout=33, Cin=65, K=15), dict(rows=63, Cout=1, Cin=1, K=1), dict(rows=64, Cout=16, Cin=32, K=13)]
KINDS = ("plain", "mean30", "plain", "gamma0", "tinyvar", "rv0")


def layer_case(form, rows, Cout, Cin, K, seed):
    """conv_case + bias, BatchNorm parameters and running statistics.  Channel c is of kind KINDS[(c + seed) % 6]: 'mean30' (a channel mean of
    30 standard deviations, through the bias), 'gamma0' (gamma exactly 0), 'tinyvar' (variance of z near eps), 'rv0' (running_var near 0: the
    eval fold's sqrt sees eps alone).  left = (K - 1) // 2: K = 2 over the upsampled input is the decoder's pre-skip conv, its one zero on the right."""
    c = conv_case(form, rows, Cout, Cin, K, seed)
    if form == "ups_skip" and seed % 2 and c["L"] % 2 == 0:
        c["Lb"] = c["L"]; c["b2"] = c["b2"][..., :c["L"]].contiguous()     # every other even-length case: Lb == L, nothing cropped
    c["left"] = (K - 1) // 2
    c["bias"] = rnd((Cout,), seed + 4, 0.3)
    c["gamma"] = 1.0 + 0.5 * rnd((Cout,), seed + 5)
    c["beta"] = rnd((Cout,), seed + 6, 0.5)
    c["rm"] = rnd((Cout,), seed + 7, 0.3)
    c["rv"] = (0.5 + rnd((Cout,), seed + 8).abs()).float()
    c["nbt"] = torch.tensor([float(seed % 5)])
    c["kinds"] = [KINDS[(ch + seed) % len(KINDS)] for ch in range(Cout)]
    for ch, kind in enumerate(c["kinds"]):
        if kind == "mean30":
            c["bias"][ch] += 30.0
        elif kind == "gamma0":
            c["gamma"][ch] = 0.0
        elif kind == "tinyvar":
            c["w"][ch] *= 3e-3; c["bias"][ch] = 0.5
        elif kind == "rv0":
            c["rv"][ch] = 1e-7
    return c


def f64(t):
    return None if t is None else t.detach().cpu().double()


def elu64(s):
    return torch.where(s > 0, s, torch.expm1(s))


def conv_elu_ref(c):
    """-> s, z, d_z (float64) of a layer case."""
    v = virtual_input(f64(c["a"]), f64(c["b2"]), c["ups"], c["L"])
    w, bias = f64(c["w"]), f64(c["bias"])
    s = conv_same(v, w, bias, c["left"])
    mag = conv_same(v.abs(), w.abs(), bias.abs(), c["left"])
    g = N.gamma(w.shape[1] * w.shape[2]) * mag
    z = elu64(s)
    d_z = g + torch.where(s <= g, 2 * ELU_ULPS * U * z.abs(), torch.zeros_like(z))
    return s, z, d_z


def _bc(t):
    return t.reshape(1, -1, 1)


def bn_eval_ref(z, d_z, gamma, beta, rm, rv):
    """-> y, d_y: eval-mode BatchNorm of z (float64) as the fold kernel and the conv's epilogue evaluate it."""
    gamma, beta, rm, rv = (_bc(f64(t)) for t in (gamma, beta, rm, rv))
    sc = gamma / torch.sqrt(rv + EPS)
    sh = beta - rm * sc
    y = (z - rm) * sc + beta
    d = 2 * (3 * U * ((z - rm) * sc).abs() + U * (rm * sc).abs() + U * sh.abs() + U * y.abs() + sc.abs() * d_z)
    return y, d


def bn_train_ref(z, gamma, beta, rm, rv, nbt, mode):
    """Batch statistics, y and the running statistics from the stored z (fp32 values, evaluated in float64), with the bounds of the inference
    path (mode 1) or the training path (mode 2).  -> dict of (reference, bound) pairs."""
    z = f64(z)
    gamma, beta, rm, rv = (f64(t) for t in (gamma, beta, rm, rv))
    n = z.shape[0] * z.shape[2]
    mean = z.mean((0, 2)); var = z.var((0, 2), unbiased=False)
    dmean = (n + 4) * U64 * z.abs().mean((0, 2)); dvar = (n + 4) * U64 * 2 * (z * z).mean((0, 2))
    rstd = 1.0 / torch.sqrt(var + EPS)
    zc = z - _bc(mean); zh = zc * _bc(rstd)
    y = zh * _bc(gamma) + _bc(beta)
    dm = U * mean.abs() + dmean
    if mode == 2:
        drs = U + dvar / (2 * (var + EPS))
        d_y = 2 * (_bc(gamma.abs()) * (_bc(rstd) * (_bc(dm) + U * zc.abs()) + zh.abs() * _bc(drs + U)) + U * y.abs())
    else:
        dsc = 3 * U + dvar / (2 * (var + EPS))
        sc = gamma * rstd; sh = beta - mean * sc
        d_y = 2 * ((zh * _bc(gamma)).abs() * _bc(dsc) + _bc(sc.abs() * dm + U * (mean * sc).abs() + U * sh.abs()) + U * y.abs())
    unb = var * n / (n - 1)
    rm2 = KEEP * rm + MOM * mean; rv2 = KEEP * rv + MOM * unb
    d_rm = 2 * (U * (KEEP * rm).abs() + MOM * (2 * U * mean.abs() + dmean) + U * rm2.abs())
    d_rv = 2 * (U * (KEEP * rv).abs() + MOM * (2 * U * unb + dvar * n / (n - 1)) + U * rv2.abs())
    out = dict(y=(y, d_y), rm=(rm2, d_rm), rv=(rv2, d_rv), nbt=(f64(nbt) + 1.0, torch.zeros(1, dtype=torch.float64)))
    if mode == 2:
        out["mean"] = (mean, 2 * dm); out["rstd"] = (rstd, 2 * rstd * (U + dvar / (2 * (var + EPS))))
    return out


def maxpool_fwd_ref(y):
    """ConstantPad1d(1, 0) on both sides at odd L, then torch's MaxPool1d(2): (..., L) -> (..., Lo), any float dtype, NaN propagating."""
    p = F.pad(y, (1, 1)) if y.shape[-1] % 2 else y
    return F.max_pool1d(p.reshape(1, -1, p.shape[-1]), 2, 2).reshape(*y.shape[:-1], -1)


def clf_fwd_ref(x, P, win):
    """The inference head on x (B, C1, L) with P = [w0 (C1, C1), b0, w3 (ncls, C1), b3, w5 (ncls, ncls), b5] -> y (B, ncls, S), d_y."""
    x = f64(x); w0, b0, w3, b3, w5, b5 = (f64(p) for p in P)
    C1, ncls = w0.shape[0], w5.shape[0]
    S = x.shape[-1] // win
    x = x[..., :S * win]
    lin = lambda w, b, v: F.conv1d(v, w[:, :, None], b)
    h = lin(w0, b0, x); t = torch.tanh(h)
    d_t = N.gamma(C1) * lin(w0.abs(), b0.abs(), x.abs()) + 2 * ELU_ULPS * U * t.abs()
    m = F.avg_pool1d(t, win); d_m = F.avg_pool1d(d_t, win) + U * m.abs()
    g = lin(w3, b3, m); mag_g = lin(w3.abs(), b3.abs(), m.abs())
    e = elu64(g)
    d_e = lin(w3.abs(), None, d_m) + N.gamma(C1) * mag_g + 2 * ELU_ULPS * U * e.abs()
    y = lin(w5, b5, e)
    d_y = 2 * (lin(w5.abs(), None, d_e) + N.gamma(ncls) * lin(w5.abs(), b5.abs(), e.abs()))
    return y, d_y


# ---------------------------------------------------------------------------------------------------- judging
def check_bound(name, got, ref, d):
    """|got - ref| <= d element by element, and the same non-finite pattern (NaN where the reference has NaN, the same infinity where it has
    one).  -> worst error / bound over the finite elements.  AssertionError("bound ...") names the worst element."""
    got, ref, d = f64(got), f64(ref), f64(d)
    assert got.shape == ref.shape, f"bound {name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    d = d.expand_as(ref)
    fin = torch.isfinite(ref) & torch.isfinite(d)          # (a bound that an infinite operand made infinite or NaN bounds nothing)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), f"bound {name}: NaN pattern differs ({int(torch.isnan(got).sum())} against {int(torch.isnan(ref).sum())})"
    inf = torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]) and torch.equal(torch.isinf(got), inf), f"bound {name}: infinities differ"
    if not bool(fin.any()):
        return 0.0
    err = (got - ref).abs()[fin]; dd = d[fin]
    bad = err > dd
    ratio = err / dd.clamp_min(1e-300)
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, ratio, torch.zeros_like(ratio))))
        idx = tuple(int(v) for v in torch.nonzero(fin)[i])
        raise AssertionError(f"bound {name}: {int(bad.sum())} of {int(fin.sum())} elements outside; worst at {idx}: error {float(err[i]):.3e} bound {float(dd[i]):.3e}")
    return float(ratio.max())


def check_exact(name, got, want):
    """Bit-for-bit agreement in value (torch.equal), with NaN equal to NaN: the NaN positions are compared first and named when they differ."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f"exact {name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"exact {name}: NaN positions differ: {int(gn.sum())} against {int(wn.sum())}, first at {(gn != wn).nonzero()[0].tolist()}"
    ok = torch.equal(got[~wn], want[~wn])
    assert ok, f"exact {name}: {int((got[~wn] != want[~wn]).sum())} values differ"


def check_pool(name, pooled, y):
    """The pooled stage against torch's pad + MaxPool1d(2) of the stored y: exact, NaN positions included."""
    check_exact(f"pooled stage {name}", pooled, maxpool_fwd_ref(y.detach().cpu()))


def judge_layer(name, c, mode, out):
    """One layer's outputs (fp32 tensors: y, rm, rv, nbt; z in modes 1 and 2; optional pooled, stat = mean | rstd in mode 2) against the staged
    references: mode 0 judges y from the operands; modes 1 and 2 judge z from the operands, then the statistics, y and the running statistics
    from the stored z.  pooled is judged exactly from the stored y.  -> {quantity: worst error / bound}."""
    s, z, d_z = conv_elu_ref(c)
    worst = {}
    if mode == 0:
        y, d_y = bn_eval_ref(z, d_z, c["gamma"], c["beta"], c["rm"], c["rv"])
        worst["y"] = check_bound(f"{name} y", out["y"], y, d_y)
        for k in ("rm", "rv", "nbt"):
            check_exact(f"{name} {k} (eval mode leaves it alone)", out[k], c[k])
    else:
        worst["z"] = check_bound(f"{name} z", out["z"], z, d_z)
        worst["expm1 ulps"] = expm1_branch_ulps(out["z"], s, z, d_z)
        r = bn_train_ref(out["z"], c["gamma"], c["beta"], c["rm"], c["rv"], c["nbt"], mode)
        for k in ("y", "rm", "rv", "nbt"):
            worst[k] = check_bound(f"{name} {k}", out[k], *r[k])
        if mode == 2 and out.get("stat") is not None:
            C = c["Cout"]
            worst["mean"] = check_bound(f"{name} mean", out["stat"][:C], *r["mean"])
            worst["rstd"] = check_bound(f"{name} rstd", out["stat"][C:], *r["rstd"])
    if out.get("pooled") is not None:
        check_pool(name, out["pooled"], out["y"])
    return worst


def expm1_branch_ulps(z_got, s, z, d_z):
    """Worst error of the s <= 0 branch beyond the convolution's share gamma mag, in fp32 ulps of z (the headroom under the 4 ulp granted)."""
    z_got, conv = f64(z_got), d_z - 2 * ELU_ULPS * U * z.abs()
    m = (s <= -conv) & torch.isfinite(z) & torch.isfinite(z_got)
    if not bool(m.any()):
        return 0.0
    over = ((z_got - z).abs() - conv).clamp_min(0)[m] / N.ulp(z[m], "f32")
    return float(over.max())
