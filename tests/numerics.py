"""Float64 references and rounding-aware checks for the HIP kernels (imported by the GPU tests and by test_numerics_model.py; not a conftest).

A kernel that reads 16-bit or fp32 operands, accumulates in fp32 in any order and rounds once at the end can differ from the exact
result only by (a) fp32 summation error, at most gamma_n * sum|a*b| for a reduction of length n, and (b) the one final rounding.  The
references here are evaluated in float64 on the exact values the kernel reads (the operands already rounded to the storage type), so
both sources of error can be bounded without a fitted constant:

  check A (hard):  fp32 outputs   |got - ref| <= gamma_n * mag
                   16-bit outputs got in [RNE(ref - d), RNE(ref + d)], d = gamma_n * mag  (RNE is monotone: whatever fp32 value s with
                                  |s - ref| <= d the kernel rounds, RNE(s) lies in that interval; it holds RNE(ref) and, only where ref
                                  is within d of a rounding midpoint, the other neighbour of ref)
  check B (statistical, 16-bit outputs):
                   share of elements != RNE(ref)  <= 2 * m_emul + 1e-3, m_emul = the same share for torch fp32 on the same operands
                   (CPU, same shape) rounded by `rne`, when there are >= 1e4 elements (below that one legitimate flip at a
                   rounding midpoint is already more than 1e-3 of them: check A alone judges those);
                   mean signed error (towards larger |ref|) in ulps of each element within +-0.02 ulp when there are >= 1e5 elements.

gamma_n = (n + 4) * 2^-24: n products summed in fp32 (the classic (n - 1) u bound of recursive summation, u = 2^-24, holds for every order,
split-K chunks and atomics included) plus up to 4 further fp32 additions or multiplications of the epilogue (bias, per-sample row,
residual, activation slope, a `+=` into an existing fp32 value).  mag = the same operation on |operands| (sum |a*b| per output, plus the
magnitudes of the epilogue terms).

`rne` rounds float64 to bf16 / fp16 ONCE: torch's float64 -> bf16 / fp16 cast goes through float32 and rounds twice
(1 + 2^-8 + 2^-30 becomes 1.0 in bf16, not 1.0078125)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (precision p incl. the implicit bit, smallest normal exponent, largest exponent)
FORMATS = {"bf16": (8, -126, 127), "f16": (11, -14, 15)}
U32 = 2.0 ** -24


def _f64(t):
    return t.detach().to("cpu", torch.float64) if torch.is_tensor(t) else torch.as_tensor(np.asarray(t, dtype=np.float64))


def _quantum(x, fmt):
    """spacing of `fmt` values in the binade of x (subnormal spacing below the normal range): float64 powers of two"""
    p, emin, _ = FORMATS[fmt]
    ax = np.abs(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        _, e = np.frexp(np.where(np.isfinite(ax) & (ax > 0), ax, 1.0))     # ax = m 2^e, m in [0.5, 1): leading bit 2^(e - 1)
    return np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))


def _round(x, fmt, how):
    _, _, emax = FORMATS[fmt]
    x = np.asarray(x, dtype=np.float64)
    q = _quantum(x, fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        r = how(x / q) * q                     # x / q: exact (power-of-two scaling far inside the float64 range)
    big = np.ldexp(1.0, emax + 1)
    r = np.where(np.abs(r) >= big, np.copysign(np.inf, r), r)       # the tie at max + ulp / 2 rounds to even = 2^(emax + 1): inf
    return np.where(np.isfinite(x), r, x)


def rne(x, fmt):
    """float64 -> nearest `fmt` value, ties to even, overflow to +-inf, subnormals kept, NaN stays NaN: one rounding (float64 result)"""
    if fmt == "f32":
        return _f64(x).float().double()        # float64 -> float32 is a single IEEE rounding
    return torch.from_numpy(_round(_f64(x).numpy(), fmt, np.rint))


def rtz(x, fmt):
    """truncation towards zero (a defect model: what a kernel that drops the low bits would store)"""
    return torch.from_numpy(_round(_f64(x).numpy(), fmt, np.trunc))


def ulp(x, fmt):
    """size of the rounding cell of `fmt` that holds x"""
    if fmt == "f32":
        p, emin = 24, -126
        ax = np.abs(_f64(x).numpy())
        _, e = np.frexp(np.where(np.isfinite(ax) & (ax > 0), ax, 1.0))
        return torch.from_numpy(np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1)))
    return torch.from_numpy(_quantum(_f64(x).numpy(), fmt))


def gamma(n):
    return (n + 4) * U32


def to_storage(t, fmt):
    """float64 / float32 tensor -> the exact values a kernel reads from `fmt` storage (float64), correctly rounded"""
    return rne(t, fmt) if fmt != "f32" else _f64(t).float().double()


def torch_dtype(fmt):
    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[fmt]


# ---------------------------------------------------------------- reference operations (any float dtype, NCL layout)
def conv1d_fwd(x, w, b=None, stride=1, pad_l=0, pad_r=0, row=None, resid=None, slope=None):
    """Conv1d(x; w) + bias[c] + row[b, c] + resid[b, c, l], then LeakyReLU(slope) when given"""
    y = F.conv1d(F.pad(x, (pad_l, pad_r)), w, None, stride=stride)
    if b is not None:
        y = y + b[:, None]
    if row is not None:
        y = y + row[:, :, None]
    if resid is not None:
        y = y + resid
    if slope is not None:
        y = F.leaky_relu(y, slope)
    return y


def _conv_grads(x, w, dy, stride, pad_l, pad_r, want):
    x = x.detach().clone().requires_grad_(want == "x"); w = w.detach().clone().requires_grad_(want == "w")
    y = F.conv1d(F.pad(x, (pad_l, pad_r)), w, None, stride=stride)
    (g,) = torch.autograd.grad(y, x if want == "x" else w, dy)
    return g


def conv1d_dgrad(dy, w, L, stride=1, pad_l=0, pad_r=0, resid=None):
    """d(conv)/dx for an input of length L (+ resid[b, c, l])"""
    B, Cin = dy.shape[0], w.shape[1]
    dx = _conv_grads(torch.zeros(B, Cin, L, dtype=dy.dtype), w, dy, stride, pad_l, pad_r, "x")
    return dx + resid if resid is not None else dx


def conv1d_wgrad(x, dy, K, stride=1, pad_l=0, pad_r=0, acc=None):
    """d(conv)/dw as (Cout, Cin, K) (+ acc: the dW the kernel accumulates into)"""
    w0 = torch.zeros(dy.shape[1], x.shape[1], K, dtype=x.dtype)
    dw = _conv_grads(x, w0, dy, stride, pad_l, pad_r, "w")
    return dw + acc if acc is not None else dw


def bias_grad(dy, acc=None):
    """column sums of dy over (batch, length) (+ acc)"""
    db = dy.sum(dim=(0, 2)) if dy.dim() == 3 else dy.sum(dim=0)
    return db + acc if acc is not None else db


def linear_fwd(x, w, b=None):
    y = x @ w.t()
    return y + b if b is not None else y


def linear_dgrad(dy, w):
    return dy @ w


def linear_wgrad(x, dy, acc=None):
    dw = dy.t() @ x
    return dw + acc if acc is not None else dw


def _abs(v):
    return v.abs() if torch.is_tensor(v) else v


def evaluate(fn, *args, **kw):
    """(ref, mag, emul): fn in float64 on the exact operand values; fn on |operands| (activation dropped: |act(s)| <= |s| and the
    activation shrinks errors); fn in float32 on the same values (the CPU emulation behind m_emul).  Tensor args must hold values
    already representable in the storage type."""
    a64 = [_f64(a) if torch.is_tensor(a) else a for a in args]
    k64 = {k: (_f64(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    ref = fn(*a64, **k64)
    kmag = {k: _abs(v) for k, v in k64.items() if k != "slope"}
    mag = fn(*[_abs(a) for a in a64], **kmag)
    emul = fn(*[a.float() if torch.is_tensor(a) else a for a in a64], **{k: (v.float() if torch.is_tensor(v) else v) for k, v in k64.items()})
    return ref, mag, emul


# ---------------------------------------------------------------- checks
def _nonfinite_agree(got, ref):
    """where ref is NaN got must be NaN; where ref is +-inf got must be the same inf; returns the mask of finite refs"""
    fin = torch.isfinite(ref)
    nan_r = torch.isnan(ref)
    bad_nan = nan_r & ~torch.isnan(got)
    inf_r = torch.isinf(ref)
    bad_inf = inf_r & (got != ref)
    return fin, bad_nan, bad_inf


def check_a(got, ref, mag, n, fmt):
    """hard bound; returns (number of violations, worst |error| / allowed error, index of the worst element)"""
    got, ref, mag = _f64(got), _f64(ref), _f64(mag)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    fin, bad_nan, bad_inf = _nonfinite_agree(got, ref)
    d = gamma(n) * torch.where(fin, mag, torch.zeros_like(mag))
    r = torch.where(fin, ref, torch.zeros_like(ref))
    if fmt == "f32":
        lo, hi = r - d, r + d
        allow = d
    else:
        lo, hi = rne(r - d, fmt), rne(r + d, fmt)
        allow = 0.5 * ulp(r, fmt) + d            # (for the report: the interval above is this bound, cut to representable values)
    inside = (got >= lo) & (got <= hi)
    bad = (fin & ~inside) | bad_nan | bad_inf
    err = torch.where(fin, (got - r).abs(), torch.zeros_like(r))
    if fmt != "f32":
        err = torch.where(_same(got, rne(r, fmt)) & ~torch.isfinite(got), torch.zeros_like(err), err)   # correctly rounded to +-inf
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allow)
    ratio = torch.where(bad_nan | bad_inf, torch.full_like(ratio, math.inf), ratio)
    i = int(torch.argmax(torch.nan_to_num(ratio, nan=math.inf, posinf=1e300)))
    return int(bad.sum()), float(ratio.reshape(-1)[i]), i


def _same(a, b):
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def mismatch_share(got, ref, fmt):
    got, ref = _f64(got), _f64(ref)
    return float((~_same(got, rne(ref, fmt))).double().mean())


def mean_signed_ulp(got, ref, fmt):
    """mean over finite, non-zero refs of (got - ref) * sign(ref) / ulp(ref): ~0 for round-to-nearest, -0.5 for truncation"""
    got, ref = _f64(got), _f64(ref)
    m = torch.isfinite(ref) & (ref != 0) & torch.isfinite(got)
    if not bool(m.any()):
        return 0.0, 0
    e = (got[m] - ref[m]) * torch.sign(ref[m]) / ulp(ref[m], fmt)
    return float(e.mean()), int(m.sum())


def check(got, ref, mag, n, fmt, emul=None, route="", report=True, min_stat=100_000, min_share=10_000):
    """check A (always) and, for 16-bit outputs with an emulation, check B.  Raises AssertionError with the statistics; returns them."""
    got = _f64(got); ref = _f64(ref)
    nbad, worst, iw = check_a(got, ref, mag, n, fmt)
    st = dict(route=route, fmt=fmt, n_elem=ref.numel(), n_red=n, bad_a=nbad, worst=worst)
    msgs = []
    if nbad:
        msgs.append(f"check A: {nbad} of {ref.numel()} outside the bound (worst at flat index {iw}: got {got.reshape(-1)[iw].item()!r}, "
                    f"ref {ref.reshape(-1)[iw].item()!r}, mag {_f64(mag).reshape(-1)[iw].item():.4g}, {worst:.3g} x its bound)")
    if fmt != "f32":
        share = mismatch_share(got, ref, fmt)
        mu, cnt = mean_signed_ulp(got, ref, fmt)
        st.update(mismatch=share, mean_ulp=mu)
        if emul is not None:
            m_emul = mismatch_share(rne(emul, fmt), ref, fmt)
            st["m_emul"] = m_emul
            if ref.numel() >= min_share and share > 2 * m_emul + 1e-3:
                msgs.append(f"check B: {share:.3e} of the elements differ from RNE(ref), bound 2 x {m_emul:.3e} + 1e-3")
        if cnt >= min_stat and abs(mu) > 0.02:
            msgs.append(f"check B: mean signed error {mu:+.4f} ulp over {cnt} elements (bound +-0.02)")
    if report:
        print(format_report(st))
    assert not msgs, f"{route} [{fmt}]: " + "; ".join(msgs)
    return st


def format_report(st):
    s = f"[numerics] {st['route']:<44s} {st['fmt']:>4s} n={st['n_elem']:>9d} red={st['n_red']:>6d} worst={st['worst']:.3f}xbound"
    if "mismatch" in st:
        s += f" mismatch={st['mismatch']:.2e}"
        if "m_emul" in st:
            s += f" (m_emul {st['m_emul']:.2e})"
        s += f" mean={st['mean_ulp']:+.4f}ulp"
    return s


def check_b(got, ref, emul, fmt, route="", report=True, min_stat=100_000, min_share=10_000):
    """check B alone, for 16-bit outputs whose computation has no derived hard bound (the GroupNorm data gradient): mismatch share against
    the fp32 CPU emulation's and the mean signed ulp error, with the same thresholds as `check`"""
    got, ref = _f64(got), _f64(ref)
    share = mismatch_share(got, ref, fmt)
    m_emul = mismatch_share(rne(emul, fmt), ref, fmt)
    mu, cnt = mean_signed_ulp(got, ref, fmt)
    st = dict(route=route, fmt=fmt, n_elem=ref.numel(), n_red=0, bad_a=0, worst=float("nan"), mismatch=share, m_emul=m_emul, mean_ulp=mu)
    msgs = []
    if ref.numel() >= min_share and share > 2 * m_emul + 1e-3:
        msgs.append(f"check B: {share:.3e} of the elements differ from RNE(ref), bound 2 x {m_emul:.3e} + 1e-3")
    if cnt >= min_stat and abs(mu) > 0.02:
        msgs.append(f"check B: mean signed error {mu:+.4f} ulp over {cnt} elements (bound +-0.02)")
    if report:
        print(format_report(st))
    assert not msgs, f"{route} [{fmt}]: " + "; ".join(msgs)
    return st
