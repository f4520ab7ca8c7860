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


# ---------------------------------------------------------------- attention (one head; q, k, v, dO, O as (B, T, C), P, dS as (B, T, T))
# Staged references of softmax(alpha q k^T) v and its backward.  The kernels (csrc/attn.hip, and the GEMM + softmax composition of
# ops.hip / elementwise.hip) store their 16-bit intermediates P and dS in caller-owned buffers and the later stages read those very
# values, so each stage is judged on the operands the next one read: the products by check A / B as the convs are, the two row
# operations (softmax, dS) by the bounds derived below.
#
# Relative error of exp on the device (the one figure of softmax_bound that this repository's source does not give):
#   __expf (attn.hip) compiles to v_mul_f32 by fp32(log2 e), then v_exp_f32 (read from the gfx950 assembly).  AMD's public ISA
#          reference guides ("Vega" Instruction Set Architecture and its GCN3 / CDNA relatives, VOP1 opcode table, V_EXP_F32:
#          "Base2 exponent function. 1ULP accuracy, denormals are flushed") state 1 ulp (2u).  The constant's and the product's
#          roundings move the argument by up to 2u |x| log2(e), the result by a relative 2u |x|; below x = -87.4 the result is
#          under 2^-126 and softmax_bound's floor takes over, so |x| <= 88 bounds the term: 2u + 176u.
#   expf   (elementwise.hip) is the device library's routine, 1 ulp (2u) in the HIP math-API tables.
# These are stated accuracies, taken as they are; a measured figure would enter doubled.
E_EXP_FUSED, E_EXP_COMPOSITION = 178 * U32, 2 * U32


def attn_alpha(C):
    """the exact 1 / sqrt(C); the kernels use fp32(1 / sqrtf(C)): that rounding and the fp32 multiplication by it are two of the four
    spare roundings of gamma_n (both exact when C is a power of four)"""
    return 1.0 / math.sqrt(C)


def attn_logits(q, k, alpha):
    return alpha * (q @ k.transpose(1, 2))


def attn_softmax(s):
    return torch.softmax(s, dim=-1)


def attn_out(p, v):
    return p @ v


def attn_dprobs(do, v):
    return do @ v.transpose(1, 2)


def attn_dscores(p, dp, alpha):
    """dS = alpha p (dP - sum_s dP p): the form the kernels evaluate (alpha p first; 0 x inf = NaN as there)"""
    return (alpha * p) * (dp - (dp * p).sum(-1, keepdim=True))


def attn_dq(ds, k):
    return ds @ k


def attn_dk(ds, q):
    return ds.transpose(1, 2) @ q


def attn_dv(p, do):
    return p.transpose(1, 2) @ do


def softmax_bound(s_ref, s_mag, C, e_exp):
    """(p, d): the float64 softmax of the float64 logits and the absolute bound d = p r + f of a kernel that forms fp32 logits s' with
    |s' - s| <= gamma(C) s_mag (s_mag = alpha sum|q||k|), then e = exp'(s' - m) with the row maximum m, S = fp32 sum of the T e's in
    any order, p' = e (1 / S), and rounds once.  Sources of relative error:
      logits  p' = e^(s + ds) / sum e^(s + ds), |ds| <= D = max_row gamma(C) s_mag, lies within e^(+-2D) of p:   expm1(2 D)
      s' - m  one fp32 rounding: absolute error u |x| of the argument x = s - max_row s (|x'| <= |x| + 2D):        u (|x| + 2D)
      exp'    relative error e_exp (E_EXP_FUSED / E_EXP_COMPOSITION above) of every e: the numerator carries
              e_exp + u (|x| + 2D), the denominator the p-weighted mean of the same terms (the issue's r writes
              e_exp once; a ratio of two inexact quantities carries it twice):                                    sum_s p_s (...)
      sum     T positive terms in fp32, any order (gamma carries 4 spare u: 1 / S and e * (1 / S) are two):       gamma(T)
      4u      slack for the second-order terms of all of the above
    r = expm1(2D) + (e_exp + u (|x| + 2D)) + sum_s p_s (e_exp + u (|x_s| + 2D)) + gamma(T) + 4u.
    f = 2^-126: an e or a product below the smallest normal fp32 number may be flushed to zero, an absolute error of less than
    2^-126 (S >= 1 as the row maximum contributes e = 1, so 1 / S <= 1)."""
    s_ref, s_mag = _f64(s_ref), _f64(s_mag)
    T = s_ref.shape[-1]
    p = torch.softmax(s_ref, dim=-1)
    D = (gamma(C) * s_mag).amax(-1, keepdim=True)
    x = (s_ref - s_ref.amax(-1, keepdim=True)).abs()
    ex = e_exp + U32 * (x + 2 * D)
    r = torch.expm1(2 * D) + ex + (p * ex).sum(-1, keepdim=True) + gamma(T) + 4 * U32
    return p, p * r + 2.0 ** -126


def dscores_bound(p, dp_ref, dp_mag, C, alpha):
    """(dS, d): float64 dS = alpha p (dP - dl), dl = sum_s p_s dP_s, from the STORED probabilities p and the float64 dP = dO V^T, and
    the absolute bound d of a kernel that holds dP' in fp32 with |dP' - dP| <= e_dP = gamma(C) dp_mag (dp_mag = sum|dO||V|), forms
    the row dot dl' in fp32 in any order, |dl' - dl| <= e_dl = sum_s p_s e_dP_s + gamma(T) sum_s |dP_s| p_s, and evaluates
    alpha' * p * (dP' - dl') with alpha' = fp32(alpha) (relative u), the subtraction (u (|dP| + |dl|)) and two products (2u), then
    rounds once: d = alpha p (e_dP + e_dl + 4u (|dP| + |dl|)) + 2^-126.  Absolute, so the cancellation in dP - dl needs no special
    case; the floor allows a product below the smallest normal fp32 number to be flushed to zero, as in softmax_bound."""
    p, dp_ref, dp_mag = _f64(p), _f64(dp_ref), _f64(dp_mag)
    T = p.shape[-1]
    dl = (dp_ref * p).sum(-1, keepdim=True)
    e_dp = gamma(C) * dp_mag
    e_dl = (p * e_dp).sum(-1, keepdim=True) + gamma(T) * (dp_ref.abs() * p).sum(-1, keepdim=True)
    ref = (alpha * p) * (dp_ref - dl)
    d = alpha * p * (e_dp + e_dl + 4 * U32 * (dp_ref.abs() + dl.abs())) + 2.0 ** -126
    return ref, d


def _check_row_op(got, ref, d, fmt, emul, route, report, f16_subnormal_exact=False):
    """P and dS: check A with the derived absolute bound d on every element; check B on the elements of magnitude >= 2^-120 whose
    bound d is at most a quarter ulp.  Below 2^-120 the fp32 arithmetic of the row operation is in or next to its subnormal range
    (flush-to-zero is allowed by the floor of the bound, and one fp32 subnormal rounding is many bf16-subnormal ulps).  Check B
    presumes that the final rounding dominates the error; where the derived fp32 error exceeds the rounding step (the cancellation
    dP - dl of a sharp row, logits whose own error is above an ulp of P) an error of many ulps is legitimate and the mean of such a
    heavy-tailed quantity says nothing.
    f16_subnormal_exact (P in fp16): every element whose RNE(ref) is a non-zero fp16 subnormal must EQUAL RNE(ref), unless ref lies
    within d of a rounding midpoint (RNE(ref - d) != RNE(ref + d)); a kernel that flushes fp16 subnormals fails here by name."""
    got, ref, d = _f64(got), _f64(ref), _f64(d)
    st = check(got, ref, d / gamma(0), 0, fmt, route=route, report=False, min_stat=math.inf)
    msgs = []
    if fmt != "f32":
        m = (ref.abs() >= 2.0 ** -120) & (d <= 0.25 * ulp(ref, fmt))
        try:
            stb = check_b(got[m], ref[m], _f64(emul)[m], fmt, route=route, report=False)
            st.update(mismatch=stb["mismatch"], m_emul=stb["m_emul"], mean_ulp=stb["mean_ulp"])
        except AssertionError as e:
            msgs.append(str(e))
    if f16_subnormal_exact and fmt == "f16":
        r16 = rne(ref, "f16")
        sub = (r16 != 0) & (r16.abs() < 2.0 ** -14) & (rne(ref - d, "f16") == rne(ref + d, "f16"))
        wrong = sub & (got != r16)
        st["f16_subnormal"] = int(sub.sum())
        if bool(wrong.any()):
            msgs.append(f"{route} [f16]: {int(wrong.sum())} of {int(sub.sum())} fp16-subnormal elements differ from RNE(ref)")
    if report:
        print(format_report(st) + (f" f16-subnormal={st['f16_subnormal']} all = RNE(ref)" if "f16_subnormal" in st and not msgs else ""))
    assert not msgs, "; ".join(msgs)
    return st


def attention_stages(q, k, v, do, got, fmt, e_exp, route="", report=True, shared=None):
    """Judge every stage of one attention forward + backward.  q, k, v, do: float64 (B, T, C) holding storage values; got: dict of
    float64 tensors read back from the kernel under test -- P, O, dS, dQ, dK, dV, and on the composition path S and dP (the fp32
    scratch buffers).  Stages missing from `got` are skipped.  Returns (failures: {stage: message}, stats: {stage: dict}); nothing is
    raised, so that a caller can demand that a NAMED stage fails (the defect models) or that none does.  `shared` caches the
    references that depend on the operands only (logits, softmax bound, dP) between calls with identical operands."""
    (B, Tq, C), T = q.shape, k.shape[1]          # Tq query rows (a caller may judge a part of them), T keys
    alpha = attn_alpha(C)
    sh = shared if shared is not None else {}
    if "s" not in sh:
        sh["s"] = evaluate(attn_logits, q, k, alpha)
        sh["p"] = softmax_bound(sh["s"][0], sh["s"][1], C, e_exp)
        sh["dp"] = evaluate(attn_dprobs, do, v)
    (s_ref, s_mag, s_emul), (p_ref, p_d), (dp_ref, dp_mag, dp_emul) = sh["s"], sh["p"], sh["dp"]
    fails, stats = {}, {}

    def run(stage, fn):
        try:
            stats[stage] = fn()
        except AssertionError as e:
            fails[stage] = str(e)

    if "S" in got:
        run("S", lambda: check(got["S"], s_ref, s_mag, C, "f32", route=f"{route} S = alpha q k^T", report=report))
    if "P" in got:
        emul_p = torch.softmax(s_emul, dim=-1) if fmt != "f32" else None       # fp32-accumulated logits, fp32 softmax
        run("P", lambda: _check_row_op(got["P"], p_ref, p_d, fmt, emul_p, f"{route} P = softmax(S)", report, f16_subnormal_exact=True))
        P = _f64(got["P"])
        if "O" in got:
            r, m, e = evaluate(attn_out, P, v)
            run("O", lambda: check(got["O"], r, m, T, fmt, emul=e, route=f"{route} O = P_stored V", report=report))
        if "dP" in got:
            run("dP", lambda: check(got["dP"], dp_ref, dp_mag, C, "f32", route=f"{route} dP = dO V^T", report=report))
        if "dS" in got:
            ds_ref, ds_d = dscores_bound(P, dp_ref, dp_mag, C, alpha)
            emul_ds = attn_dscores(P.float(), dp_emul, float(np.float32(alpha))) if fmt != "f32" else None
            run("dS", lambda: _check_row_op(got["dS"], ds_ref, ds_d, fmt, emul_ds, f"{route} dS = alpha P (dP - dl)", report))
        if "dV" in got:
            r, m, e = evaluate(attn_dv, P, do)
            run("dV", lambda: check(got["dV"], r, m, Tq, fmt, emul=e, route=f"{route} dV = P_stored^T dO", report=report))
    if "dS" in got:
        dS = _f64(got["dS"])
        if "dQ" in got:
            r, m, e = evaluate(attn_dq, dS, k)
            run("dQ", lambda: check(got["dQ"], r, m, T, fmt, emul=e, route=f"{route} dQ = dS_stored K", report=report))
        if "dK" in got:
            r, m, e = evaluate(attn_dk, dS, q)
            run("dK", lambda: check(got["dK"], r, m, Tq, fmt, emul=e, route=f"{route} dK = dS_stored^T Q", report=report))
    return fails, stats


def attention_nonfinite(q, k, v, do, got, route="", report=True):
    """Non-finite operands (NaN / inf somewhere in q, k, v, dO): the non-finite PATTERN of every stage in `got` (P, O, dS, dQ, dK, dV)
    must be that of the float64 reference evaluated end to end on the same operands, and the reference pattern must not be empty
    (a case that poisons nothing tests nothing).  Returns {stage: message} of the stages whose pattern differs."""
    a = attn_alpha(q.shape[-1])
    q, k, v, do = _f64(q), _f64(k), _f64(v), _f64(do)
    P = attn_softmax(attn_logits(q, k, a)); dS = attn_dscores(P, attn_dprobs(do, v), a)
    ref = dict(P=P, O=attn_out(P, v), dS=dS, dQ=attn_dq(dS, k), dK=attn_dk(dS, q), dV=attn_dv(P, do))
    fails = {}
    for s, r in ref.items():
        if s not in got:
            continue
        g = _f64(got[s])
        nr, ng = ~torch.isfinite(r), ~torch.isfinite(g)
        assert bool(nr.any()), f"{route} {s}: the reference has no non-finite element"
        bad = nr != ng
        if bool(bad.any()):
            fails[s] = (f"{route} {s}: non-finite pattern differs in {int(bad.sum())} of {r.numel()} elements "
                        f"(kernel {int(ng.sum())}, reference {int(nr.sum())} non-finite)")
        elif report:
            print(f"[nonfinite] {route} {s}: {int(nr.sum())} non-finite elements, same pattern as the reference")
    return fails


# ---------------------------------------------------------------- GroupNorm (NCL layout; any float dtype: float64 reference, float32 emulation)
# y = act(xhat gamma + beta), xhat = (x - mean) rstd per (sample, group), rstd = 1 / sqrt(var + eps) with the biased variance; then the
# resample the kernels fuse: 1 = avgpool2 of the OUTPUT (pairs of rows, after the activation), 2 = nearest x2.  xr is the same resample
# of the INPUT (the residual branch of a ResBlock).  The backward takes dy at the resampled length and an optional addend dxr that
# is a gradient arriving at xr's length, resampled back the same way and added to dx.
def gn_stats(x, G, eps):
    """(mean, var, rstd), each (B, G), in x's dtype"""
    B = x.shape[0]
    xg = x.reshape(B, G, -1)
    mean = xg.mean(-1)
    var = ((xg - mean[:, :, None]) ** 2).mean(-1)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def gn_resample(t, resample):
    if resample == 1:
        return 0.5 * (t[:, :, 0::2] + t[:, :, 1::2])
    if resample == 2:
        return t.repeat_interleave(2, dim=2)
    return t


def gn_fwd(x, G, gamma, beta, eps=1e-6, silu=False, resample=0, torch_norm=False):
    """torch_norm: z from torch.nn.functional.group_norm -- the fp32 emulation behind check B's m_emul (torch's own kernel, whose fp32
    arithmetic on uncentred values is what an fp32 implementation is measured against); otherwise the centred formula, for float64"""
    B, C, L = x.shape
    if torch_norm:
        z = F.group_norm(x, G, gamma, beta, eps=eps)
    else:
        mean, _var, rstd = gn_stats(x, G, eps)
        rep = lambda t: t.repeat_interleave(C // G, dim=1)[:, :, None]
        z = (x - rep(mean)) * rep(rstd) * gamma[:, None] + beta[:, None]
    return gn_resample(F.silu(z) if silu else z, resample)


def gn_xr(x, resample):
    """the resampled copy of the input that the forward writes beside y (resample 1 and 2)"""
    return gn_resample(x, resample)


def gn_bwd(x, G, gamma, beta, dy, eps=1e-6, silu=False, resample=0, dxr=None, torch_norm=False):
    """(dx, dgamma, dbeta) of sum(gn_fwd(x) dy) [+ sum(gn_xr(x) dxr)] by autograd in the dtype of x"""
    xr = x.detach().clone().requires_grad_(True); gr = gamma.detach().clone().requires_grad_(True); br = beta.detach().clone().requires_grad_(True)
    s = (gn_fwd(xr, G, gr, br, eps, silu, resample, torch_norm) * dy).sum()
    if dxr is not None:
        s = s + (gn_xr(xr, resample) * dxr).sum()
    s.backward()
    return xr.grad, gr.grad, br.grad


# ---------------------------------------------------------------- BatchNorm1d + LeakyReLU and the fused discriminator tail / head
# Row-major operands: x, y, dy, dx as (rows, C) (rows = B L of the NLC buffers); per-channel vectors as (C,).  The references are float64;
# the bounds are those derived in the docstring of tests/test_gpu_batchnorm_rounding.py, evaluated from the reference alone.
U64 = 2.0 ** -53


_gam = gamma          # (the BatchNorm functions below take a parameter called gamma)


def gamma64(n):
    return (n + 4) * U64


def bn_stats(x, eps, rmean=None, rvar=None, nbt=0.0, momentum=0.1, repeats=1):
    """dict(mean, var (biased), rstd, rmean, rvar, nbt): per channel over all rows, and the running statistics after `repeats` momentum
    updates with the unbiased variance (n - 1 >= 1 in the divisor, as torch's BatchNorm1d; one row: the biased value)"""
    x = _f64(x)
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    out = dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps), n=n)
    if rmean is not None:
        rm, rv = _f64(rmean).clone(), _f64(rvar).clone()
        ub = var * n / max(n - 1, 1)
        for _ in range(repeats):
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * ub
        out.update(rmean=rm, rvar=rv, nbt=float(nbt) + repeats)
    return out


def bn_stats_from_sums(S1, S2, n, eps):
    """the same from column sums (the from-parts fold: S1, S2 are the exact sums of the fp32 partials)"""
    mean = _f64(S1) / n
    var = torch.clamp(_f64(S2) / n - mean * mean, min=0.0)
    return dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps), n=n)


def lrelu(z, slope):
    return torch.where(z > 0, z, slope * z)


def bn_z(x, gamma, beta, st):
    xhat = (_f64(x) - st["mean"]) * st["rstd"]
    return xhat, xhat * _f64(gamma) + _f64(beta)


def bn_lrelu_fwd(x, gamma, beta, st, slope):
    """y = lrelu(gamma (x - mean) rstd + beta); gamma None: plain LeakyReLU"""
    if gamma is None:
        return lrelu(_f64(x), slope)
    return lrelu(bn_z(x, gamma, beta, st)[1], slope)


def bn_lrelu_bwd(x, gamma, beta, st, dy, slope, mask=None):
    """(dx, dgamma, dbeta, S1, S2) for an upstream gradient dy of the ACTIVATED output; the mask is z > 0 unless given"""
    xhat, z = bn_z(x, gamma, beta, st)
    m = (z > 0) if mask is None else mask
    dz = torch.where(m, _f64(dy), slope * _f64(dy))
    S1, S2 = dz.sum(0), (dz * xhat).sum(0)
    n = x.shape[0]
    dx = _f64(gamma) * st["rstd"] * (dz - S1 / n - xhat * (S2 / n))
    return dx, S2, S1, S1, S2


def bn_stat_bounds(x, st, n_p, block_round, eps):
    """(e_mean absolute, e_rstd relative) of one-pass statistics about zero: per-thread fp32 sums of x and x^2 over at most n_p elements, fp64
    across threads, one fp32 rounding of each block partial when block_round, fp64 fold, two casts"""
    x = _f64(x)
    u = U32 if block_round else 0.0
    mean, var = st["mean"], st["var"]
    e_mean = (_gam(n_p) + u) * x.abs().mean(0) + U32 * mean.abs()
    e_var = (_gam(n_p + 2) + u) * (var + mean ** 2) + 2 * mean.abs() * e_mean
    return e_mean, e_var / (2 * (var + eps)) + 4 * U32


def bn_fwd_bound(x, gamma, beta, st, e_mean, e_rstd, slope):
    """(z, y, d): the float64 pre-activation and output and the absolute bound d of the output (and of z: LeakyReLU is continuous with slope
    <= 1): d = |gamma| (|xhat| e_rstd + rstd e_mean) + 3u |gamma| rstd (|x| + |mean|) + 4u |z| + u |y|"""
    x = _f64(x); ga = _f64(gamma).abs()
    xhat, z = bn_z(x, gamma, beta, st)
    y = lrelu(z, slope)
    d = ga * (xhat.abs() * e_rstd + st["rstd"] * e_mean) + 3 * U32 * ga * st["rstd"] * (x.abs() + st["mean"].abs()) + 4 * U32 * z.abs() + U32 * y.abs()
    return z, y, d


def bn_bwd_bounds(x, gamma, beta, st, e_mean, e_rstd, da, slope, d_z, da_mag=None, k_da=0, dgamma0=None, dbeta0=None):
    """References and bounds of the backward of lrelu(bn(x)) for an upstream gradient da (float64 reference) that the kernel holds to within
    k_da u da_mag (BatchNorm: da = dy exactly, k_da = 0; the fused tail recomputes da with three fp32 roundings).  d_z is the bound of the
    kernel's own z; U = {|z| <= d_z} is the set where a correct kernel may take either LeakyReLU branch.  Returns a dict:
      U, share            the set (with the elements whose z is NaN: a poisoned channel) and its share of the elements
      dx, dx_alt, b_dx    reference with the mask z > 0, with the opposite mask ON U (same S1, S2), the bound (valid for either on U)
      S1, S2, bS1, bS2    the column sums and their bounds (U widening included)
      dbeta, dgamma, b_dbeta, b_dgamma   = S1 + dbeta0, S2 + dgamma0 and their bounds (the start value joins the sum of magnitudes)"""
    x, da = _f64(x), _f64(da)
    n = x.shape[0]
    ga = _f64(gamma)
    mean, rstd = st["mean"], st["rstd"]
    xhat, z = bn_z(x, gamma, beta, st)
    U = (z.abs() <= d_z) | torch.isnan(z)        # (a NaN z compares false both ways: `z > 0` and `z <= 0` pick different branches)
    m = z > 0
    mag = da.abs() if da_mag is None else _f64(da_mag)
    dz = torch.where(m, da, slope * da)
    dz_alt = torch.where(m ^ U, da, slope * da)
    dzm = torch.where(m | U, mag, slope * mag)                   # bound of |dz'| whichever branch is taken on U
    e_dz = k_da * U32 * dzm
    wid = torch.where(U, (1 - slope) * mag, torch.zeros_like(mag))
    dxh = xhat.abs() * e_rstd + rstd * e_mean + 2 * U32 * rstd * (x.abs() + mean.abs())
    S1, S2 = dz.sum(0), (dz * xhat).sum(0)
    bS1 = _gam(n + k_da) * dzm.sum(0) + wid.sum(0)
    bS2 = _gam(n + k_da + 2) * (dzm * xhat.abs()).sum(0) + (dzm * dxh).sum(0) + (wid * xhat.abs()).sum(0)
    db0 = torch.zeros_like(S1) if dbeta0 is None else _f64(dbeta0)
    dg0 = torch.zeros_like(S2) if dgamma0 is None else _f64(dgamma0)
    sc = (ga * rstd).abs()
    k1, k2 = S1 / n, S2 / n

    def dx_of(d):
        return ga * rstd * (d - k1 - xhat * k2)

    dx, dx_alt = dx_of(dz), dx_of(dz_alt)
    dxa = torch.maximum(dx.abs(), dx_alt.abs())
    b_dx = sc * (bS1 / n + xhat.abs() * bS2 / n + k2.abs() * dxh + e_dz) + (e_rstd + 3 * U32) * dxa + 6 * U32 * sc * (dzm + k1.abs() + (xhat * k2).abs())
    return dict(U=U, share=float(U.double().mean()), xhat=xhat, z=z, dx=dx, dx_alt=dx_alt, b_dx=b_dx, S1=S1, S2=S2, bS1=bS1, bS2=bS2,
                dbeta=S1 + db0, dgamma=S2 + dg0, b_dbeta=bS1 + _gam(n + k_da) * db0.abs(), b_dgamma=bS2 + _gam(n + k_da + 2) * dg0.abs(),
                dzm=dzm, dz=dz)


def _within(got, ref, d, fmt):
    """element-wise: got inside [ref - d, ref + d] (16-bit outputs: inside [RNE(ref - d), RNE(ref + d)]); a NaN reference wants a NaN, an
    infinite one the same infinity.  Returns (inside, |error| / allowed error)"""
    got, ref, d = _f64(got), _f64(ref), _f64(d)
    fin = torch.isfinite(ref) & torch.isfinite(d)
    r = torch.where(fin, ref, torch.zeros_like(ref)); dd = torch.where(fin, d, torch.zeros_like(d))
    if fmt == "f32":
        inside = (got >= r - dd) & (got <= r + dd); allow = dd
    else:
        inside = (got >= rne(r - dd, fmt)) & (got <= rne(r + dd, fmt)); allow = 0.5 * ulp(r, fmt) + dd
    nonfin = torch.where(torch.isnan(ref) | torch.isnan(d), torch.isnan(got), got == ref)
    err = (got - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allow)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    ok = torch.where(fin, inside, nonfin)
    return ok, torch.where(fin, ratio, torch.where(nonfin, torch.zeros_like(ratio), torch.full_like(ratio, math.inf)))


def check_abs(got, ref, d, fmt, route="", alt=None, report=True):
    """check A with a derived absolute bound d per element.  alt = (ref2, mask): on `mask` an element also passes when it is within d of ref2
    (the mask-uncertain set of a LeakyReLU backward).  Prints one [numerics] line; raises AssertionError with the worst element."""
    got, ref, d = _f64(got), _f64(ref), _f64(d)
    assert got.shape == ref.shape == d.shape, (got.shape, ref.shape, d.shape)
    ok, ratio = _within(got, ref, d, fmt)
    if alt is not None:
        ok2, ratio2 = _within(got, alt[0], d, fmt)
        ok = ok | (alt[1] & ok2); ratio = torch.where(alt[1], torch.minimum(ratio, ratio2), ratio)
    nbad = int((~ok).sum())
    i = int(torch.argmax(torch.nan_to_num(ratio, posinf=1e300)))
    worst = float(ratio.reshape(-1)[i])
    st = dict(route=route, fmt=fmt, n_elem=ref.numel(), n_red=0, bad_a=nbad, worst=worst)
    if fmt != "f32":
        mu, _cnt = mean_signed_ulp(got, ref, fmt)
        st.update(mismatch=mismatch_share(got, ref, fmt), mean_ulp=mu)
    if report:
        print(format_report(st))
    assert nbad == 0, (f"{route} [{fmt}]: check A: {nbad} of {ref.numel()} outside the bound (worst at flat index {i}: got {got.reshape(-1)[i].item()!r}, "
                       f"ref {ref.reshape(-1)[i].item()!r}, bound {d.reshape(-1)[i].item():.4g}, {worst:.3g} x its bound)")
    return st


# fused tail: y (B, L, C); w3 (3, C) fp32 master weights; logits / dl (B, L)
def _shift_rows(a, t):
    """a[:, l + t] with zeros outside the sample (a: (B, L, ...))"""
    out = torch.zeros_like(a)
    L = a.shape[1]
    if t == 0:
        return a.clone()
    if t > 0:
        out[:, :L - t] = a[:, t:]
    else:
        out[:, -t:] = a[:, :L + t]
    return out


def tail_logits(y, gamma, beta, st, w3, bias, slope, a=None):
    """logits[b, l] = bias + sum_t sum_c w3[t, c] a[b, l + t - 1, c], a = lrelu(bn(y)) (or the `a` given: the magnitudes of the bound)"""
    y, w3 = _f64(y), _f64(w3)
    if a is None:
        a = bn_lrelu_fwd(y, gamma, beta, st, slope)
    out = sum((_shift_rows(a, t - 1) * w3[t]).sum(-1) for t in range(3))
    return out + (float(bias) if bias is not None else 0.0)


def tail_da(dl, w3):
    """da[b, l, c] = dl[b, l + 1] w0[c] + dl[b, l] w1[c] + dl[b, l - 1] w2[c]: the data gradient of the one-channel conv"""
    dl, w3 = _f64(dl), _f64(w3)
    return sum(_shift_rows(dl, 1 - t)[:, :, None] * w3[t] for t in range(3))


def tail_bwd(y, gamma, beta, st, w3, slope, dl, mask=None):
    """(dy, dgamma, dbeta, dw3, dbias); statistics over all B L rows"""
    y = _f64(y); B, L, C = y.shape
    a = bn_lrelu_fwd(y, gamma, beta, st, slope)
    da = tail_da(dl, w3)
    dx, dga, dbe, _s1, _s2 = bn_lrelu_bwd(y.reshape(B * L, C), gamma, beta, st, da.reshape(B * L, C), slope, None if mask is None else mask.reshape(B * L, C))
    dw3 = torch.stack([(a * _shift_rows(_f64(dl), 1 - t)[:, :, None]).sum((0, 1)) for t in range(3)])
    return dx.reshape(B, L, C), dga, dbe, dw3, _f64(dl).sum()


# fused head: x (B, L) one input channel, w (3, C0), da (B, Lo, C0); pad 1
def head_taps(x, stride, Lo):
    """(3, B, Lo): x[b, s l + t - 1], zero outside the sample"""
    x = _f64(x); B, L = x.shape
    xp = torch.zeros(B, L + 2, dtype=torch.float64); xp[:, 1:L + 1] = x
    return torch.stack([xp[:, t:t + stride * Lo:stride][:, :Lo] for t in range(3)])


def head_z(x, w, bias, stride, Lo):
    xt = head_taps(x, stride, Lo); w = _f64(w)
    z = sum(xt[t][:, :, None] * w[t] for t in range(3))
    mag = sum((xt[t][:, :, None] * w[t]).abs() for t in range(3))
    if bias is not None:
        z = z + _f64(bias)
    return z, mag


def head_bwd(da, x, w, bias, slope, stride, mask=None):
    """(dw (3, C0), db (C0,), dx (B, L)) of a0 = lrelu(conv(x; w, stride, pad 1) + bias) for the gradient da of a0; mask recomputed from x"""
    da, w = _f64(da), _f64(w)
    B, Lo, C0 = da.shape; L = x.shape[1]
    z, _mag = head_z(x, w, bias, stride, Lo)
    m = (z > 0) if mask is None else mask
    dy = torch.where(m, da, slope * da)
    xt = head_taps(x, stride, Lo)
    dw = torch.stack([(dy * xt[t][:, :, None]).sum((0, 1)) for t in range(3)])
    q = torch.stack([(dy * w[t]).sum(-1) for t in range(3)])           # (3, B, Lo)
    dxp = torch.zeros(B, L + 2 + stride, dtype=torch.float64)
    for t in range(3):
        dxp[:, t:t + stride * Lo:stride][:, :Lo] += q[t]
    return dw, dy.sum((0, 1)), dxp[:, 1:L + 1]


def col_stats(y_unrounded):
    """(sum, sum of squares) per column of a (rows, N) float64 matrix"""
    y = _f64(y_unrounded)
    return y.sum(0), (y * y).sum(0)


# ---------------------------------------------------------------- fused frozen encoder (csrc/enc_fused.hip) and the other normalise-on-load conv
# y[b, :, l] = bias + sum_t W[:, :, t] a[b, :, l + t - 1] (+ row[b, :]) (+ resid[b, :, l]),  a = RNE_fmt(silu(x scale_b + shift_b)), zero outside the
# sample (the padding is of the ACTIVATED tensor).  NCL layout: x (B, Cin, L), w (Cout, Cin, 3), resid (B, Cout, L), row (B, Cout).
# Two forms of the fp32 apply (act_on_load's `form`):
#   "fp32" (eegldm_conv1d_fwd_gn's table kernel; pre_conv3_kernel before its shift moved to fp64): everything in fp32,
#       rstd' = fl(rstd), mean' = fl(mean), scale' = fl(gamma rstd'), shift' = fl(beta - fl(mean' scale')), z' = fl(x scale' + shift') (one fma),
#     so scale' carries 2u, mean' scale' 4u and the subtraction and the fma one rounding each:
#       |z' - z| <= u (2 |x scale| + 5 |mean scale| + |beta| + |z|) + O(u^2);  d_z spends one more u on every term for the O(u^2) part.
#     The errors act on the UNcentred magnitudes |x| rstd and |mean| rstd: at a mean of m sigma d_z is ~ 9 m u.
#   "centred" (pre_conv3_kernel): (mean, rstd) are fp64 values from the (sum, sum of squares) slots; scale' = fl(gamma fl(rstd)) as above,
#     mean = mh + ml with mh = fl(mean), and z' = fl(fl(x - mh) scale' + fl(beta - ml scale')): x - mh is exact for a 16-bit x within a factor
#     of two of the mean and carries u |x - mh| otherwise, the small shift u (|beta| + u |mean scale|), the fma u |z|:
#       |z' - z| <= u (3 |x - mean| |scale| + |beta| + |z|) + 2 u^2 |mean scale| + O(u^2);  again one more u per term below.
#     Every rounding acts on the centred value: d_z does not grow with |mean| / sigma.
def enc_affine(in_stats, n, gamma, beta, eps):
    """(mean (B,), var (B,) clamped at 0, rstd (B,), scale (B, C), shift (B, C)), float64, from per-sample (sum, sum of squares) slots over n
    elements -- the kernel's own fp64 expressions (eps is the fp32 value the kernel is handed, widened)"""
    S = _f64(in_stats).reshape(-1, 2)
    mean = S[:, 0] / n
    var = torch.clamp(S[:, 1] / n - mean * mean, min=0.0)
    var = torch.where(torch.isnan(S[:, 1] / n - mean * mean), S[:, 1] / n - mean * mean, var)       # (clamp keeps NaN in torch; explicit all the same)
    rstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    scale = _f64(gamma)[None, :] * rstd[:, None]
    shift = _f64(beta)[None, :] - mean[:, None] * scale
    return mean, var, rstd, scale, shift


def gn_affine(stats, C, gamma, beta):
    """the same per-(sample, channel) scale and shift from a (B, G, 2) buffer of (mean, rstd) -- eegldm_conv1d_fwd_gn's operand; returns
    (mean (B, C), scale (B, C), shift (B, C))"""
    st = _f64(stats)
    B, G, _ = st.shape
    mean = st[:, :, 0].repeat_interleave(C // G, dim=1); rstd = st[:, :, 1].repeat_interleave(C // G, dim=1)
    scale = _f64(gamma)[None, :] * rstd
    return mean, scale, _f64(beta)[None, :] - mean * scale


def act_on_load(x, mean, scale, shift, beta, silu=True, form="centred"):
    """(a, d_a): float64 silu(x scale + shift) and the fp32 bound of the apply derived above; through silu_f (z * rcp(1 + __expf(-z)), slope
    <= 1.1) it is 1.1 d + 8u |a|, the model tests/test_gpu_groupnorm_rounding.py uses for the same device function.  mean: (B,) or (B, C)."""
    x = _f64(x)
    sc, sh = scale[:, :, None], shift[:, :, None]
    mn = mean[:, None, None] if mean.dim() == 1 else mean[:, :, None]
    z = x * sc + sh
    if form == "fp32":
        d = U32 * (3 * (x * sc).abs() + 6 * (mn * sc).abs() + 2 * _f64(beta).abs()[None, :, None] + 2 * z.abs())
    else:
        d = U32 * (4 * ((x - mn) * sc).abs() + 2 * _f64(beta).abs()[None, :, None] + 2 * z.abs()) + 4 * U32 ** 2 * (mn * sc).abs()
    if not silu:
        return z, d
    a = F.silu(z)
    return a, 1.1 * d + 8 * U32 * a.abs()


def _conv3(a, w):
    return F.conv1d(F.pad(a, (1, 1)), w)


def _epilogue(y, bias, row, resid, mag=False):
    f = (lambda t: _f64(t).abs()) if mag else _f64
    if bias is not None:
        y = y + f(bias)[None, :, None]
    if row is not None:
        y = y + f(row)[:, :, None]
    if resid is not None:
        y = y + f(resid)
    return y


def conv3_on_load_ref(a, d_a, w, bias, resid, fmt, row=None):
    """(y_ref, mag, d) of the 3-tap conv whose operand is RNE_fmt(a') for SOME a' within d_a of a (the kernel rounds the activated operand to
    `fmt` before the MFMA, a point no test can observe): a_lo = RNE(a - d_a) <= operand <= a_hi = RNE(a + d_a) element by element, so
      y_ref = conv(RNE(a)) + bias + row + resid,   d = gamma(3 Cin) mag + conv(|w|, a_hi - a_lo),
    mag = the same operation on |operands| (the larger of |a_lo|, |a_hi| for the operand)."""
    w = _f64(w)
    Cin = w.shape[1]
    a_lo, a_hi = rne(a - d_a, fmt), rne(a + d_a, fmt)
    y_ref = _epilogue(_conv3(rne(a, fmt), w), bias, row, resid)
    mag = _epilogue(_conv3(torch.maximum(a_lo.abs(), a_hi.abs()), w.abs()), bias, row, resid, mag=True)
    d = gamma(3 * Cin) * mag + _conv3(a_hi - a_lo, w.abs())
    return y_ref, mag, d


def pre_conv3_ref(x, in_stats, gamma, beta, w, bias, resid, fmt, eps, gn_stats=None, row=None):
    """(y_ref, mag, d) of pre_conv3_kernel (in_stats: (B, 2) fp64 sums, one group) or, with gn_stats (B, G, 2) = (mean, rstd) in place of
    in_stats, of eegldm_conv1d_fwd_gn with G groups and a per-sample row vector.  Check A: numerics.check(y, y_ref, d / gamma(0), 0, fmt)."""
    x = _f64(x)
    B, C, L = x.shape
    if gn_stats is None:
        mean, _var, _rstd, scale, shift = enc_affine(in_stats, C * L, gamma, beta, eps)
    else:
        mean, scale, shift = gn_affine(gn_stats, C, gamma, beta)
    a, d_a = act_on_load(x, mean, scale, shift, beta, form="centred" if gn_stats is None else "fp32")
    return conv3_on_load_ref(a, d_a, w, bias, resid, fmt, row=row)


def pre_conv3_emul(x, G, gamma, beta, w, bias, resid, fmt, eps, row=None):
    """check B's emulation: torch fp32 group_norm + SiLU -> RNE -> F.conv1d -> + bias + row + resid (float32; `check` rounds it)"""
    x32 = _f64(x).float()
    a = F.silu(F.group_norm(x32, G, _f64(gamma).float(), _f64(beta).float(), eps=eps))
    a = rne(a.double(), fmt).float()
    y = F.conv1d(F.pad(a, (1, 1)), _f64(w).float())
    f32 = lambda t: None if t is None else _f64(t).float()
    return _epilogue(y, f32(bias), f32(row), f32(resid))


def sums_bound(values, depth, n64=0, preload=0.0):
    """bound of a one-pass fp32 sum of `values` (summed over the last dimension) whose every element passes through at most `depth`
    fp32 additions, in any order: gamma(depth) sum|v|; n64 further fp64 additions (block partials, atomics onto `preload`) add
    gamma64(n64) (sum|v| + |preload|)"""
    s = _f64(values).abs().sum(-1)
    return gamma(depth) * s + (gamma64(n64) * (s + _f64(torch.as_tensor(preload)).abs()) if n64 else 0.0)


def sample_stats_depth(n_per_sample):
    """additions behind one element of sample_stats_kernel: 8 per 16-byte chunk of a thread's grid-stride loop, 6 shuffle levels, 2 spare;
    `per` blocks of 256 threads per sample as sample_stats_launch computes it"""
    nch = n_per_sample // 8
    per = min(64, max(1, (nch + 255) // 256))
    return 8 * -(-nch // (per * 256)) + 6 + 2


PRE_CONV3_STATS_DEPTH = 64 + 6          # pre_conv3 epilogue: at most 64 values per lane (kept for every shape: any-order bound), 6 shuffle levels


def pre_conv3_pivots(y):
    """y (B, Cout, L) -> the pivot of every element: a lane of pre_conv3_kernel owns rows 64 w + 16 i + lm (i = 0..3) and channels
    32 h + 16 j + 4 q + (0..3) of a tile and sums them about the first, y[64 w + lm, 4 q]"""
    y = _f64(y)
    _B, C, L = y.shape
    li = torch.arange(L); ci = torch.arange(C)
    return y[:, ((ci % 16) // 4 * 4)[:, None], ((li // 64) * 64 + li % 16)[None, :]]


def pivot_sums_bounds(v, pivot, depth, n64=0, preload=None):
    """(e_S1, e_S2), each (B,): bounds of the (sum, sum of squares) of v (B, ...) as the kernels of csrc/enc_fused.hip form them -- fp32 sums
    D1 = sum d, D2 = sum d^2 of d = fl(v - p) about a pivot p that is itself an element of the tensor (`pivot`: broadcastable to v; pre_conv3:
    pre_conv3_pivots, one pivot per lane; sample_stats: the sample's first element), rebuilt in fp64 as S1 = D1 + g p, S2 = D2 + p (2 D1 + g p)
    per group of g elements that share a pivot:
      e(D1) = gamma(depth + 1) sum |d|            (the subtraction is one more rounding of every term)
      e(D2) = gamma(depth + 4) sum d^2            (d carries u, its square 2u, the fma one more)
      e_S1 = e(D1),   e_S2 = e(D2) + 2 gamma(depth + 1) sum |p| |d|,   plus gamma64(n64) of the magnitudes for the fp64 additions and atomics.
    pivot = None: p = 0, one-pass sums about zero (gamma(depth), gamma(depth + 2))."""
    v = _f64(v)
    B = v.shape[0]
    extra = 0 if pivot is None else 1
    p = torch.zeros_like(v) if pivot is None else _f64(pivot).expand_as(v)
    d = (v - p).reshape(B, -1); p = p.reshape(B, -1); vf = v.reshape(B, -1)
    pre = torch.zeros(B, 2, dtype=torch.float64) if preload is None else _f64(preload)
    f64 = gamma64(n64) if n64 else 0.0
    e_s1 = gamma(depth + extra) * d.abs().sum(-1) + f64 * (vf.abs().sum(-1) + pre[:, 0].abs())
    e_s2 = gamma(depth + 2 + 2 * extra) * (d * d).sum(-1) + 2 * gamma(depth + extra) * (p.abs() * d.abs()).sum(-1) + f64 * ((vf * vf).sum(-1) + pre[:, 1].abs())
    return e_s1, e_s2


def enc_stats_bounds(v, depth, eps, n64=0, pivot=None):
    """v: (B, ...) float64 values of the stored tensor.  The statistics a consumer derives in fp64 from the (sum, sum of squares) slots, and
    their bounds.  With the pivots of pivot_sums_bounds the errors of the slots are dS1 = sum_g dD1_g, dS2 = sum_g dD2_g + 2 p_g dD1_g, so for
    mean = S1 / n, var = S2 / n - mean^2:
      e_mean = gamma(depth + 1) sum |d| / n
      e_var  = gamma(depth + 4) sum d^2 / n + (2 / n) gamma(depth + 1) sum |p - mean| |d| + e_mean^2
      e_rstd (relative) = (1 - r)^(-1/2) - 1 with r = e_var / (var + eps): e_var / (2 (var + eps)) to first order.
    Sums about zero (pivot = None: p = 0, d = v) are the "split kernels" formulas of tests/test_gpu_groupnorm_rounding.py with m = mean: the
    first term then holds var + mean^2 and the second 2 |mean| e_mean -- the 1 + 3 mean^2 / var amplification.  About pivots that are
    elements of the tensor both terms are of the size of var: no mean^2 / var term, at any mean.
    Returns dict(mean, var, rstd, e_mean, e_var, e_rstd), each (B,)."""
    v = _f64(v)
    B = v.shape[0]
    extra = 0 if pivot is None else 1
    p = (torch.zeros_like(v) if pivot is None else _f64(pivot).expand_as(v)).reshape(B, -1)
    vf = v.reshape(B, -1)
    n = vf.shape[1]
    d = vf - p
    epsf = float(np.float32(eps))
    mean = vf.mean(-1)
    var = ((vf - mean[:, None]) ** 2).mean(-1)
    f64 = gamma64(n64) if n64 else 0.0
    e_mean = gamma(depth + extra) * d.abs().mean(-1) + f64 * vf.abs().mean(-1)
    e_var = gamma(depth + 2 + 2 * extra) * (d * d).mean(-1) + 2 * gamma(depth + extra) * ((p - mean[:, None]).abs() * d.abs()).mean(-1) + e_mean ** 2 \
        + f64 * (2 * (vf * vf).mean(-1) + 2 * mean.abs() * vf.abs().mean(-1))
    r = e_var / (var + epsf)
    e_rstd = torch.where(r < 1, (1 - torch.clamp(r, max=1 - 1e-12)) ** -0.5 - 1, torch.full_like(r, math.inf))
    return dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + epsf), e_mean=e_mean, e_var=e_var, e_rstd=e_rstd)


def check_rows(got, ref, d, fmt, rows, route="", report=True):
    """check A with the absolute bound d on single positions l of (B, C, L) tensors, one verdict per (sample, row): a defect at a tile or
    sample seam is named by its row instead of being averaged over the tensor.  rows: positions (negative: from the end); those outside
    the tensor are skipped.  Returns the list of failure messages (one per failing row, each naming "sample b row l")."""
    got, ref, d = _f64(got), _f64(ref), _f64(d)
    B, _C, L = ref.shape
    ls = sorted({r % L for r in rows if -L <= r < L})
    fails, worst = [], []
    for l in ls:
        ok, ratio = _within(got[:, :, l], ref[:, :, l], d[:, :, l], fmt)
        worst.append(float(ratio.max()))
        for b in range(B):
            if not bool(ok[b].all()):
                i = int(torch.argmax(torch.nan_to_num(ratio[b], posinf=1e300)))
                fails.append(f"{route} [{fmt}]: sample {b} row {l}: {int((~ok[b]).sum())} of {ok.shape[1]} channels outside the bound (channel {i}: got "
                             f"{got[b, i, l].item()!r}, ref {ref[b, i, l].item()!r}, {float(ratio[b, i]):.3g} x its bound)")
    if report:
        print(f"[numerics] {route} rows " + " ".join(f"{l}:{w:.2f}" for l, w in zip(ls, worst)) + " (worst error / bound per row, all samples)")
    return fails
