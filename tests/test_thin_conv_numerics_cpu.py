"""CPU: the checks of tests/numerics.py are sharp at the shapes tests/test_gpu_thin_conv_rounding.py runs on the thin direct kernels
(csrc/direct_conv.hip).  From the float64 reference of six of its cases this file builds what a subtly wrong kernel would store -- a tap
dropped on the first row of a segment, a tap read across a sample boundary, the bias omitted in one 8-channel group, truncation instead of
one rounding, a row segment missing from a weight gradient, a `+=` that overwrites -- and asserts that numerics.check rejects each, and that
it accepts the correctly rounded reference and a plain fp32 evaluation.  No kernel runs in a wrong form: the defect models live here."""
import math

import pytest
import torch

import numerics as N


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _lout(L, K, s, pl, pr):
    return (L + pl + pr - K) // s + 1


def _fwd_operands(shape, fmt, bias=True):
    """the operands test_gpu_thin_conv_rounding._fwd builds (same seeds)"""
    B, L, Cin, Cout, K, s, pl, pr = shape
    x = N.to_storage(_randn((B, Cin, L), 1), fmt)
    w = N.to_storage(_randn((Cout, Cin, K), 2, 1 / math.sqrt(Cin * K)), fmt)
    b = N.rne(_randn((Cout,), 3), "f32") if bias else None
    return x, w, b


def _wgrad_operands(shape, fmt, accumulate=False):
    B, L, Cin, Cout, K, s, pl, pr = shape
    x = N.to_storage(_randn((B, Cin, L), 31), fmt)
    dy = N.to_storage(_randn((B, Cout, _lout(L, K, s, pl, pr)), 32), fmt)
    acc = N.rne(_randn((Cout, Cin, K), 33, 8.0), "f32") if accumulate else None
    return x, dy, acc


def _fails(fn):
    with pytest.raises(AssertionError, match="check [AB]"):
        fn()


def _fwd_judge(shape, fmt, x, w, b):
    B, L, Cin, Cout, K, s, pl, pr = shape
    ref, mag, emul = N.evaluate(N.conv1d_fwd, x, w, b, s, pl, pr)
    n = K * Cin
    run = lambda got, route="model: defect", report=False: N.check(got, ref, mag, n, fmt, emul=emul, route=route, report=report)
    run(N.rne(ref, fmt), "model: RNE(ref)", True)
    run(N.rne(emul, fmt), "model: torch fp32, rounded once", True)
    return ref, emul, run


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_tap_dropped_on_the_first_row_of_a_segment(fmt):
    """in1_seg, (3,129,1,32,3,1,1,1): output row 128 is the only row of the second 128-row segment; its tap 0 (x[127]) is lost"""
    shape = (3, 129, 1, 32, 3, 1, 1, 1)
    x, w, b = _fwd_operands(shape, fmt)
    ref, emul, run = _fwd_judge(shape, fmt, x, w, b)
    bad = emul.clone()
    bad[:, :, 128] -= (x[:, 0, 127, None] * w[None, :, 0, 0]).float()
    _fails(lambda: run(N.rne(bad, fmt)))
    one = emul.clone()                                  # the same in one sample only: 32 wrong elements of 12384
    one[1, :, 128] = bad[1, :, 128]
    _fails(lambda: run(N.rne(one, fmt)))


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_tap_read_across_a_sample_boundary(fmt):
    """thin_out_run, (3,8,32,1,3,1,1,1): one run per sample; tap 0 of row 0 reads the last row of the previous sample instead of the padding,
    tap 2 of the last row the first row of the next sample (what an unclamped, unguarded window load would do)"""
    shape = (3, 8, 32, 1, 3, 1, 1, 1)
    x, w, b = _fwd_operands(shape, fmt)
    ref, emul, run = _fwd_judge(shape, fmt, x, w, b)
    lo = emul.clone()
    lo[1:, 0, 0] += (x[:-1, :, -1] * w[0, :, 0]).sum(-1).float()
    _fails(lambda: run(N.rne(lo, fmt)))
    hi = emul.clone()
    hi[:-1, 0, -1] += (x[1:, :, 0] * w[0, :, 2]).sum(-1).float()
    _fails(lambda: run(N.rne(hi, fmt)))


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_bias_omitted_in_one_channel_group(fmt):
    """thin_in_reg, (2,64,2,32,3,1,1,1) with bias: the second 8-channel group of every row misses its bias"""
    shape = (2, 64, 2, 32, 3, 1, 1, 1)
    x, w, b = _fwd_operands(shape, fmt)
    ref, emul, run = _fwd_judge(shape, fmt, x, w, b)
    bad = emul.clone()
    bad[:, 8:16, :] -= b[8:16].float()[None, :, None]
    _fails(lambda: run(N.rne(bad, fmt)))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_truncation_instead_of_one_rounding(fmt):
    """thin_in_reg check-B shape (4,512,2,64,3,1,1,1): 131072 outputs; on the 2432-element small shape (2,19,.,.) check A alone sees it"""
    for shape in ((4, 512, 2, 64, 3, 1, 1, 1), (2, 19, 4, 8, 3, 1, 1, 1)):
        x, w, b = _fwd_operands(shape, fmt)
        ref, emul, run = _fwd_judge(shape, fmt, x, w, b)
        _fails(lambda: run(N.rtz(emul, fmt)))


def test_row_segment_missing_from_a_weight_gradient():
    """in1out, (2,192,32,1,3,1,1,1) bf16: three 64-row segments of x per sample, each a block whose partial sums a fold adds; one is lost"""
    shape = (2, 192, 32, 1, 3, 1, 1, 1)
    x, dy, _ = _wgrad_operands(shape, "bf16")
    ref, mag, emul = N.evaluate(N.conv1d_wgrad, x, dy, 3, 1, 1, 1)
    n = 2 * 192
    N.check(N.rne(ref, "f32"), ref, mag, n, "f32", route="model: dW RNE(ref)")
    N.check(emul, ref, mag, n, "f32", route="model: dW torch fp32")
    xm = x.clone(); xm[1, :, 64:128] = 0
    _fails(lambda: N.check(N.conv1d_wgrad(xm.float(), dy.float(), 3, 1, 1, 1), ref, mag, n, "f32", report=False))
    bref, bmag, bemul = N.evaluate(N.bias_grad, dy)
    N.check(bemul, bref, bmag, n, "f32", route="model: db torch fp32")
    dm = dy.clone(); dm[1, :, 64:128] = 0
    _fails(lambda: N.check(N.bias_grad(dm.float()), bref, bmag, n, "f32", report=False))


@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_accumulation_that_overwrites(fmt):
    """tinyv, (2,37,2,4,3,1,1,1) run as += onto non-zero dW: the fold writes instead of adding"""
    shape = (2, 37, 2, 4, 3, 1, 1, 1)
    x, dy, acc = _wgrad_operands(shape, fmt, accumulate=True)
    ref, mag, emul = N.evaluate(N.conv1d_wgrad, x, dy, 3, 1, 1, 1, acc)
    n = 2 * 37
    N.check(N.rne(ref, "f32"), ref, mag, n, "f32", route="model: dW += RNE(ref)")
    N.check(emul, ref, mag, n, "f32", route="model: dW += torch fp32")
    _fails(lambda: N.check(emul - acc.float(), ref, mag, n, "f32", report=False))


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_zero_tap_times_inf_is_rejected(fmt):
    """in1_seg K = 1, (2,130,1,16,1,1,0,0) with +inf at x[0, 0, 0]: the outputs it feeds are +-inf; a kernel that also multiplies it by the
    zero weight of a tap beyond K stores NaN there, and check A must say so (an inf stays the same inf)"""
    shape = (2, 130, 1, 16, 1, 1, 0, 0)
    x, w, b = _fwd_operands(shape, fmt)
    x = x.clone(); x[0, 0, 0] = math.inf
    ref, mag, emul = N.evaluate(N.conv1d_fwd, x, w, b, 1, 0, 0)
    assert bool(torch.isinf(ref[0, :, 0]).all()) and int(torch.isinf(ref).sum()) == 16
    N.check(N.rne(emul, fmt), ref, mag, 1, fmt, emul=emul, route="model: inf in x, correct")
    bad = N.rne(emul, fmt).clone(); bad[0, :, 0] = math.nan
    _fails(lambda: N.check(bad, ref, mag, 1, fmt, emul=emul, report=False))


def test_lost_wrapped_rows_need_the_wrapped_rows_only_run():
    """tinyv wrap case at 256 CUs, (2, 65836, 1, 1, 3,1,1,1): 512 blocks of 256 rows, 600 wrapped rows of 131672.  The bound of the full sum
    (gamma(131672) x the sum of magnitudes) is wider than everything the wrapped rows contribute, so a kernel that never comes round again
    passes the full case; with dy zero on the first pass's rows, as the GPU test runs it a second time, the same bound rejects it."""
    shape = (2, 256 * 256 + 300, 1, 1, 3, 1, 1, 1)
    B, L = shape[0], shape[1]
    x, dy, _ = _wgrad_operands(shape, "bf16")
    covered, n = 512 * 256, B * L
    flat = dy.permute(0, 2, 1).reshape(n, 1)
    head, tail = flat.clone(), flat.clone()
    head[covered:] = 0; tail[:covered] = 0
    back = lambda f: f.reshape(B, L, 1).permute(0, 2, 1).contiguous()
    lost = N.conv1d_wgrad(x.float(), back(head).float(), 3, 1, 1, 1)            # what a loop without the wrap would sum
    ref, mag, _ = N.evaluate(N.conv1d_wgrad, x, dy, 3, 1, 1, 1)
    assert N.check_a(lost, ref, mag, n, "f32")[0] == 0                          # the full case cannot see it
    ref, mag, emul = N.evaluate(N.conv1d_wgrad, x, back(tail), 3, 1, 1, 1)
    N.check(emul, ref, mag, n, "f32", route="model: dW of the wrapped rows alone")
    _fails(lambda: N.check(torch.zeros_like(emul), ref, mag, n, "f32", report=False))
