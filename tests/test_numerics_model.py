"""CPU: the checks of tests/numerics.py are sharp at the shapes tests/test_gpu_rounding.py runs.  Results a correct kernel may produce (fp32
accumulation in two different orders, rounded once) pass check A and check B; emulations of the defects a kernel could have (truncation,
a second rounding in the epilogue, 16-bit partial sums, a lost K stage or split-K chunk, a wrong partial tile, fp16 saturation or
subnormal flush, a NaN turned finite) fail one of them."""
import math

import pytest
import torch

import numerics as N

FWD = dict(B=2, L=192, Cin=128, Cout=192, K=3)          # the 128 x 128 kernel's forward case: sample boundaries inside tiles, a partial N tile
WGRAD = dict(B=2, L=192, Cin=192, Cout=128, K=3)        # weight gradient: reduction B * L = 384, a partial 128-column tile of Cin


def _fwd_operands(fmt, seed=0, wscale=1.0, with_epilogue=True):
    g = torch.Generator().manual_seed(seed)
    B, L, Cin, Cout, K = (FWD[k] for k in ("B", "L", "Cin", "Cout", "K"))
    x = N.to_storage(torch.randn(B, Cin, L, generator=g, dtype=torch.float64), fmt)
    w = N.to_storage(torch.randn(Cout, Cin, K, generator=g, dtype=torch.float64) * wscale / math.sqrt(Cin * K), fmt)
    ep = {}
    if with_epilogue:
        ep = dict(b=N.rne(torch.randn(Cout, generator=g, dtype=torch.float64) * wscale, "f32"),
                  row=N.rne(torch.randn(B, Cout, generator=g, dtype=torch.float64) * wscale, "f32"),
                  resid=N.to_storage(torch.randn(B, Cout, L, generator=g, dtype=torch.float64) * wscale, fmt))
    return x, w, ep


def _fp32_chunked(x, w, ep, chunks=8, reverse=True, round_partials=None, drop_last_stage=False):
    """fp32 conv with the reduction over Cin cut into `chunks` pieces summed in fp32 (reverse order), epilogue in fp32"""
    x32, w32 = x.float(), w.float().clone()
    if drop_last_stage:
        w32[:, -32:, -1] = 0             # the last K stage of the reduction: the last 32 input channels of the last tap
    Cin = x.shape[1]
    step = Cin // chunks
    parts = []
    for c in range(chunks):
        ws = w32[:, c * step:(c + 1) * step]
        p = torch.nn.functional.conv1d(x32[:, c * step:(c + 1) * step], ws, padding=1)
        parts.append(N.rne(p, round_partials).float() if round_partials else p)
    acc = torch.zeros_like(parts[0])
    for p in (reversed(parts) if reverse else parts):
        acc = acc + p
    return acc


def _epilogue32(acc, ep):
    y = acc.float()
    if "b" in ep:
        y = y + ep["b"].float()[:, None]
    if "row" in ep:
        y = y + ep["row"].float()[:, :, None]
    if "resid" in ep:
        y = y + ep["resid"].float()
    return y


def _ref(x, w, ep):
    return N.evaluate(N.conv1d_fwd, x, w, ep.get("b"), 1, 1, 1, ep.get("row"), ep.get("resid"))


def _fails(fn):
    with pytest.raises(AssertionError, match="check [AB]"):
        fn()


# ---------------------------------------------------------------- the rounding helper
@pytest.mark.parametrize("fmt,x,want", [
    ("bf16", 1 + 2 ** -8, 1.0),                          # tie: to even (down)
    ("bf16", 1 + 3 * 2 ** -8, 1 + 2 ** -6),              # tie: to even (up)
    ("bf16", 1 + 2 ** -8 + 2 ** -30, 1 + 2 ** -7),       # just above the tie: torch's float64 -> float32 -> bf16 path gives 1.0
    ("bf16", 1 + 2 ** -8 - 2 ** -30, 1.0),
    ("f16", 1 + 2 ** -11, 1.0),
    ("f16", 1 + 2 ** -11 + 2 ** -40, 1 + 2 ** -10),      # (double-rounded by torch to 1.0)
    ("f16", 65504.0, 65504.0),
    ("f16", 65520.0 - 2 ** -20, 65504.0),                # just below the overflow threshold
    ("f16", 65520.0, math.inf),                          # max + ulp / 2: the tie goes to inf
    ("f16", -70000.0, -math.inf),
    ("bf16", (2 - 2 ** -8) * 2.0 ** 127, math.inf),
    ("bf16", (2 - 2 ** -8) * 2.0 ** 127 * (1 - 2 ** -20), (2 - 2 ** -7) * 2.0 ** 127),
    ("f16", 2.0 ** -24, 2.0 ** -24),                     # smallest subnormal
    ("f16", 2.0 ** -25, 0.0),                            # tie with zero: to even
    ("f16", 2.0 ** -25 * (1 + 2 ** -30), 2.0 ** -24),
    ("f16", 3 * 2.0 ** -25, 2 * 2.0 ** -24),             # subnormal tie 1.5 ulp -> 2 ulp
    ("f16", 2.0 ** -14 - 2.0 ** -26, 2.0 ** -14),        # top of the subnormal range rounds into the normals
    ("bf16", 2.0 ** -133, 2.0 ** -133),                  # smallest bf16 subnormal
    ("bf16", 2.0 ** -134, 0.0),
    ("bf16", -2.0 ** -134 * 1.5, -2.0 ** -133),
])
def test_rne_edges(fmt, x, want):
    got = float(N.rne(torch.tensor([x], dtype=torch.float64), fmt))
    assert got == want, (fmt, x, got, want)


def test_rne_nonfinite_and_signed_zero():
    x = torch.tensor([math.nan, math.inf, -math.inf, -0.0, 0.0], dtype=torch.float64)
    for fmt in ("bf16", "f16"):
        r = N.rne(x, fmt)
        assert math.isnan(r[0]) and r[1] == math.inf and r[2] == -math.inf
        assert math.copysign(1.0, float(r[3])) == -1.0 and float(r[4]) == 0.0


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_rne_equals_the_single_rounding_of_float32_values(fmt):
    """for float32 inputs torch's cast is ONE correct rounding: the helper must agree bit for bit (normals, subnormals, overflow)"""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200_000, generator=g) * torch.exp2(torch.randint(-30, 20, (200_000,), generator=g).float())
    want = x.to(N.torch_dtype(fmt)).double()
    got = N.rne(x.double(), fmt)
    assert torch.equal(got, want)


def test_rtz_and_ulp():
    x = torch.tensor([1 + 2 ** -7 - 2 ** -20, -(1 + 2 ** -7 - 2 ** -20)], dtype=torch.float64)
    assert N.rtz(x, "bf16").tolist() == [1.0, -1.0]
    assert N.ulp(torch.tensor([1.0, 2.0 ** -20], dtype=torch.float64), "f16").tolist() == [2 ** -10, 2 ** -24]


# ---------------------------------------------------------------- forward (16-bit outputs)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_two_fp32_summation_orders_are_accepted(fmt):
    x, w, ep = _fwd_operands(fmt)
    ref, mag, emul = _ref(x, w, ep)
    n = FWD["K"] * FWD["Cin"]
    N.check(N.rne(emul, fmt), ref, mag, n, fmt, emul=emul, route="model: torch fp32 order")
    alt = _epilogue32(_fp32_chunked(x, w, ep, chunks=8, reverse=True), ep)
    N.check(N.rne(alt, fmt), ref, mag, n, fmt, emul=emul, route="model: 8 K chunks, reversed")


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_forward_defects_are_rejected(fmt):
    x, w, ep = _fwd_operands(fmt)
    ref, mag, emul = _ref(x, w, ep)
    n = FWD["K"] * FWD["Cin"]
    run = lambda got: N.check(got, ref, mag, n, fmt, emul=emul, route="model: defect", report=False)
    _fails(lambda: run(N.rtz(emul, fmt)))                                                      # truncation instead of RNE
    conv32 = torch.nn.functional.conv1d(x.float(), w.float(), padding=1)
    _fails(lambda: run(N.rne(_epilogue32(N.rne(conv32, fmt), ep), fmt)))                       # bias + row + residual after a 16-bit rounding
    _fails(lambda: run(N.rne(_epilogue32(N.rne(conv32, fmt) , {"resid": ep["resid"]}) + ep["b"][:, None] + ep["row"][:, :, None], fmt)))  # residual only
    _fails(lambda: run(N.rne(_epilogue32(_fp32_chunked(x, w, ep, round_partials=fmt), ep), fmt)))   # 16-bit split partials
    _fails(lambda: run(N.rne(_epilogue32(_fp32_chunked(x, w, ep, drop_last_stage=True), ep), fmt)))  # last 32-channel K stage dropped
    bad = N.rne(emul, fmt).clone(); bad.view(-1)[::997] = N.rne(emul, fmt).view(-1)[::997] + N.ulp(emul, fmt).view(-1)[::997]
    _fails(lambda: run(bad))                                                                    # one ulp off on 0.1 % of the elements


def test_bias_added_after_rounding_without_epilogue_operands_is_one_rounding():
    """(sanity of the model above: with no epilogue terms a second rounding of a 16-bit value is a no-op and must pass)"""
    x, w, _ = _fwd_operands("bf16", with_epilogue=False)
    ref, mag, emul = _ref(x, w, {})
    N.check(N.rne(N.rne(emul, "bf16"), "bf16"), ref, mag, 3 * FWD["Cin"], "bf16", emul=emul, route="model: no epilogue")


def test_fp16_saturation_and_subnormal_flush_are_rejected():
    for wscale, defect in ((2.0 ** 15, "saturate"), (2.0 ** -17, "flush")):
        x, w, _ = _fwd_operands("f16", seed=3, wscale=wscale, with_epilogue=False)
        ref, mag, emul = _ref(x, w, {})
        good = N.rne(emul, "f16")
        if defect == "saturate":
            assert bool(torch.isinf(N.rne(ref, "f16")).any())
            bad = good.clamp(-65504.0, 65504.0)
        else:
            sub = (good != 0) & (good.abs() < 2.0 ** -14)
            assert float(sub.double().mean()) > 0.5
            bad = torch.where(sub, torch.zeros_like(good), good)
        N.check(good, ref, mag, 3 * FWD["Cin"], "f16", emul=emul, route=f"model: f16 {defect} range, correct")
        _fails(lambda: N.check(bad, ref, mag, 3 * FWD["Cin"], "f16", emul=emul, report=False))


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_nan_turned_finite_is_rejected(fmt):
    x, w, ep = _fwd_operands("f16" if fmt == "f16" else "bf16")
    x = x.clone(); x[1, 5, 77] = math.nan; x[0, 9, 3] = math.inf
    ref, mag, emul = _ref(x, w, ep)
    assert bool(torch.isnan(ref).any())
    good = N.rne(emul, fmt)
    N.check(good, ref, mag, 3 * FWD["Cin"], fmt, emul=emul, route="model: non-finite input, correct")
    _fails(lambda: N.check(torch.nan_to_num(good, nan=0.0, posinf=65504.0, neginf=-65504.0), ref, mag, 3 * FWD["Cin"], fmt, emul=emul, report=False))


# ---------------------------------------------------------------- weight gradient (fp32 outputs, check A)
def _wgrad_operands(fmt, seed=5):
    g = torch.Generator().manual_seed(seed)
    B, L, Cin, Cout = (WGRAD[k] for k in ("B", "L", "Cin", "Cout"))
    x = N.to_storage(torch.randn(B, Cin, L, generator=g, dtype=torch.float64), fmt)
    dy = N.to_storage(torch.randn(B, Cout, L, generator=g, dtype=torch.float64), fmt)
    return x, dy


def _wgrad_chunks(x, dy, chunks=16, drop=None):
    """fp32 dW as `chunks` split-K pieces over the flattened (sample, position) reduction, summed in reverse"""
    B, _, L = x.shape
    rows = B * L // chunks
    acc = None
    pieces = []
    for c in range(chunks):
        m = torch.zeros(B * L)
        m[c * rows:(c + 1) * rows] = 1
        m = m.view(B, 1, L)
        pieces.append(N.conv1d_wgrad(x.float(), (dy.float() * m), 3, 1, 1, 1) if c != drop else None)
    for p in reversed(pieces):
        if p is not None:
            acc = p if acc is None else acc + p
    return acc


@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_weight_gradient_orders_accepted_and_defects_rejected(fmt):
    x, dy = _wgrad_operands(fmt)
    ref, mag, emul = N.evaluate(N.conv1d_wgrad, x, dy, 3, 1, 1, 1)
    n = WGRAD["B"] * WGRAD["L"]
    N.check(emul, ref, mag, n, "f32", route="model: dW torch fp32")
    N.check(_wgrad_chunks(x, dy), ref, mag, n, "f32", route="model: dW 16 split-K chunks, reversed")
    run = lambda got: N.check(got, ref, mag, n, "f32", report=False)
    _fails(lambda: run(_wgrad_chunks(x, dy, drop=7)))                        # one of 16 split-K chunks lost
    _fails(lambda: run(_wgrad_chunks(x, dy) + _wgrad_chunks(x, dy, chunks=16, drop=None) / 16))    # a chunk counted twice (on average)
    bad = emul.clone(); bad[:, 128:] *= 1.01
    _fails(lambda: run(bad))                                                 # last partial N (Cin) tile wrong by 1 %
    bad = emul.clone(); bad[-1, -1, -1] = math.nan
    _fails(lambda: run(bad))
    db_ref, db_mag, db_emul = N.evaluate(N.bias_grad, dy)
    N.check(db_emul, db_ref, db_mag, n, "f32", route="model: db")
    _fails(lambda: N.check(db_emul * (1 + 2 ** -12), db_ref, db_mag, n, "f32", report=False))


def test_weight_gradient_accumulation_into_nonzero_dw():
    x, dy = _wgrad_operands("bf16")
    acc = torch.randn(WGRAD["Cout"], WGRAD["Cin"], 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64).float().double() * 10
    ref, mag, emul = N.evaluate(N.conv1d_wgrad, x, dy, 3, 1, 1, 1, acc)
    n = WGRAD["B"] * WGRAD["L"]
    N.check(emul, ref, mag, n, "f32", route="model: dW += into non-zero")
    _fails(lambda: N.check(emul - acc.float(), ref, mag, n, "f32", report=False))          # overwrote instead of accumulating
