"""-m gpu: the whole-network AutoencoderKL kernels (csrc/aekl_thin.hip: one workgroup per window interprets the model as micro-ops over four
LDS tensors) and their program builder (csrc/aekl.hip: thin_eligible, ThinBuilder, thin_build, thin_ready) against oracle/aekl.py run in
float64 (tests/aekl_thin_reference.py).

Every case runs forward and backward and compares EVERY element of recon, z_mu, z_sigma, the KL scalar, dx and every parameter gradient
(full tensors, unpacked through net.entries; no digests).  Per tensor e(t) = max |t - t64| / max |t64| over the whole batch; the yardstick is
the same quantity of the float32 CPU oracle on the same case, computed here at run time; the bound is
    e_engine <= 8 * max(e_fp32_oracle, 2^-20).
8 covers summation order (four positions per thread, 16-lane rows, waves, then atomics across windows, against aten's order) and the hardware
exp / rcp / rsqrt of SiLU and the norms; 2^-20 = 16 fp32 epsilons keeps the bound meaningful where the fp32 oracle happens to be exact.
Gradients that are exactly zero in exact arithmetic (biases in front of a one-channel GroupNorm) are measured against the largest gradient of
their class instead of their own float64 rounding noise (aekl_thin_reference.vanishing_grads).

Each case confirms from eegldm_debug_aekl_last_route which route served both directions; each whole-network case runs again on the
layer-by-layer path of the fp32 engine (EEGLDM_AEKL_NO_THIN=1) under the same bound, and one runs with the bfloat16 engine (the whole-network
kernels compute in fp32 whatever the engine dtype).  Each run prints one `[numerics]` line per tensor class: worst e_engine / max(e_fp32, 2^-20).

Worst ratio per class over all cases, measured on an MI355X (whole-network route | layer-by-layer route: EEGLDM_AEKL_NO_THIN=1 and the
fallback cases), and the case that gave it:
  recon                  0.67 (backward_ex_low_clamp)     | 1.01 (wide_lat4_nrb3)
  z_mu                   1.08 (lengths_64_128_64)         | 2.21 (rows_not_float4)
  z_sigma                0.29 (nine_convs_c1_lat2)        | 0.47 (nine_convs_c1_lat2)
  kl                     0.41 (smallest_length)           | 1.03 (rows_not_float4)
  dx                     1.62 (wide_lat4_nrb3)            | 1.56 (lengths_64_128_64)
  grad conv.weight       2.45 (lengths_64_128_64)         | 3.17 (nine_convs_c1_lat2)
  grad conv.bias         6.43 (lengths_64_128_64)         | 4.55 (two_levels)
  grad norm.weight       5.81 (four_levels)               | 3.48 (outlier_first_element)
  grad norm.bias         3.15 (wide_lat4_nrb3)            | 4.40 (rows_not_float4)
  grad shortcut.weight   1.38 (lengths_64_128_64)         | 1.40 (lengths_64_128_64)
  grad shortcut.bias     2.59 (backward_ex_low_clamp)     | 2.56 (two_levels)
  grad heads             6.86 (batch_1_then_5)            | 4.76 (batch_1_then_5)
  grad post_quant        3.16 (batch_1_then_5)            | 4.37 (lengths_64_128_64)
The bias gradients, the one-element gradients of the LAT = 1 heads and the norm scales sit closest to the bound: sums of up to B * L terms
whose yardstick is on the 2^-20 floor.

The outlier cases.  f_gn_t used to take its one-pass variance about the tensor's first element.  With that kernel outlier_first_element
(L = 512) passed at 4.37 (grad norm.weight) and outlier_first_element_full_window (L = 3072, added for this reason: the cancellation grows
with the number of values behind the outlier) failed on 99 of 131 tensors: recon 50, z_mu 60, dx 168, grad conv.bias 206, grad norm.bias 220
x the yardstick (errors of 5e-5 to 7e-4 of the tensor's scale), while the layer-by-layer path stayed under 1.0.  With the second pass that
f_gn_t now takes when the first element lies more than two standard deviations from the mean, the same cases measure 4.26 (grad norm.weight)
and 1.68 (grad conv.weight) at worst.

edge_accepted (4 L = THIN_MAX_FLOATS - 1024) fits the LDS: the whole-network program runs it, with no spare LDS tensor left for the tape
prefetch of the backward kernel -- the only case on that branch.
"""
import ctypes

import pytest
import torch

import aekl_thin_reference as R

pytestmark = pytest.mark.gpu

WHOLE = [n for n, c in R.CASES.items() if c["route"] != R.FALLBACK]
RUNS = [(n, "default") for n in R.CASES] + [(n, "no_thin") for n in WHOLE]


def _G():
    import gpu_util as G
    return G


def _net(name, dtype="float32"):
    from eegldm.models import AutoencoderKL
    cfg = R.cfg_of(R.CASES[name])
    net = AutoencoderKL(spatial_dims=1, attention_levels=[False] * len(cfg["num_channels"]), dtype=dtype, **cfg)
    inp = R.make_inputs(name, *R.steps_of(R.CASES[name])[0])
    assert list(net.entries) == list(inp["sd"])
    assert int(_G().lib.eegldm_aekl_num_params(net.h)) == R.engine_nparams({k: v.shape for k, v in inp["sd"].items()})
    net.load_state_dict({k: torch.from_numpy(v) for k, v in inp["sd"].items()})
    return net


def _route(net):
    G = _G()
    out = (ctypes.c_int * 10)()
    G.check(G.lib.eegldm_debug_aekl_last_route(net.h, out))
    keys = ("thin", "nfwd", "nbwd", "maxt", "lds_fail")
    return dict(zip(keys, out[0:5])), dict(zip(keys, out[5:10]))


def _step(net, inp, need_dx=True, zero=True):
    """one forward + backward on the engine -> (tensors by the names of aekl_thin_reference.flatten, forward route, backward route)"""
    G = _G()
    dev = net.device
    klo = torch.zeros(1, device=dev)
    recon, mu, sg = net(torch.from_numpy(inp["x"]), eps=torch.from_numpy(inp["eps"]), kl_out=klo)
    if zero:
        net.zero_grad()
    dy = torch.from_numpy(inp["dy"]).to(dev)
    dx = torch.full((inp["B"], inp["cfg"]["in_channels"], inp["L"]), float("nan"), device=dev) if need_dx else None
    dmu = torch.from_numpy(inp["d_mu"]).to(dev) if inp["d_mu"] is not None else None
    dsg = torch.from_numpy(inp["d_sigma"]).to(dev) if inp["d_sigma"] is not None else None
    G.check(G.lib.eegldm_aekl_backward_ex(net.h, G.ptr(dy), G.ptr(dmu), G.ptr(dsg), float(inp["kl_weight"]), G.ptr(dx)))
    torch.cuda.synchronize()
    got = dict(recon=recon, z_mu=mu, z_sigma=sg, kl=klo)
    if need_dx:
        got["dx"] = dx
    for k, v in net.grad_dict().items():
        got["grad:" + k] = v
    fwd, bwd = _route(net)
    return {k: v.detach().double().cpu() for k, v in got.items()}, fwd, bwd


def _hold(tag, got, f64, yard, scale):
    """every tensor inside FACTOR x its yardstick; one `[numerics]` line per class; returns the worst ratio per class"""
    worst, bad = {}, []
    for k, t64 in f64.items():
        assert tuple(got[k].shape) == tuple(t64.shape), (tag, k, got[k].shape, t64.shape)
        e = R.rel_err(got[k], t64, scale[k]); ratio = e / yard[k]
        c = R.tensor_class(k)
        if c not in worst or ratio > worst[c][0]:
            worst[c] = (ratio, k, e, yard[k])
        if not ratio <= R.FACTOR:
            bad.append(f"{k}: e {e:.3e} = {ratio:.2f} x max(fp32 oracle, 2^-20) = {yard[k]:.3e}")
    for c, (ratio, k, e, y) in worst.items():
        print(f"[numerics] {tag} {c}: worst ratio {ratio:.3f} ({k}: e {e:.2e}, yardstick {y:.2e})")
    assert not bad, f"{tag}: {len(bad)} tensors past {R.FACTOR:g} x their yardstick:\n  " + "\n  ".join(bad)
    return worst


def _confirm(tag, case, mode, fwd, bwd):
    print(f"[route] {tag}: forward {fwd} backward {bwd}")
    for r in (fwd, bwd):
        if mode == "no_thin" or case["route"] == R.FALLBACK:
            assert r["thin"] == 0 and r["lds_fail"] == 0 and r["nfwd"] == 0, f"{tag}: expected the layer-by-layer path, got {r}"
        elif case["route"] == R.THIN:
            assert r["thin"] == 1 and r["nfwd"] > 0 and r["nbwd"] > 0 and 0 < r["maxt"] <= R.THIN_MAX_FLOATS, f"{tag}: the whole-network program did not run: {r}"
        else:       # accepted by thin_eligible: the program ran, or the footprint check refused it and says so
            assert (r["thin"] == 1) != (r["lds_fail"] == 1), f"{tag}: neither the whole-network program nor its fit fallback: {r}"
    assert fwd == bwd, f"{tag}: forward and backward took different routes"


def _exact_zero_rows(tag, case, got):
    if "lv_bias0" in case:      # latent channel 0 is clamped everywhere: no gradient may reach its log-variance head
        gw, gb = got["grad:quant_conv_log_sigma.conv.weight"], got["grad:quant_conv_log_sigma.conv.bias"]
        assert float(gw[0].abs().max()) == 0.0 and float(gb[0].abs()) == 0.0, f"{tag}: gradient through the clamp: {gw[0].tolist()} {float(gb[0])}"


@pytest.mark.parametrize("name,mode", RUNS, ids=[f"{n}-{m}" for n, m in RUNS])
def test_every_element_against_float64(name, mode, env_switches):
    case = R.CASES[name]
    env_switches(EEGLDM_AEKL_NO_THIN="1" if mode == "no_thin" else None)
    inst = R.instantiations(R.cfg_of(case))
    print(f"[reach] {name}: convs {inst['convs']} norms {inst['norms']} heads LAT={inst['heads']}")
    net = _net(name)
    maxts = []
    for i, (B, L) in enumerate(R.steps_of(case)):
        inp, f64, yard, _e32, scale = R.reference(*((name, B, L) if "steps" in case else (name,)))
        tag = f"{name} {mode} B={B} L={L}" + (f" step {i}" if "steps" in case else "")
        got, fwd, bwd = _step(net, inp)
        _confirm(tag, case, mode, fwd, bwd)
        _hold(tag, got, f64, yard, scale)
        _exact_zero_rows(tag, case, got)
        maxts.append((L, fwd["maxt"]))
    if mode == "default" and name == "lengths_64_128_64":       # the program was rebuilt for every length
        assert maxts[1][1] == 2 * maxts[0][1] and maxts[2][1] == maxts[0][1], maxts


def test_bfloat16_engine_runs_the_same_fp32_program():
    name = "nine_convs_c1_lat2"
    inp, f64, yard, _e32, scale = R.reference(name)
    net = _net(name, dtype="bfloat16")
    got, fwd, bwd = _step(net, inp)
    _confirm(f"{name} bfloat16", R.CASES[name], "default", fwd, bwd)
    _hold(f"{name} bfloat16", got, f64, yard, scale)


def _near(a, b, what):
    """elementwise within 2^-22 of the tensor's largest value: identical terms, the atomics of the windows in another order"""
    for k in b:
        if k.startswith("grad:"):
            m = float(b[k].abs().max())
            d = float((a[k] - b[k]).abs().max())
            assert d <= 2.0 ** -22 * m, f"{what}: {k} differs by {d:.3e} = {d / m:.2e} of its max"


def test_gradients_accumulate_and_do_not_depend_on_need_dx():
    name = "tested_config"
    inp = R.reference(name)[0]
    net = _net(name)
    once, fwd, _b = _step(net, inp)
    assert fwd["thin"] == 1
    twice, _f, _b = _step(net, inp, zero=False)
    _near(twice, {k: 2.0 * v for k, v in once.items()}, "two backward passes without zero_grad")
    nodx, _f, bwd = _step(net, inp, need_dx=False)
    assert bwd["thin"] == 1
    _near(nodx, once, "need_dx=False")


def test_deterministic_mode_is_bit_equal_with_and_without_dx(env_switches):
    env_switches(EEGLDM_DETERMINISTIC="1")
    name = "tested_config"
    inp = R.reference(name)[0]
    net = _net(name)
    a, fwd, bwd = _step(net, inp)
    assert fwd["thin"] == 1 and bwd["thin"] == 1, "the deterministic mode left the whole-network route"
    b, _f, _b = _step(net, inp, need_dx=False)
    c, _f, _b = _step(net, inp)
    for k in b:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), f"{k}: not bit-equal in the deterministic mode"
    assert torch.equal(a["dx"], c["dx"])
