"""CPU: the reference side of tests/test_gpu_aekl_thin_rounding.py (tests/aekl_thin_reference.py) is itself pinned -- the float64 oracle
against the committed golden of the reference's own autoencoder, the determinism of the generated cases, the case matrix against a
restatement of csrc/aekl.hip::thin_eligible, and the float32 yardstick of every case."""
import os

import numpy as np
import pytest
import torch

import aekl_thin_reference as R
from oracle import aekl as A
from param_gen import gen_param, normal, eeg_windows

ALL_PAIRS = [(a, b) for a in (1, 2, 4) for b in (1, 2, 4)]


def test_float64_oracle_reproduces_the_one_group_golden(golden_dir):
    """oracle/aekl.py in float64 at [32,32,64], G = 1 against aekl_twin_32_32_64_g1.npz (the reference's local autoencoder, fp32), within the
    tolerances tests/test_oracle_golden.py holds the fp32 oracle to."""
    g = np.load(os.path.join(golden_dir, "aekl_twin_32_32_64_g1.npz"))
    nc = [int(v) for v in g["num_channels"]]; B, L = int(g["B"]), int(g["L"])
    cfg = dict(num_channels=nc, latent_channels=1, in_channels=1, out_channels=1, num_res_blocks=2, norm_num_groups=1)
    sw, sx, se, sdy = [int(v) for v in g["seeds"]]
    shapes = A.aekl_param_shapes(cfg)
    assert list(shapes.keys()) == [str(k) for k in g["keys"]]
    inp = dict(cfg=cfg, sd={k: gen_param(sw, k, s) for k, s in shapes.items()}, x=eeg_windows(B, seed=sx, length=L, pad=8),
               eps=normal((B, 1, L // 4), seed=se), dy=normal((B, 1, L), seed=sdy), kl_weight=0.3, d_mu=None, d_sigma=None)
    r = R.run_oracle(inp, torch.float64)
    assert r["recon"].dtype == torch.float64 and all(v.dtype == torch.float64 for v in r["grads"].values())
    np.testing.assert_allclose(r["recon"].numpy(), g["recon"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(r["z_mu"].numpy(), g["z_mu"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(r["z_sigma"].numpy(), g["z_sigma"], rtol=2e-4, atol=2e-5)
    assert abs(float(r["kl"]) - float(g["kl"])) < 1e-5 * abs(float(g["kl"]))
    np.testing.assert_allclose(r["dx"].numpy(), g["dx"], rtol=2e-3, atol=2e-4)
    gscale = max(float(g["g_l2:" + k]) for k in shapes)
    for k in shapes:
        gr = r["grads"][k].reshape(-1); l2 = float(g["g_l2:" + k])
        assert abs(float(gr.norm()) - l2) <= 1e-3 * l2 + 1e-5 * gscale, k
        np.testing.assert_allclose(gr[:16].numpy(), g["g_head:" + k], rtol=2e-3, atol=2e-4 * max(1.0, gscale / 100))


def test_backward_ex_scalar_matches_hand_written_gradients():
    """The scalar's d_mu / d_sigma / clamp terms: on a case whose latent channel 0 is clamped, the log-variance head's row 0 gets exactly
    zero gradient, row 1 does not, and removing <z_mu, d_mu> + <z_sigma, d_sigma> changes the heads' gradients."""
    for name in ("backward_ex_low_clamp", "backward_ex_high_clamp"):
        inp = R.make_inputs(name)
        r = R.run_oracle(inp, torch.float64)
        gw, gb = r["grads"]["quant_conv_log_sigma.conv.weight"], r["grads"]["quant_conv_log_sigma.conv.bias"]
        assert float(gw[0].abs().max()) == 0.0 and float(gb[0].abs()) == 0.0
        assert float(gw[1].abs().max()) > 0.0 and float(gb[1].abs()) > 0.0
        lv_edge = -30.0 if "low" in name else 20.0
        assert torch.allclose(r["z_sigma"][:, 0], torch.full_like(r["z_sigma"][:, 0], float(np.exp(lv_edge / 2))), rtol=1e-12, atol=0)
        plain = R.run_oracle(dict(inp, d_mu=None, d_sigma=None), torch.float64)
        assert float((plain["grads"]["quant_conv_mu.conv.bias"] - r["grads"]["quant_conv_mu.conv.bias"]).abs().max()) > 1e-3
        assert float((plain["grads"]["quant_conv_log_sigma.conv.bias"][1] - gb[1]).abs()) > 1e-3
        # d/d bias_mu[c] = sum (dz + d_mu + kl_weight / B * mu): the d_mu share is the plain sum of d_mu over the channel
        want = torch.from_numpy(inp["d_mu"]).double().sum(dim=(0, 2))
        got = r["grads"]["quant_conv_mu.conv.bias"] - plain["grads"]["quant_conv_mu.conv.bias"]
        assert torch.allclose(got, want, rtol=1e-9, atol=1e-9)


def test_case_generation_is_deterministic():
    for name in ("nine_convs_c1_lat2", "outlier_first_element", "backward_ex_high_clamp"):
        a, b = R.make_inputs(name), R.make_inputs(name)
        for k in ("x", "eps", "dy"):
            assert np.array_equal(a[k], b[k]) and a[k].dtype == np.float32
        assert list(a["sd"]) == list(b["sd"]) and all(np.array_equal(a["sd"][k], b["sd"][k]) for k in a["sd"])
    inp = R.make_inputs("tested_config")
    # GroupNorm scales away from 1 and shifts away from 0: a kernel that dropped either would not pass
    for k, v in inp["sd"].items():
        if v.ndim == 1 and ("norm" in k or k.count(".") == 3):
            assert float(np.abs(v - (1.0 if k.endswith("weight") else 0.0)).max()) > 1e-2, k
    spike = R.make_inputs("outlier_first_element")
    assert np.array_equal(spike["x"][1:], inp["x"][1:]) and np.array_equal(spike["x"][0, 0, 2:], inp["x"][0, 0, 2:])
    assert float(spike["x"][0, 0, 0]) > 150 * float(inp["x"][0].std())


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_matrix_matches_the_acceptance_rule(name):
    case = R.CASES[name]; cfg = R.cfg_of(case)
    shapes = A.aekl_param_shapes(cfg)
    nparams = R.engine_nparams(shapes)
    assert nparams <= R.THIN_MAX_PARAMS
    levels = len(cfg["num_channels"])
    for _B, L in R.steps_of(case):
        assert L % (1 << (levels - 1)) == 0, "the model itself refuses this length"
        assert R.thin_eligible(cfg, L, nparams) == (case["route"] in (R.THIN, R.EDGE)), (name, L)
    inst = R.instantiations(cfg)
    print(f"[matrix] {name}: nparams {nparams} convs {inst['convs']} norms {inst['norms']} heads LAT={inst['heads']}")


def test_acceptance_edges_sit_where_the_table_says():
    e, p = R.CASES["edge_accepted"], R.CASES["edge_refused"]
    assert max(e["num_channels"]) * e["L"] == R.THIN_MAX_FLOATS - 1024
    assert max(p["num_channels"]) * p["L"] > R.THIN_MAX_FLOATS - 1024 and (p["L"] >> 2) % 4 == 0      # refused by the size rule alone
    r = R.CASES["rows_not_float4"]
    assert (r["L"] >> 2) % 4 != 0 and r["L"] % 4 == 0 and max(r["num_channels"]) * r["L"] < R.THIN_MAX_FLOATS - 1024
    q = R.CASES["one_quad_past_a_pass"]
    assert q["L"] // 4 == 512 + 4 and ((q["L"] >> 2) // 4) % 2 == 1
    s = R.CASES["smallest_length"]
    assert (s["L"] >> 2) == 4 and not R.thin_eligible(R.cfg_of(s), s["L"] - 4, 0)


def test_the_mixed_rows_reach_every_instantiation():
    thin = [n for n, c in R.CASES.items() if c["route"] != R.FALLBACK]
    convs, norms, heads = set(), set(), set()
    for n in ("nine_convs_c1_lat2", "wide_lat4_nrb3"):
        inst = R.instantiations(R.cfg_of(R.CASES[n]))
        convs.update(inst["convs"]); norms.update(inst["norms"]); heads.add(inst["heads"])
    assert sorted(convs) == ALL_PAIRS, sorted(set(ALL_PAIRS) - convs)
    assert set(R.instantiations(R.cfg_of(R.CASES["nine_convs_c1_lat2"]))["convs"]) == set(ALL_PAIRS)
    for n in thin:
        inst = R.instantiations(R.cfg_of(R.CASES[n]))
        norms.update(inst["norms"]); heads.add(inst["heads"])
    assert sorted(norms) == [1, 2, 4] and sorted(heads) == [1, 2, 4]


def test_instantiations_agree_with_the_parameter_shapes():
    """every conv weight of the state dict is one of the derived pairs, and every pair has a weight"""
    for name, case in R.CASES.items():
        cfg = R.cfg_of(case)
        shapes = A.aekl_param_shapes(cfg)
        pairs = {(s[1], s[0]) for k, s in shapes.items() if len(s) == 3 and not k.startswith("quant_conv_")}
        assert pairs == set(R.instantiations(cfg)["convs"]), name


@pytest.mark.parametrize("name", list(R.CASES))
def test_fp32_oracle_is_finite_and_the_yardstick_is_positive(name):
    case = R.CASES[name]
    for B, L in R.steps_of(case):
        args = (name, B, L) if "steps" in case else (name,)
        inp, f64, yard, e32, scale = R.reference(*args)
        assert set(yard) == set(f64) == set(scale) and len(f64) == 5 + len(inp["sd"])
        van = set(R.vanishing_grads(inp["cfg"]))
        assert van <= set(f64)
        for k, y in yard.items():
            assert np.isfinite(e32[k]) and y >= R.FLOOR and y < 1e-3, (k, e32[k])       # fp32 arithmetic, not a different function
            # the structural list of analytically zero gradients is exactly the set of tensors that are rounding noise in float64
            assert (float(f64[k].abs().max()) < 2.0 ** -40 * scale[k]) == (k in van), (k, float(f64[k].abs().max()), scale[k])
            assert scale[k] > 0.0
        worst = max(e32, key=e32.get)
        print(f"[yardstick] {name} B={B} L={L}: fp32 oracle worst {worst} {e32[worst]:.2e}; {sum(e <= R.FLOOR for e in e32.values())} of {len(e32)} tensors on the floor")


def test_vanishing_gradients_are_the_one_channel_norm_biases():
    assert R.vanishing_grads(R.cfg_of(R.CASES["tested_config"])) == [] and R.vanishing_grads(R.cfg_of(R.CASES["wide_lat4_nrb3"])) == []
    assert R.vanishing_grads(R.cfg_of(R.CASES["nine_convs_c1_lat2"])) == [
        "grad:encoder.blocks.1.conv1.conv.bias", "grad:decoder.blocks.5.conv1.conv.bias", "grad:decoder.blocks.5.conv2.conv.bias",
        "grad:decoder.blocks.5.nin_shortcut.conv.bias"]


def test_tensor_classes():
    assert R.tensor_class("recon") == "recon" and R.tensor_class("grad:quant_conv_mu.conv.weight") == "grad heads"
    assert R.tensor_class("grad:encoder.blocks.1.norm2.bias") == "grad norm.bias" and R.tensor_class("grad:decoder.blocks.9.weight") == "grad norm.weight"
    assert R.tensor_class("grad:encoder.blocks.3.conv.conv.weight") == "grad conv.weight" and R.tensor_class("grad:encoder.blocks.0.conv.bias") == "grad conv.bias"
    assert R.tensor_class("grad:decoder.blocks.3.nin_shortcut.conv.weight") == "grad shortcut.weight"
    assert R.tensor_class("grad:post_quant_conv.conv.bias") == "grad post_quant"


def test_rel_err():
    t64 = torch.tensor([1.0, -4.0, 0.0], dtype=torch.float64)
    assert R.rel_err(torch.tensor([1.0, -4.0, 0.5]), t64) == 0.125
    assert R.rel_err(torch.zeros(2), torch.zeros(2, dtype=torch.float64)) == 0.0
    assert R.rel_err(torch.tensor([1e-9, 0.0]), torch.zeros(2, dtype=torch.float64)) == float("inf")
    assert R.rel_err(torch.tensor([float("nan"), 0.0]), torch.ones(2, dtype=torch.float64)) == float("inf")
