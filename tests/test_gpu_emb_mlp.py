"""-m gpu: the time-embedding MLP on its purpose-built kernels (csrc/emb_mlp.hip) against float64 numpy.

The chain and its backward run on their own through eegldm_debug_unet_embed / _embed_backward, which call the functions every forward,
the sampler's table and every backward call.  References are float64 restatements inside this file:
  forward   staged: each tensor from the DEVICE's previous tensor (h1 from e0, a1 from h1, emb from a1, semb from emb, emb_all from semb),
            so that a bound speaks about one product / one silu and not about the 6e-5 that one ulp of the fp32 frequency moves cos / sin
            at t ~ 1000; e0 itself against the reference's formula with fp32 frequencies (unet.py:12-36)
  backward  the six (seven) parameter gradients and dsemb from the device tape and demb_all
Bounds: BOUNDS[case][tensor] = 2 x the rel-L2 error of the OLD path (EEGLDM_NO_EMB_MLP=1: general GEMM + element-wise kernels) measured on
MI355X on the same cases, records in profiles/emb_mlp_numerics.txt.  Both are fp32 chains of the same length; the factor covers a
different but fixed summation order.  Where the old path's error is exactly 0 the new one must be 0 as well.

Shapes: model_channels 32, channel_mult [1, 2], one ResBlock per level, no resblock_updown: te = 128 and E = 416 = 6.5 tiles of 64
(832 with use_scale_shift_norm); n = 1, 3, 17, 64 (below, across and exactly one tile of rows); model_channels 128 (te = 512, E = 1664) at
n = 8.  E of every case is asserted below.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from param_gen import gen_param, normal, timesteps  # noqa: E402

BASE = dict(image_size=64, in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=[], channel_mult=[1, 2])
# name -> (constructor arguments, n, E, class labels or None)
CASES = {
    "n1": (BASE, 1, 416, None),
    "n3": (BASE, 3, 416, None),
    "n17": (BASE, 17, 416, None),
    "n64": (BASE, 64, 416, None),
    "te512_n8": (dict(BASE, model_channels=128), 8, 1664, None),
    "labels_n17": (dict(BASE, num_classes=5), 17, 416, [0, 3, 3, 1, 4, 0, 0, 3, 1, 1, 4, 3, 0, 1, 3, 4, 0]),      # class 2 absent
    "ssn_n17": (dict(BASE, use_scale_shift_norm=True), 17, 832, None),
    "table_n5": (BASE, 5, 416, None),      # the rows of a 5-step sampling run (timesteps of make_sampling_scheduler(5))
}
FWD = ("e0", "h1", "a1", "emb", "semb", "emb_all")
BWD = ("g_emb_w", "g_emb_b", "g_te2_w", "g_te2_b", "g_te0_w", "g_te0_b", "dsemb")

# 2 x the old path's measured rel-L2 (profiles/emb_mlp_numerics.txt), per case and tensor
BOUNDS = {
    'n1': {'e0': 4.299e-06, 'h1': 1.904e-07, 'a1': 9.247e-08, 'emb': 3.773e-07, 'semb': 8.558e-08, 'emb_all': 3.810e-07, 'g_emb_b': 0.000e+00, 'g_emb_w': 5.134e-08, 'dsemb': 7.736e-07, 'g_te2_b': 8.007e-07, 'g_te2_w': 8.037e-07, 'g_te0_b': 1.047e-06, 'g_te0_w': 1.050e-06},
    'n3': {'e0': 6.940e-06, 'h1': 1.875e-07, 'a1': 9.349e-08, 'emb': 3.802e-07, 'semb': 8.448e-08, 'emb_all': 3.673e-07, 'g_emb_b': 6.870e-08, 'g_emb_w': 7.166e-08, 'dsemb': 7.817e-07, 'g_te2_b': 8.040e-07, 'g_te2_w': 7.833e-07, 'g_te0_b': 9.277e-07, 'g_te0_w': 8.671e-07},
    'n17': {'e0': 5.829e-06, 'h1': 2.027e-07, 'a1': 9.225e-08, 'emb': 3.786e-07, 'semb': 9.071e-08, 'emb_all': 3.999e-07, 'g_emb_b': 1.239e-07, 'g_emb_w': 1.524e-07, 'dsemb': 7.542e-07, 'g_te2_b': 7.022e-07, 'g_te2_w': 7.459e-07, 'g_te0_b': 7.966e-07, 'g_te0_w': 8.319e-07},
    'n64': {'e0': 5.392e-06, 'h1': 2.156e-07, 'a1': 9.263e-08, 'emb': 3.867e-07, 'semb': 9.708e-08, 'emb_all': 3.907e-07, 'g_emb_b': 1.720e-07, 'g_emb_w': 2.943e-07, 'dsemb': 7.411e-07, 'g_te2_b': 6.195e-07, 'g_te2_w': 7.414e-07, 'g_te0_b': 7.205e-07, 'g_te0_w': 8.484e-07},
    'te512_n8': {'e0': 1.043e-05, 'h1': 4.137e-07, 'a1': 9.682e-08, 'emb': 7.948e-07, 'semb': 9.221e-08, 'emb_all': 7.214e-07, 'g_emb_b': 1.129e-07, 'g_emb_w': 1.062e-07, 'dsemb': 6.122e-07, 'g_te2_b': 6.148e-07, 'g_te2_w': 6.226e-07, 'g_te0_b': 9.763e-07, 'g_te0_w': 1.010e-06},
    'labels_n17': {'e0': 5.829e-06, 'h1': 2.027e-07, 'a1': 9.225e-08, 'emb': 3.713e-07, 'semb': 9.918e-08, 'emb_all': 3.903e-07, 'g_emb_b': 1.239e-07, 'g_emb_w': 1.533e-07, 'dsemb': 7.542e-07, 'g_te2_b': 6.893e-07, 'g_te2_w': 7.357e-07, 'g_te0_b': 7.838e-07, 'g_te0_w': 8.223e-07, 'g_label': 7.358e-07},
    'ssn_n17': {'e0': 5.829e-06, 'h1': 2.027e-07, 'a1': 9.225e-08, 'emb': 3.786e-07, 'semb': 9.071e-08, 'emb_all': 3.958e-07, 'g_emb_b': 1.579e-07, 'g_emb_w': 1.541e-07, 'dsemb': 1.067e-06, 'g_te2_b': 8.966e-07, 'g_te2_w': 1.002e-06, 'g_te0_b': 9.164e-07, 'g_te0_w': 1.044e-06},
    'table_n5': {'e0': 2.228e-06, 'h1': 2.136e-07, 'a1': 9.114e-08, 'emb': 3.758e-07, 'semb': 9.761e-08, 'emb_all': 3.960e-07, 'g_emb_b': 8.575e-08, 'g_emb_w': 8.926e-08, 'dsemb': 7.844e-07, 'g_te2_b': 8.742e-07, 'g_te2_w': 8.226e-07, 'g_te0_b': 9.376e-07, 'g_te0_w': 8.999e-07},
}


@contextlib.contextmanager
def old_path(on):
    from eegldm._lib import lib
    prev = os.environ.get("EEGLDM_NO_EMB_MLP")
    if on:
        os.environ["EEGLDM_NO_EMB_MLP"] = "1"
    else:
        os.environ.pop("EEGLDM_NO_EMB_MLP", None)
    lib.eegldm_debug_reload_env()
    try:
        yield
    finally:
        if prev is None:
            os.environ.pop("EEGLDM_NO_EMB_MLP", None)
        else:
            os.environ["EEGLDM_NO_EMB_MLP"] = prev
        lib.eegldm_debug_reload_env()


def launches(reset=False):
    from eegldm._lib import lib, check
    v = ctypes.c_long()
    check(lib.eegldm_debug_emb_mlp_launches(ctypes.byref(v), 1 if reset else 0))
    return v.value


_NETS = {}


def _net(name):
    """(net, float64 weights, timesteps, labels, demb_all): built once per case"""
    if name in _NETS:
        return _NETS[name]
    from eegldm.models import UNetModel
    kw, n, E, labels = CASES[name]
    net = UNetModel(**kw)
    net.load_state_dict({k: torch.from_numpy(gen_param(31, k, s)) for k, (_o, _n, s) in net.entries.items()})
    sd = net.state_dict()
    rows = sorted((k for k in net.entries if ".emb_layers.1.weight" in k), key=lambda k: net.entries[k][0])
    W = {"w0": sd["time_embed.0.weight"], "b0": sd["time_embed.0.bias"], "w2": sd["time_embed.2.weight"], "b2": sd["time_embed.2.bias"],
         "we": torch.cat([sd[k] for k in rows]), "be": torch.cat([sd[k[:-6] + "bias"] for k in rows])}
    if labels is not None:
        W["label"] = sd["label_emb.weight"]
    W = {k: v.double().cpu().numpy() for k, v in W.items()}
    assert W["we"].shape == (E, 4 * kw["model_channels"]), (name, W["we"].shape)      # the E the constructor reports
    if name == "table_n5":
        from eegldm.sampling import make_sampling_scheduler
        t = make_sampling_scheduler(5).timesteps.cpu().numpy().astype(np.int64)
        assert t.shape == (5,)
    else:
        t = timesteps(n, seed=41)
    _NETS[name] = (net, W, rows, t, labels, normal((n, E), seed=43))
    return _NETS[name]


def run(name, old, backward_calls=1):
    """One forward (+ backward_calls backwards without zeroing in between) of the chain -> dict of float32 numpy arrays"""
    from eegldm._lib import lib, check, ptr
    net, _W, rows, t, labels, demb_all = _net(name)
    kw, n, E, _l = CASES[name]
    mc, te, dev = kw["model_channels"], 4 * kw["model_channels"], net.device
    t_d = torch.from_numpy(t).to(dev)
    lab_d = None if labels is None else torch.tensor(labels, dtype=torch.int64, device=dev)
    table = torch.full((n, E), float("nan"), device=dev); work = torch.full((n * (mc + 4 * te),), float("nan"), device=dev)
    dsemb = torch.full((n, te), float("nan"), device=dev); d_d = torch.from_numpy(demb_all).to(dev)
    with old_path(old):
        check(lib.eegldm_debug_unet_embed(net.h, ptr(t_d), ptr(lab_d), n, ptr(table), ptr(work)))
        net.zero_grad()
        for _ in range(backward_calls):
            check(lib.eegldm_debug_unet_embed_backward(net.h, ptr(lab_d), n, ptr(d_d), ptr(work), ptr(dsemb)))
        torch.cuda.synchronize()
    w = work.cpu().numpy()
    out = {"e0": w[:n * mc].reshape(n, mc)}
    for i, k in enumerate(("h1", "a1", "emb", "semb")):
        out[k] = w[n * mc + i * n * te:n * mc + (i + 1) * n * te].reshape(n, te)
    out["emb_all"] = table.cpu().numpy(); out["dsemb"] = dsemb.cpu().numpy()
    g = net.grad_dict()
    out["g_te0_w"], out["g_te0_b"] = g["time_embed.0.weight"].cpu().numpy(), g["time_embed.0.bias"].cpu().numpy()
    out["g_te2_w"], out["g_te2_b"] = g["time_embed.2.weight"].cpu().numpy(), g["time_embed.2.bias"].cpu().numpy()
    out["g_emb_w"] = torch.cat([g[k] for k in rows]).cpu().numpy(); out["g_emb_b"] = torch.cat([g[k[:-6] + "bias"] for k in rows]).cpu().numpy()
    if labels is not None:
        out["g_label"] = g["label_emb.weight"].cpu().numpy()
    return out


def _silu(z):
    return z / (1.0 + np.exp(-z))


def _dsilu(z):
    s = 1.0 / (1.0 + np.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def reference(name, out):
    """float64: forward staged on the device tensors of `out`, backward from its tape"""
    _net_, W, _rows, t, labels, demb_all = _net(name)
    kw = CASES[name][0]
    mc, d = kw["model_channels"], {k: v.astype(np.float64) for k, v in out.items()}
    half = mc // 2
    freqs = np.exp(np.float32(-np.log(np.float32(10000.0))) * np.arange(half, dtype=np.float32) / np.float32(half)).astype(np.float32)
    args = (t.astype(np.float32)[:, None] * freqs[None]).astype(np.float32).astype(np.float64)
    ref = {"e0": np.concatenate([np.cos(args), np.sin(args)], axis=1)}
    ref["h1"] = d["e0"] @ W["w0"].T + W["b0"]
    ref["a1"] = _silu(d["h1"])
    ref["emb"] = d["a1"] @ W["w2"].T + W["b2"]
    if labels is not None:
        ref["emb"] = ref["emb"] + W["label"][np.asarray(labels)]
    ref["semb"] = _silu(d["emb"])
    ref["emb_all"] = d["semb"] @ W["we"].T + W["be"]
    D = demb_all.astype(np.float64)
    ref["g_emb_b"] = D.sum(0); ref["g_emb_w"] = D.T @ d["semb"]
    ref["dsemb"] = D @ W["we"]
    demb = ref["dsemb"] * _dsilu(d["emb"])
    ref["g_te2_b"] = demb.sum(0); ref["g_te2_w"] = demb.T @ d["a1"]
    dh1 = (demb @ W["w2"]) * _dsilu(d["h1"])
    ref["g_te0_b"] = dh1.sum(0); ref["g_te0_w"] = dh1.T @ d["e0"]
    if labels is not None:
        ref["g_label"] = np.zeros_like(W["label"])
        np.add.at(ref["g_label"], np.asarray(labels), demb)
    return ref


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def errors(name, old):
    out = run(name, old)
    ref = reference(name, out)
    return {k: rel_l2(out[k], ref[k]) for k in ref}, out


_NEW = {}


def new_run(name):      # one run of the new path per case, shared by the tests below
    if name not in _NEW:
        _NEW[name] = errors(name, False)
    return _NEW[name]


def _keys(name, which):
    return which + (("g_label",) if which is BWD and CASES[name][3] is not None else ())


@pytest.mark.parametrize("name", list(CASES))
def test_forward_within_twice_the_old_paths_float64_error(name):
    err, _out = new_run(name)
    print(name, {k: f"{err[k]:.3e}" for k in FWD})
    for k in FWD:
        assert err[k] <= BOUNDS[name][k], f"{name} {k}: rel-L2 {err[k]:.3e} vs bound {BOUNDS[name][k]:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_forward_is_bit_identical_to_the_old_path(name):
    """Measured, not designed: the tile kernel feeds k = 16 g + 4 h + j to MFMA step j exactly like the general GEMM's fp32 fragments, each
    output is one chain over ascending chunks, and bias / label row / silu follow in the old order -- so tape and emb_all keep their bits
    (profiles/emb_mlp_numerics.txt), and with them every forward, evaluation and sampling result."""
    _err, new = new_run(name)
    old = run(name, True)
    for k in FWD:
        assert np.array_equal(new[k], old[k]), f"{name} {k}: {int((new[k] != old[k]).sum())} elements differ from the old path"


@pytest.mark.parametrize("name", list(CASES))
def test_backward_within_twice_the_old_paths_float64_error(name):
    err, _out = new_run(name)
    print(name, {k: f"{err[k]:.3e}" for k in _keys(name, BWD)})
    for k in _keys(name, BWD):
        assert err[k] <= BOUNDS[name][k], f"{name} {k}: rel-L2 {err[k]:.3e} vs bound {BOUNDS[name][k]:.3e}"


@pytest.mark.parametrize("name", ["n17", "te512_n8", "labels_n17", "ssn_n17"])
def test_two_runs_are_bitwise_equal(name):
    """forward and backward, without EEGLDM_DETERMINISTIC: one writer per output, a fixed order"""
    assert not os.environ.get("EEGLDM_DETERMINISTIC")
    _err, a = new_run(name)
    b = run(name, False)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{name} {k} differs between two runs"


@pytest.mark.parametrize("name", ["n17", "labels_n17"])
def test_backward_accumulates(name):
    """two backward calls without zeroing: twice the gradient.  The second call adds the same bits to a buffer that holds them (0 + g = g
    exactly), and g + g is exact in binary floating point, so "within fp32 rounding" is equality here."""
    _err, a = new_run(name)
    b = run(name, False, backward_calls=2)
    for k in _keys(name, BWD):
        if k != "dsemb":
            assert np.array_equal(b[k], 2.0 * a[k]), f"{name} {k}: max |g2 - 2 g1| {np.abs(b[k] - 2.0 * a[k]).max():.3e}"
    assert np.array_equal(b["dsemb"], a["dsemb"])      # written, not accumulated


@pytest.mark.parametrize("tile", ["32", "64"])
@pytest.mark.parametrize("name", ["n3", "n64", "te512_n8", "labels_n17"])
def test_both_tile_sizes_give_the_same_bits(name, tile):
    """Products of fewer than 128 tiles of 64 x 64 run on 32 x 32 tiles; the k order of an output does not depend on the tile, so forcing
    either size (EEGLDM_EMB_MLP_TILE) must reproduce the default run bit for bit -- forward and backward -- on shapes where the default
    mixes both."""
    _err, a = new_run(name)
    os.environ["EEGLDM_EMB_MLP_TILE"] = tile
    try:
        b = run(name, False)
    finally:
        os.environ.pop("EEGLDM_EMB_MLP_TILE", None)
        from eegldm._lib import lib
        lib.eegldm_debug_reload_env()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{name} {k}: tile {tile} differs from the default"


def test_switch_runs_the_old_kernels():
    launches(reset=True)
    run("n17", True)
    assert launches() == 0, "EEGLDM_NO_EMB_MLP=1 still launched the purpose-built kernels"
    run("n17", False)
    assert launches() == 3 + 5, launches()      # forward: three products; backward: two weight-gradient launches, partials, fold, dh1
    launches(reset=True)
    run("labels_n17", False)
    assert launches() == 3 + 5      # the label-embedding gradient stays on ew_label_emb_grad


def test_sampler_table_runs_the_new_kernels_and_is_reproducible():
    """5-step DDIM run through the public entry: the table of embedding rows is computed once, by the three forward launches; a seeded run
    repeats bit for bit; the old path's samples agree to 1e-4 rel-L2 (each path lies within 5e-5 of the fp32 oracle,
    tests/test_gpu_sampling.py)."""
    from eegldm.sampling import ddim_sample, make_sampling_scheduler
    net = _net("table_n5")[0]
    noise = torch.from_numpy(normal((2, 1, 64), seed=47))
    launches(reset=True)
    with old_path(False):
        a, _z = ddim_sample(net, None, make_sampling_scheduler(5), noise, crop=0)
        assert launches() == 3, launches()
        b, _z = ddim_sample(net, None, make_sampling_scheduler(5), noise, crop=0)
    with old_path(True):
        c, _z = ddim_sample(net, None, make_sampling_scheduler(5), noise, crop=0)
    assert torch.equal(a, b)
    r = rel_l2(a.cpu().numpy(), c.cpu().numpy())
    print("sampler new vs old rel-L2", r)
    assert r < 1e-4
