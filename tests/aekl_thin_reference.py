"""Reference side of the whole-network AutoencoderKL tests (csrc/aekl_thin.hip and the program builder in csrc/aekl.hip).

The reference is oracle/aekl.py run in float64 (its `sq` / `wq` storage points are the identity outside the storage emulation) on the
float32 parameters and inputs the engine gets.  The gradients are autograd of the scalar
    <recon, dy> + <z_mu, d_mu> + <z_sigma, d_sigma> + kl_weight * KL
with the KL of oracle/losses.py::kl_loss and the clamp(-30, 20) of oracle/aekl.py::encode -- what eegldm_aekl_backward (d_mu = d_sigma =
none) and eegldm_aekl_backward_ex compute.  The same function run in float32 on the CPU is the yardstick of the GPU test: an engine tensor
may be 8 x as far from the float64 result as aten's own float32 arithmetic is (tests/test_gpu_aekl_thin_rounding.py).

Nothing here touches the device; tests/test_aekl_thin_numerics_cpu.py pins this file itself.
"""
import functools
from collections import OrderedDict

import numpy as np
import torch

from oracle import aekl as A
from oracle import losses as Ls
from param_gen import gen_param, normal, eeg_windows

# restated from csrc/aekl_thin.h and csrc/aekl.hip::thin_eligible
THIN_MAX_FLOATS = 9216
THIN_MAX_PARAMS = 4096
THIN_CHANNELS = (1, 2, 4)

FLOOR = 2.0 ** -20          # 16 fp32 epsilons of the tensor's scale
FACTOR = 8.0

THIN, FALLBACK, EDGE = "thin", "fallback", "edge"     # EDGE: accepted by thin_eligible; the LDS footprint check of thin_upload decides


def _case(nc, io, nrb, L, B=3, route=THIN, **kw):
    return dict(num_channels=list(nc), in_channels=io[0], out_channels=io[1], latent_channels=io[2], num_res_blocks=nrb, L=L, B=B, route=route, **kw)


# name -> case.  `steps`: (B, L) of consecutive calls on ONE net where the case is a sequence.
CASES = OrderedDict([
    ("tested_config", _case([2, 2, 4], (1, 1, 1), 2, 512)),
    ("smallest_length", _case([2, 2, 4], (1, 1, 1), 2, 16)),                      # bottom level: one float4 per row
    ("nine_convs_c1_lat2", _case([1, 2, 4], (4, 4, 2), 1, 64)),
    ("wide_lat4_nrb3", _case([4, 4, 4], (2, 2, 4), 3, 64)),
    ("two_levels", _case([2, 4], (1, 1, 1), 2, 40)),
    ("four_levels", _case([1, 2, 2, 4], (1, 1, 1), 1, 96)),
    ("one_quad_past_a_pass", _case([2, 2, 4], (1, 1, 1), 2, 2064, B=1)),          # L / 4 = 516 = 512 threads + 4; 129 quads per row at the bottom
    ("edge_accepted", _case([4, 4, 4], (1, 1, 1), 1, 2048, B=1, route=EDGE)),     # 4 L = THIN_MAX_FLOATS - 1024 exactly
    ("edge_refused", _case([4, 4, 4], (1, 1, 1), 1, 2064, B=1, route=FALLBACK)),
    ("rows_not_float4", _case([2, 2, 4], (1, 1, 1), 2, 24, route=FALLBACK)),      # (L >> 2) % 4 != 0
    ("outlier_first_element", _case([2, 2, 4], (1, 1, 1), 2, 512, spike=200.0)),
    # the same spike on a whole 30-s window: the cancellation of a one-pass variance about an outlying first element grows with the number of
    # values behind it (relative error of the variance ~ eps * n / (elements the spike reaches)), so only the production length shows it in full
    ("outlier_first_element_full_window", _case([2, 2, 4], (1, 1, 1), 2, 3072, B=1, spike=200.0)),
    ("backward_ex_low_clamp", _case([2, 2, 4], (1, 1, 2), 2, 64, ex=True, kl_weight=0.3, lv_bias0=-45.0)),
    ("backward_ex_high_clamp", _case([2, 2, 4], (1, 1, 2), 2, 64, ex=True, kl_weight=0.3, lv_bias0=35.0)),
    ("batch_1_then_5", _case([2, 2, 4], (1, 1, 1), 2, 64, steps=[(1, 64), (5, 64)])),
    ("lengths_64_128_64", _case([2, 2, 4], (1, 1, 1), 2, 64, steps=[(3, 64), (3, 128), (3, 64)])),
])
PARAM_SEED = 57
KL_WEIGHT = 0.3


def cfg_of(case):
    return dict(num_channels=case["num_channels"], in_channels=case["in_channels"], out_channels=case["out_channels"],
                latent_channels=case["latent_channels"], num_res_blocks=case["num_res_blocks"], norm_num_groups=1)


def steps_of(case):
    return case.get("steps") or [(case["B"], case["L"])]


def engine_nparams(shapes):
    """The engine lays every tensor out at a multiple of 8 floats (csrc/aekl.hip::Layout)."""
    return sum((int(np.prod(s)) + 7) // 8 * 8 for s in shapes.values())


def thin_eligible(cfg, L, nparams):
    """csrc/aekl.hip::thin_eligible, restated (without the EEGLDM_AEKL_NO_THIN switch)."""
    nc = cfg["num_channels"]; levels = len(nc)
    if cfg.get("norm_num_groups", 1) != 1:
        return False
    if any(c not in THIN_CHANNELS for c in (cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"], *nc)):
        return False
    if (L >> (levels - 1)) % 4 != 0:
        return False
    mx = max(c * (L >> i) for i, c in enumerate(nc))
    return mx <= THIN_MAX_FLOATS - 1024 and nparams <= THIN_MAX_PARAMS and cfg["in_channels"] * L <= THIN_MAX_FLOATS and L % (1 << (levels - 1)) == 0


def instantiations(cfg):
    """What the whole-network program of `cfg` instantiates: the (cin, cout) pairs of its convs (f_conv_t / b_conv_t), the channel counts of
    its GroupNorms (f_gn_t / b_gn_t) and its latent-head width (f_heads_t / b_heads_t), derived from the block plan."""
    enc, dec = A.aekl_plan(cfg["num_channels"], cfg["num_res_blocks"])
    lat = cfg["latent_channels"]
    convs, norms = set(), set()
    for plan, first_in, last_out in ((enc, cfg["in_channels"], lat), (dec, lat, cfg["out_channels"])):
        for kind, ci, co in plan:
            if kind == "conv3":
                convs.add((first_in if ci is None else ci, last_out if co is None else co))
            elif kind == "res":
                norms.update((ci, co)); convs.update(((ci, co), (co, co)))          # conv1 (and the 1x1 shortcut when ci != co), conv2
            elif kind in ("down", "up"):
                convs.add((ci, co))
            elif kind == "gn":
                norms.add(ci)
    convs.add((lat, lat))                                                           # post_quant_conv
    return dict(convs=sorted(convs), norms=sorted(norms), heads=lat)


def make_inputs(name, B=None, L=None):
    """float32 parameters and inputs of a case (of one step of it), deterministic in (name, B, L)."""
    case = CASES[name]; cfg = cfg_of(case)
    B = case["B"] if B is None else B; L = case["L"] if L is None else L
    shapes = A.aekl_param_shapes(cfg)
    sd = OrderedDict((k, gen_param(PARAM_SEED, k, s)) for k, s in shapes.items())
    if "lv_bias0" in case:                           # every log-variance of latent channel 0 lies past one clamp edge
        sd["quant_conv_log_sigma.conv.bias"][0] = case["lv_bias0"]
    cin, cout, lat = cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"]
    Ll = L >> (len(cfg["num_channels"]) - 1)
    pad = min(8, L // 8)
    x = np.concatenate([eeg_windows(B, seed=100 + c, length=L, pad=pad) for c in range(cin)], axis=1) + 0.05 * normal((B, cin, L), seed=25)
    if "spike" in case:                              # an artefact on the first two samples of window 0 only
        x[0, 0, 0:2] += case["spike"] * float(x[0].std())
    out = dict(cfg=cfg, B=B, L=L, Ll=Ll, sd=sd, x=x.astype(np.float32), eps=normal((B, lat, Ll), seed=26), dy=normal((B, cout, L), seed=27),
               kl_weight=case.get("kl_weight", KL_WEIGHT), d_mu=None, d_sigma=None)
    if case.get("ex"):
        out["d_mu"] = normal((B, lat, Ll), seed=28); out["d_sigma"] = normal((B, lat, Ll), seed=29)
    return out


def run_oracle(inp, dtype):
    """oracle/aekl.py forward + autograd in `dtype`; every result as a float64 tensor: recon, z_mu, z_sigma, kl, dx, and `grads` by key."""
    t = lambda a: torch.from_numpy(a).to(dtype)
    sd = {k: t(v).requires_grad_(True) for k, v in inp["sd"].items()}
    x = t(inp["x"]).requires_grad_(True)
    recon, mu, sg = A.forward(sd, inp["cfg"], x, t(inp["eps"]))
    kl = Ls.kl_loss(mu, sg)
    loss = (recon * t(inp["dy"])).sum() + inp["kl_weight"] * kl
    if inp["d_mu"] is not None:
        loss = loss + (mu * t(inp["d_mu"])).sum() + (sg * t(inp["d_sigma"])).sum()
    loss.backward()
    d = lambda v: v.detach().double()
    return dict(recon=d(recon), z_mu=d(mu), z_sigma=d(sg), kl=d(kl).reshape(1), dx=d(x.grad), grads=OrderedDict((k, d(v.grad)) for k, v in sd.items()))


def flatten(res):
    """name -> tensor over everything a case compares"""
    out = OrderedDict((k, res[k]) for k in ("recon", "z_mu", "z_sigma", "kl", "dx"))
    for k, v in res["grads"].items():
        out["grad:" + k] = v
    return out


def rel_err(t, t64, scale=None):
    """e(t) = max |t - t64| / max |t64| over the whole tensor (0 / 0 = 0: a tensor that must vanish and does); `scale` replaces the
    denominator for the tensors of vanishing_grads()"""
    t = torch.as_tensor(t).detach().double().cpu().reshape(t64.shape)
    num = float((t - t64).abs().max()); den = float(t64.abs().max()) if scale is None else float(scale)
    if not np.isfinite(num):
        return float("inf")
    return 0.0 if num == 0.0 else (num / den if den > 0.0 else float("inf"))


def vanishing_grads(cfg):
    """Gradients that are exactly zero in exact arithmetic: the bias of a conv whose output reaches the loss only through a ONE-channel
    GroupNorm(G = 1) -- a constant added to the norm's only channel is removed by its mean.  These are conv1.bias of a ResBlock with one output
    channel (consumer: norm2) and, where the last level has one channel, conv2.bias / nin_shortcut.bias of the last ResBlock (consumer: the final
    norm).  Their float64 value is rounding noise (1e-15), so max |t64| is no scale: the error of such a tensor is measured against the largest
    gradient of its own class in the same case instead -- the terms that cancel in it are of that size, and so is their rounding error."""
    out = []
    for prefix, plan in zip(("encoder", "decoder"), A.aekl_plan(cfg["num_channels"], cfg["num_res_blocks"])):
        for i, (kind, ci, co) in enumerate(plan):
            if kind == "res" and co == 1:
                out.append(f"grad:{prefix}.blocks.{i}.conv1.conv.bias")
                if plan[i + 1][0] == "gn":
                    out.append(f"grad:{prefix}.blocks.{i}.conv2.conv.bias")
                    if ci != co:
                        out.append(f"grad:{prefix}.blocks.{i}.nin_shortcut.conv.bias")
    return out


def scales(cfg, f64):
    """name -> denominator of e(t): max |t64|, or the class maximum for the tensors of vanishing_grads()"""
    cls = {}
    for k, v in f64.items():
        c = tensor_class(k); cls[c] = max(cls.get(c, 0.0), float(v.abs().max()))
    van = set(vanishing_grads(cfg))
    return OrderedDict((k, cls[tensor_class(k)] if k in van else float(v.abs().max())) for k, v in f64.items())


def tensor_class(name):
    if not name.startswith("grad:"):
        return name
    k = name[5:]
    if k.startswith("quant_conv_"):
        return "grad heads"
    if k.startswith("post_quant_conv"):
        return "grad post_quant"
    if ".norm" in k or k.count(".") == 3 and ".conv." not in k:          # ResBlock norms and the final norms (encoder.blocks.N.weight)
        return "grad norm." + k.rsplit(".", 1)[1]
    if ".nin_shortcut." in k:
        return "grad shortcut." + k.rsplit(".", 1)[1]
    return "grad conv." + k.rsplit(".", 1)[1]


@functools.lru_cache(maxsize=None)
def reference(name, B=None, L=None):
    """(inputs, float64 results, yardstick, fp32 errors, denominators) of one step of a case, computed once per process and shared: yardstick[name] =
    max(e(float32 CPU oracle), FLOOR) per tensor.  Callers must not modify what they get."""
    inp = make_inputs(name, B, L)
    r64 = run_oracle(inp, torch.float64); r32 = run_oracle(inp, torch.float32)
    f64, f32 = flatten(r64), flatten(r32)
    for k, v in f32.items():
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(f64[k]).all()), f"{name}: non-finite oracle tensor {k}"
    scale = scales(inp["cfg"], f64)
    e32 = OrderedDict((k, rel_err(f32[k], f64[k], scale[k])) for k in f64)
    yard = OrderedDict((k, max(e, FLOOR)) for k, e in e32.items())
    return inp, f64, yard, e32, scale
