"""Test-local restatement of the class-conditional UNetModel forward (unet.py:512-563 with num_classes set): oracle.unet's pieces plus
the label row, emb = time_embed(t_emb) + label_emb.weight[y] (unet.py:531-533).  Kept out of oracle/ (test helper, not product)."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import unet as U


def cond_param_shapes(cfg):
    """the reference's state_dict keys and shapes, label_emb.weight right after time_embed.2.bias (its named_parameters() order)"""
    out = OrderedDict()
    for k, s in U.unet_param_shapes(cfg).items():
        out[k] = s
        if k == "time_embed.2.bias":
            out["label_emb.weight"] = (cfg["num_classes"], 4 * cfg["model_channels"])
    return out


def unet_forward_cond(sd, cfg, x, t, y):
    mc = cfg["model_channels"]
    ssn = bool(cfg.get("use_scale_shift_norm", False))
    inp, mid, out = U._plan(cfg)
    emb = U.timestep_embedding(t, mc)
    emb = F.linear(emb, sd["time_embed.0.weight"], sd["time_embed.0.bias"])
    emb = F.linear(F.silu(emb), sd["time_embed.2.weight"], sd["time_embed.2.bias"])
    emb = emb + F.embedding(torch.as_tensor(y, dtype=torch.int64), sd["label_emb.weight"])
    hs = []
    h = U.sq(F.conv1d(U.sq(x), U.wq(sd["input_blocks.0.0.weight"]), sd["input_blocks.0.0.bias"], padding=1))
    hs.append(h)
    for i, layers in enumerate(inp[1:], start=1):
        h = U._run_layers(sd, f"input_blocks.{i}.", layers, h, emb, ssn)
        hs.append(h)
    h = U._run_layers(sd, "middle_block.", mid, h, emb, ssn)
    for i, layers in enumerate(out):
        h = torch.cat([h, hs.pop()], dim=1)
        h = U._run_layers(sd, f"output_blocks.{i}.", layers, h, emb, ssn)
    h = U.sq(U._gn(h, sd, "out.0", True))
    return U.sq(F.conv1d(h, U.wq(sd["out.2.weight"]), sd["out.2.bias"], padding=1))
