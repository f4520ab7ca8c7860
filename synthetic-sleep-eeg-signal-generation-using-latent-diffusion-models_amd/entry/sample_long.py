"""Long synthetic recordings: overlapped-window sampling on one latent canvas (sampling.sample_long), so that minutes of EEG that follow a
hypnogram come out as ONE signal instead of concatenated 30-s windows.  Models, configs, EMA, label, guidance and sampler flags are those
of sample_trials.py (--pixel: the pixel-space model of sample_trials_dm.py, --config_file instead of the two LDM configs); the sampler
is DPM-Solver++ (--solver_order 1 = DDIM on the same grid).  Length: --n_windows W, or --minutes X (the smallest W whose recording is at
least that long).  --margin / --ramp are in latent positions (window samples with --pixel); the defaults are sample_long's.
--hypnogram stages.npy holds one stage per 30-s epoch: window k takes the stage at its centre time; --class_label gives every window the
same stage.  Writes long_{seed}.npy (1, 1, samples: the recording with crop 36 off both ends), long_{seed}_labels.npy (one class per
window; only for a class-conditional UNet) and long_{seed}_layout.json (window starts, margin, ramp, stride and the seam spans in samples of
the written recording -- what tools/seam_report.py reads)."""
import argparse
import json
import math
import os

import numpy as np
import torch

from ..models import AutoencoderKL, UNetModel
from ..sampling import long_layout, make_sampling_scheduler, sample_long, window_labels_from_hypnogram
from ..training import randn
from .common import context_model_kwargs, load_config

WINDOW = 3072
SFREQ = 100.0           # 3072 samples are the 30-s epoch plus the 36-sample border pad on both sides
CROP = 36


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--output_dir", required=True); p.add_argument("--diffusion_path", required=True)
    p.add_argument("--best_model_path", default=None); p.add_argument("--autoencoderkl_config_file_path", default=None)
    p.add_argument("--ldm_config_file_path", default=None)
    p.add_argument("--pixel", action="store_true", help="the pixel-space diffusion model (no autoencoder); needs --config_file")
    p.add_argument("--config_file", default=None)
    p.add_argument("--minutes", type=float, default=None, help="length of the recording; rounded up to whole windows")
    p.add_argument("--n_windows", type=int, default=None)
    p.add_argument("--margin", type=int, default=None, help="zero-weight positions at a window edge that has a neighbour (default 2 * 36 / down)")
    p.add_argument("--ramp", type=int, default=None, help="positions of the linear cross-fade (default 4 * 36 / down)")
    p.add_argument("--hypnogram", default=None, help=".npy / text file, one sleep stage per 30-s epoch")
    p.add_argument("--class_label", type=int, default=None, help="the sleep stage of every window (W 0, N1 1, N2 2, N3 3, REM 4)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--guidance_scale", type=float, default=7.0); p.add_argument("--num_inference_steps", type=int, default=20)
    p.add_argument("--spe", default="no-spectral"); p.add_argument("--latent_channels", type=int, default=1)
    p.add_argument("--type_dataset", default="edfx")
    p.add_argument("--prediction_type", default="v_prediction")
    p.add_argument("--dtype", default="float32")
    p.add_argument("--num_classes", type=int, default=None, help="class-conditional UNet (overrides unet_config.params.num_classes)")
    p.add_argument("--null_class", type=int, default=None, help="classifier-free guidance: the unconditional class; --guidance_scale "
                   "applies to a class-conditional UNet only when it is given")
    p.add_argument("--use_ema", action="store_true", help="sample from best_model_ema.pth (a run trained with --ema_decay) instead of best_model.pth")
    p.add_argument("--sampler", default="dpmpp_2m", choices=["dpmpp_2m"], help="the canvas step is the multistep form; --solver_order 1 is DDIM")
    p.add_argument("--solver_order", type=int, default=2, choices=[1, 2])
    return p.parse_args(argv)


def check_args(args):
    if (args.minutes is None) == (args.n_windows is None):
        raise ValueError("pass exactly one of --minutes and --n_windows")
    if args.minutes is not None and not args.minutes > 0:
        raise ValueError("--minutes must be > 0")
    if args.n_windows is not None and args.n_windows < 1:
        raise ValueError("--n_windows must be >= 1")
    if args.hypnogram is not None and args.class_label is not None:
        raise ValueError("pass --hypnogram or --class_label, not both")
    if args.pixel:
        if not args.config_file:
            raise ValueError("--pixel needs --config_file")
    elif not (args.best_model_path and args.autoencoderkl_config_file_path and args.ldm_config_file_path):
        raise ValueError("the LDM needs --best_model_path, --autoencoderkl_config_file_path and --ldm_config_file_path (or pass --pixel)")


def plan_layout(args, window_len, down):
    """-> the LongLayout of the run at the sampler's resolution (window_len positions per window, `down` samples per position)"""
    m = 2 * CROP // down if args.margin is None else args.margin
    r = 4 * CROP // down if args.ramp is None else args.ramp
    if args.n_windows is not None:
        return long_layout(args.n_windows, window_len, m, r)
    one = long_layout(1, window_len, m, r)
    need = args.minutes * 60.0 * SFREQ + 2 * CROP           # samples of the uncropped recording
    W = max(1, math.ceil((need / down - window_len) / one.stride) + 1)
    return long_layout(W, window_len, m, r)


def load_hypnogram(path):
    st = np.load(path) if path.endswith(".npy") else np.loadtxt(path, dtype=np.int64, ndmin=1)
    return np.asarray(st, np.int64).reshape(-1)


def layout_json(lay, down, crop=CROP):
    """The layout in samples of the written (cropped) recording."""
    w = lay.scaled(down)
    return {"n_windows": w.n_windows, "window_len": w.window_len, "m": w.margin, "r": w.ramp, "S": w.stride, "crop": crop, "down": down,
            "sfreq": SFREQ, "samples": w.canvas_len - 2 * crop, "starts": [s - crop for s in w.starts],
            "seams": [[a - crop, b - crop] for a, b in w.seams()]}


def main(args):
    check_args(args)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    name = f"long_dm_{args.spe}_{args.type_dataset}" if args.pixel else f"long_ldm_{args.latent_channels}_{args.spe}_{args.type_dataset}"
    out = os.path.join(args.output_dir, name)
    os.makedirs(out, exist_ok=True)
    stage1, scale_factor = None, 1.0
    if args.pixel:
        up = dict(load_config(args.config_file)["model"]["params"]["unet_config"]["params"])
        up["in_channels"] = up["out_channels"] = 1
        window_len, down = WINDOW, 1
    else:
        ae_cfg = dict(load_config(args.autoencoderkl_config_file_path).autoencoderkl.params)
        ae_cfg.setdefault("num_channels", [32, 32, 64]); ae_cfg["latent_channels"] = args.latent_channels
        stage1 = AutoencoderKL(**ae_cfg, dtype=args.dtype, device=local)
        stage1.load_state_dict(torch.load(os.path.join(args.best_model_path, "best_model.pth"), map_location="cpu"))
        up = dict(load_config(args.ldm_config_file_path)["model"]["params"]["unet_config"]["params"])
        up["in_channels"] = up["out_channels"] = args.latent_channels
        scale_factor = float(torch.load(os.path.join(args.diffusion_path, "checkpoint.pth"), map_location="cpu")["scale_factor"])
        down = stage1.down
        window_len = WINDOW // down
    lay = plan_layout(args, window_len, down)
    if args.num_classes is not None:
        up["num_classes"] = args.num_classes
    labels = None
    if up.get("num_classes") is not None:
        if args.hypnogram:
            labels = window_labels_from_hypnogram(load_hypnogram(args.hypnogram), lay, down=down, sfreq=SFREQ)
        elif args.class_label is not None:
            labels = np.full(lay.n_windows, args.class_label, np.int64)
        else:
            raise ValueError("a class-conditional UNet needs --hypnogram or --class_label")
    guided = labels is not None and args.null_class is not None
    weights = os.path.join(args.diffusion_path, "best_model_ema.pth" if args.use_ema else "best_model.pth")
    if args.use_ema and not os.path.exists(weights):
        raise FileNotFoundError(f"--use_ema: {weights} not found (train with --ema_decay to have it written)")
    sd = torch.load(weights, map_location="cpu")
    # (a context model -- trained with --context -- is recognised by its checkpoint: in_channels = 2 C + 1, the context formed by the sampler)
    ckw = context_model_kwargs(up, sd, args.diffusion_path)      # (widens up["in_channels"]: ahead of the constructor call)
    unet = UNetModel(**up, dtype=args.dtype, device=local, **ckw)
    unet.load_state_dict(sd)
    sched = make_sampling_scheduler(args.num_inference_steps, prediction_type=args.prediction_type, device=local, sampler="dpmpp_2m",
                                    solver_order=args.solver_order)
    noise = randn(unet.ctx, (1, unet.x_channels, lay.canvas_len), seed=args.seed)
    rec, _canvas = sample_long(unet, stage1, sched, noise, lay.n_windows, margin=lay.margin, ramp=lay.ramp, scale_factor=scale_factor, crop=CROP,
                               labels=labels, guidance_scale=args.guidance_scale if guided else 1.0, null_class=args.null_class if guided else None)
    np.save(os.path.join(out, f"long_{args.seed}.npy"), rec.cpu().numpy())
    if labels is not None:
        np.save(os.path.join(out, f"long_{args.seed}_labels.npy"), labels)
    with open(os.path.join(out, f"long_{args.seed}_layout.json"), "w") as f:
        json.dump(layout_json(lay, down), f)
    return out


if __name__ == "__main__":
    main(parse_args())
