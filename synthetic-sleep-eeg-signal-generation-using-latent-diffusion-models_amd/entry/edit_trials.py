"""Variation and repair of real EEG windows: sampling that starts from an input (SDEdit) and, with a mask, regenerates only the marked
span (inpainting).  Models, configs, EMA, label, guidance and sampler flags are those of sample_trials.py (--pixel: the pixel-space model
of sample_trials_dm.py, --config_file instead of the two LDM configs).  --input windows.npy holds (N, 3072) or (N, 1, 3072) windows;
window i is noised with the N(0, 1) draw of seed --seed + i up to --strength of the schedule and denoised from there.  --mask mask.npy
((3072,), (N, 3072) or (N, 1, 3072), values in [0, 1], 1 = keep) and / or --mask_span START:STOP (window samples START .. STOP - 1 are
regenerated; may be repeated) select what is replaced; the kept samples come back bit for bit unless --no_composite.  Writes
edit_{i}.npy of shape (1, 1, 3000) (crop [36:-36], as sample_{i}.npy) and, when a mask was used, edit_{i}_mask.npy: the keep-mask of
the same shape.  --resamples R --jump_length J (defaults 1 and 1: the plain repair; needs a mask): RePaint's resampling, R - 1 jumps of
J steps back up the schedule at every J-th level, each with fresh noise from the Philox key schedulers.RESAMPLE_KEY + --seed + (index of
the call's first window), so that no two calls -- batches or ranks -- share their jump noise (a window's result is reproducible for a given
--batch and world size; its position inside the call decides which part of the stream it reads); the cost is the forward count, and with R > 1 edit_{i}_resample.json records {"resamples", "jump_length", "forwards"}.  J = 1 is a convention: no
(R, J) has been measured on sleep data.  A checkpoint trained with --context is recognised by its 'context' entry (a bare state dict: by
its first conv) and the kept signal and the mask then also reach the model as its context, at no extra forward; --no_blend drops the
replacement blend and leaves the learned conditioning alone.  Windows are batched and sharded over ranks (no collective)."""
import argparse
import json
import os

import numpy as np
import torch

from .. import distributed as D
from ..models import AutoencoderKL, UNetModel
from ..sampling import make_sampling_scheduler, sample
from ..training import randn
from .common import context_model_kwargs, load_config

WINDOW = 3072


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--output_dir", required=True); p.add_argument("--diffusion_path", required=True)
    p.add_argument("--input", required=True, help=".npy of (N, 3072) or (N, 1, 3072) windows")
    p.add_argument("--best_model_path", default=None); p.add_argument("--autoencoderkl_config_file_path", default=None)
    p.add_argument("--ldm_config_file_path", default=None)
    p.add_argument("--pixel", action="store_true", help="the pixel-space diffusion model (no autoencoder); needs --config_file")
    p.add_argument("--config_file", default=None)
    p.add_argument("--strength", type=float, default=1.0, help="in (0, 1]: the share of the schedule that is run; small = close to the input")
    p.add_argument("--mask", default=None, help=".npy keep-mask, 1 = keep, 0 = regenerate")
    p.add_argument("--mask_span", action="append", default=None, help="START:STOP in window samples, regenerated; may be repeated")
    p.add_argument("--no_composite", action="store_true", help="return the decoded windows as they are instead of pasting the kept samples back")
    p.add_argument("--seed", type=int, default=0, help="window i is noised with the draw of seed SEED + i")
    p.add_argument("--guidance_scale", type=float, default=7.0); p.add_argument("--num_inference_steps", type=int, default=200)
    p.add_argument("--spe", default="no-spectral"); p.add_argument("--latent_channels", type=int, default=1)
    p.add_argument("--type_dataset", default="edfx")
    p.add_argument("--prediction_type", default="v_prediction")
    p.add_argument("--batch", type=int, default=256); p.add_argument("--dtype", default="float32")
    p.add_argument("--num_classes", type=int, default=None, help="class-conditional UNet (overrides unet_config.params.num_classes)")
    p.add_argument("--class_label", type=int, default=None, help="the sleep stage of every window (W 0, N1 1, N2 2, N3 3, REM 4)")
    p.add_argument("--labels_file", default=None, help=".npy / text file with one label per input window")
    p.add_argument("--null_class", type=int, default=None, help="classifier-free guidance: the unconditional class; --guidance_scale "
                   "applies to a class-conditional UNet only when it is given")
    p.add_argument("--use_ema", action="store_true", help="sample from best_model_ema.pth (a run trained with --ema_decay) instead of best_model.pth")
    p.add_argument("--sampler", default="ddim", choices=["ddim", "dpmpp_2m"])
    p.add_argument("--solver_order", type=int, default=2, choices=[1, 2], help="dpmpp_2m only")
    p.add_argument("--resamples", type=int, default=1, help="RePaint resampling: visits of every jump point (1 = none); needs a mask")
    p.add_argument("--jump_length", type=int, default=1, help="steps a jump goes back up, and the spacing of the jump points")
    p.add_argument("--no_blend", action="store_true", help="a context model only (a checkpoint trained with --context, recognised by itself): use the "
                   "learned conditioning alone instead of also resetting the kept latents after every step")
    return p.parse_args(argv)


def check_args(args):
    if not 0.0 < args.strength <= 1.0:
        raise ValueError(f"--strength must lie in (0, 1], got {args.strength}")
    if args.resamples < 1 or args.jump_length < 1:
        raise ValueError("--resamples and --jump_length must be >= 1")
    if args.resamples > 1 and args.mask is None and not args.mask_span:
        raise ValueError("--resamples > 1 needs --mask or --mask_span")
    if args.pixel:
        if not args.config_file:
            raise ValueError("--pixel needs --config_file")
    elif not (args.best_model_path and args.autoencoderkl_config_file_path and args.ldm_config_file_path):
        raise ValueError("the LDM needs --best_model_path, --autoencoderkl_config_file_path and --ldm_config_file_path (or pass --pixel)")


def build_mask(args, n, length=WINDOW):
    """-> the keep-mask (n, 1, length) float32, 1 = keep, or None when neither --mask nor --mask_span is given"""
    if args.mask is None and not args.mask_span:
        return None
    keep = np.ones((n, 1, length), np.float32)
    if args.mask is not None:
        m = np.asarray(np.load(args.mask), np.float32)
        if m.shape not in ((length,), (n, length), (n, 1, length)):
            raise ValueError(f"{args.mask}: shape {m.shape}, expected ({length},), ({n}, {length}) or ({n}, 1, {length})")
        if not ((m >= 0) & (m <= 1)).all():
            raise ValueError(f"{args.mask}: values must lie in [0, 1]")
        keep = keep * m.reshape((1, 1, length) if m.ndim == 1 else (n, 1, length))
    for span in args.mask_span or ():
        try:
            a, b = (int(v) for v in span.split(":"))
        except ValueError:
            raise ValueError(f"--mask_span {span!r}: expected START:STOP") from None
        if not 0 <= a < b <= length:
            raise ValueError(f"--mask_span {span}: needs 0 <= START < STOP <= {length}")
        keep[:, :, a:b] = 0.0
    return keep


def load_windows(path):
    x = np.asarray(np.load(path), np.float32)
    if x.ndim == 2:
        x = x[:, None, :]
    if x.ndim != 3 or x.shape[1:] != (1, WINDOW):
        raise ValueError(f"{path}: shape {x.shape}, expected (N, {WINDOW}) or (N, 1, {WINDOW})")
    return x


def main(args):
    check_args(args)
    rank, local, world = D.init_from_env()
    torch.cuda.set_device(local)
    x_in = load_windows(args.input)
    N = len(x_in)
    keep = build_mask(args, N)
    name = f"edits_dm_{args.spe}_{args.type_dataset}" if args.pixel else f"edits_ldm_{args.latent_channels}_{args.spe}_{args.type_dataset}"
    out = os.path.join(args.output_dir, name)
    os.makedirs(out, exist_ok=True)
    stage1, scale_factor = None, 1.0
    if args.pixel:
        up = dict(load_config(args.config_file)["model"]["params"]["unet_config"]["params"])
        up["in_channels"] = up["out_channels"] = 1
        latent_len = WINDOW
    else:
        ae_cfg = dict(load_config(args.autoencoderkl_config_file_path).autoencoderkl.params)
        ae_cfg.setdefault("num_channels", [32, 32, 64]); ae_cfg["latent_channels"] = args.latent_channels
        stage1 = AutoencoderKL(**ae_cfg, dtype=args.dtype, device=local)
        stage1.load_state_dict(torch.load(os.path.join(args.best_model_path, "best_model.pth"), map_location="cpu"))
        up = dict(load_config(args.ldm_config_file_path)["model"]["params"]["unet_config"]["params"])
        up["in_channels"] = up["out_channels"] = args.latent_channels
        scale_factor = float(torch.load(os.path.join(args.diffusion_path, "checkpoint.pth"), map_location="cpu")["scale_factor"])
        latent_len = WINDOW // stage1.down
    if args.num_classes is not None:
        up["num_classes"] = args.num_classes
    labels = None
    if up.get("num_classes") is not None:
        if args.labels_file:
            f = args.labels_file
            labels = np.load(f) if f.endswith(".npy") else np.loadtxt(f, dtype=np.int64, ndmin=1)
            labels = np.asarray(labels, dtype=np.int64).reshape(-1)
            if len(labels) != N:
                raise ValueError(f"{f}: {len(labels)} labels for {N} windows")
        elif args.class_label is not None:
            labels = np.full(N, args.class_label, np.int64)
        else:
            raise ValueError("a class-conditional UNet needs --class_label or --labels_file")
    guided = labels is not None and args.null_class is not None
    weights = os.path.join(args.diffusion_path, "best_model_ema.pth" if args.use_ema else "best_model.pth")
    if args.use_ema and not os.path.exists(weights):
        raise FileNotFoundError(f"--use_ema: {weights} not found (train with --ema_decay to have it written)")
    sd = torch.load(weights, map_location="cpu")
    # (a context model -- trained with --context -- is recognised by its checkpoint: in_channels = 2 C + 1, the context formed by the sampler)
    ckw = context_model_kwargs(up, sd, args.diffusion_path)      # (widens up["in_channels"]: ahead of the constructor call)
    unet = UNetModel(**up, dtype=args.dtype, device=local, **ckw)
    unet.load_state_dict(sd)
    sched = make_sampling_scheduler(args.num_inference_steps, prediction_type=args.prediction_type, device=local, sampler=args.sampler,
                                    solver_order=args.solver_order)
    lo, hi = D.shard_range(N, rank, world)
    lat = unet.x_channels
    for k in range(lo, hi, args.batch):
        idx = list(range(k, min(k + args.batch, hi)))
        noise = torch.empty(len(idx), lat, latent_len, device=unet.device)
        for j, i in enumerate(idx):
            noise[j] = randn(unet.ctx, (lat, latent_len), seed=args.seed + i)
        m = None if keep is None else torch.from_numpy(keep[idx[0]:idx[-1] + 1])
        info = {}
        windows, _ = sample(unet, stage1, sched, noise, scale_factor=scale_factor, labels=None if labels is None else labels[idx[0]:idx[-1] + 1],
                            guidance_scale=args.guidance_scale if guided else 1.0, null_class=args.null_class if guided else None,
                            init=torch.from_numpy(x_in[idx[0]:idx[-1] + 1]), strength=args.strength, mask=m,
                            composite=False if args.no_composite else None, resamples=args.resamples, jump_length=args.jump_length,
                            seed=args.seed + idx[0], info=info, blend=not args.no_blend)
        arr = windows.cpu().numpy()
        for j, i in enumerate(idx):
            np.save(os.path.join(out, f"edit_{i}.npy"), arr[j:j + 1])
            if keep is not None:
                np.save(os.path.join(out, f"edit_{i}_mask.npy"), keep[i:i + 1, :, 36:-36])
            if args.resamples > 1:
                with open(os.path.join(out, f"edit_{i}_resample.json"), "w") as f:
                    json.dump(dict(resamples=args.resamples, jump_length=args.jump_length, forwards=info["forwards"]), f)
    return out


if __name__ == "__main__":
    main(parse_args())
