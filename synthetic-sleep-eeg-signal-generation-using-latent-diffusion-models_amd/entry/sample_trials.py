"""DDIM sampling of synthetic EEG windows -- counterpart of /root/reference/src/sample_trials.py: loads the stage-1
autoencoder + UNet checkpoints, reads scale_factor from checkpoint.pth (:130-132), samples one window per seed
(batched; seeds sharded over ranks, no collective), writes sample_{i}.npy of shape (1,1,3000) (:169-170).
--num_inference_steps is honoured (the reference hard-codes 200, :144); PSD plots (mne) are out of scope."""
import argparse
import os

import numpy as np
import torch

from .. import distributed as D
from ..models import AutoencoderKL, UNetModel
from ..sampling import make_sampling_scheduler, sample_seeds
from .common import context_model_kwargs, load_config


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--output_dir", required=True); p.add_argument("--best_model_path", required=True)
    p.add_argument("--diffusion_path", required=True); p.add_argument("--autoencoderkl_config_file_path", required=True)
    p.add_argument("--ldm_config_file_path", required=True)
    p.add_argument("--start_seed", type=int, default=0); p.add_argument("--stop_seed", type=int, default=1000)
    p.add_argument("--guidance_scale", type=float, default=7.0); p.add_argument("--num_inference_steps", type=int, default=200)
    p.add_argument("--path_pre_processed", default=None); p.add_argument("--spe", default="no-spectral")
    p.add_argument("--latent_channels", type=int, default=1); p.add_argument("--type_dataset", default="edfx")
    p.add_argument("--prediction_type", default="v_prediction", help="sample_trials.py:141 uses v_prediction")
    p.add_argument("--batch", type=int, default=256); p.add_argument("--dtype", default="float32")
    p.add_argument("--num_classes", type=int, default=None, help="class-conditional UNet (overrides unet_config.params.num_classes)")
    p.add_argument("--class_label", type=int, default=None, help="the sleep stage of every window (W 0, N1 1, N2 2, N3 3, REM 4)")
    p.add_argument("--labels_file", default=None, help=".npy / text file with one label per seed, seeds start_seed .. stop_seed - 1 in order")
    p.add_argument("--null_class", type=int, default=None, help="classifier-free guidance: the unconditional class; --guidance_scale "
                   "applies to a class-conditional UNet only when it is given")
    p.add_argument("--use_ema", action="store_true", help="sample from best_model_ema.pth (a run trained with --ema_decay) instead of best_model.pth")
    p.add_argument("--sampler", default="ddim", choices=["ddim", "dpmpp_2m"], help="dpmpp_2m: DPM-Solver++ (2M), second-order multistep; "
                   "reaches DDIM's 50-step result in fewer --num_inference_steps")
    p.add_argument("--solver_order", type=int, default=2, choices=[1, 2], help="dpmpp_2m only (1 = first order, DDIM on the linspace grid)")
    return p.parse_args(argv)


def main(args):
    rank, local, world = D.init_from_env()
    torch.cuda.set_device(local)
    out = os.path.join(args.output_dir, f"samples_ldm_{args.latent_channels}_{args.spe}_{args.type_dataset}")
    os.makedirs(out, exist_ok=True)
    ae_cfg = dict(load_config(args.autoencoderkl_config_file_path).autoencoderkl.params)
    ae_cfg.setdefault("num_channels", [32, 32, 64]); ae_cfg["latent_channels"] = args.latent_channels     # sample_trials.py:97-98
    stage1 = AutoencoderKL(**ae_cfg, dtype=args.dtype, device=local)
    stage1.load_state_dict(torch.load(os.path.join(args.best_model_path, "best_model.pth"), map_location="cpu"))
    up = dict(load_config(args.ldm_config_file_path)["model"]["params"]["unet_config"]["params"])
    up["in_channels"] = up["out_channels"] = args.latent_channels
    if args.num_classes is not None:
        up["num_classes"] = args.num_classes
    labels = None
    if up.get("num_classes") is not None:
        if args.labels_file:
            f = args.labels_file
            labels = np.load(f) if f.endswith(".npy") else np.loadtxt(f, dtype=np.int64, ndmin=1)
            labels = np.asarray(labels, dtype=np.int64).reshape(-1)
            if len(labels) != args.stop_seed - args.start_seed:
                raise ValueError(f"{f}: {len(labels)} labels for {args.stop_seed - args.start_seed} seeds")
        elif args.class_label is not None:
            labels = np.full(args.stop_seed - args.start_seed, args.class_label, np.int64)
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
    scale_factor = float(torch.load(os.path.join(args.diffusion_path, "checkpoint.pth"), map_location="cpu")["scale_factor"])
    sched = make_sampling_scheduler(args.num_inference_steps, prediction_type=args.prediction_type, device=local, sampler=args.sampler,
                                    solver_order=args.solver_order)
    lo, hi = D.shard_range(args.stop_seed - args.start_seed, rank, world)
    seeds = list(range(args.start_seed + lo, args.start_seed + hi))
    for k in range(0, len(seeds), args.batch):
        chunk = seeds[k:k + args.batch]
        lab = None if labels is None else labels[lo + k:lo + k + len(chunk)]
        windows, _ = sample_seeds(unet, stage1, sched, chunk, latent_len=up.get("image_size", 768), scale_factor=scale_factor, labels=lab,
                                  guidance_scale=args.guidance_scale if guided else 1.0, null_class=args.null_class if guided else None)
        arr = windows.cpu().numpy()
        for j, sd in enumerate(chunk):
            np.save(os.path.join(out, f"sample_{sd}.npy"), arr[j:j + 1])
            if lab is not None:                         # the window's class beside it
                np.save(os.path.join(out, f"sample_{sd}_label.npy"), lab[j:j + 1])
    return out


if __name__ == "__main__":
    main(parse_args())
