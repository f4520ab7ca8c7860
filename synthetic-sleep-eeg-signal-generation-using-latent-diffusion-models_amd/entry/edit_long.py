"""Repair, vary or continue a REAL recording on one latent canvas (sampling.sample_long with init / mask).  Model, EMA, label, guidance,
sampler, margin and ramp flags are those of sample_long.py.  --input recording.npy holds (n,), (R, n) or (R, 1, n) samples, normalised
like training windows, WITHOUT the 36-sample edge pads: the script pads `crop` zeros at both ends, as a training window holds them.
It takes the largest W with down * ((W - 1) * S + L) - 2 * crop <= n (defaults: 2784 (W - 1) + 3000 <= n) and prints how many trailing
samples were left out.  --strength: the share of the step grid that runs (1 = from pure noise wherever the mask is 0).  --mask mask.npy
(the input's shape, 1 = keep) and / or --mask_span START:STOP (repeatable, input samples, regenerated) say what is regenerated; without
either, and without --extend_minutes, the whole recording is varied.  --extend_minutes X appends enough windows to cover X more minutes:
the input is kept (mask 1) and the extension is regenerated (mask 0, init zero there).  --mask_erode E shrinks the kept regions of the
LATENT keep-mask by E samples beside every regenerated span (default 0; no value has been measured against anything); the composite
uses the mask as given.  --no_composite returns the decoded recording instead of input-where-kept.
Writes edit_long_{seed}.npy ((R, 1, samples), crop off both ends), edit_long_{seed}_mask.npy (the mask used, same shape; all zeros when
nothing was kept), edit_long_{seed}_labels.npy (class-conditional UNet only) and edit_long_{seed}_layout.json (sample_long.py's layout
file plus input_samples / left_out / kept_windows: what tools/seam_report.py reads).  --resamples R --jump_length J (defaults 1 and 1: the
plain repair; needs something kept, i.e. a mask or an extension): RePaint's resampling as in edit_trials.py, fresh noise from the Philox key
schedulers.RESAMPLE_KEY + --seed; with R > 1 the layout file gains {"resamples", "jump_length", "forwards"}."""
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
from .sample_long import CROP, SFREQ, WINDOW, layout_json, load_hypnogram


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--output_dir", required=True); p.add_argument("--diffusion_path", required=True)
    p.add_argument("--input", required=True, help=".npy: (n,), (R, n) or (R, 1, n) samples, normalised like training windows, without edge pads")
    p.add_argument("--best_model_path", default=None); p.add_argument("--autoencoderkl_config_file_path", default=None)
    p.add_argument("--ldm_config_file_path", default=None)
    p.add_argument("--pixel", action="store_true", help="the pixel-space diffusion model (no autoencoder); needs --config_file")
    p.add_argument("--config_file", default=None)
    p.add_argument("--strength", type=float, default=1.0, help="share of the step grid that runs, in (0, 1]")
    p.add_argument("--mask", default=None, help=".npy of the input's shape, 1 = keep, 0 = regenerate")
    p.add_argument("--mask_span", action="append", default=[], metavar="START:STOP", help="input samples to regenerate (repeatable)")
    p.add_argument("--mask_erode", type=int, default=0, help="shrink the latent keep-mask by this many samples beside every regenerated span")
    p.add_argument("--no_composite", action="store_true")
    p.add_argument("--no_blend", action="store_true", help="a context model only (a checkpoint trained with --context, recognised by itself): use the "
                   "learned conditioning alone instead of also resetting the kept canvas positions after every step")
    p.add_argument("--extend_minutes", type=float, default=0.0, help="continue the recording by at least this many minutes")
    p.add_argument("--margin", type=int, default=None, help="zero-weight positions at a window edge that has a neighbour (default 2 * 36 / down)")
    p.add_argument("--ramp", type=int, default=None, help="positions of the linear cross-fade (default 4 * 36 / down)")
    p.add_argument("--hypnogram", default=None, help=".npy / text file, one sleep stage per 30-s epoch (input and extension)")
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
    p.add_argument("--resamples", type=int, default=1, help="RePaint resampling: visits of every jump point (1 = none); needs a mask or an extension")
    p.add_argument("--jump_length", type=int, default=1, help="steps a jump goes back up, and the spacing of the jump points")
    return p.parse_args(argv)


def check_args(args):
    if not 0.0 < args.strength <= 1.0:
        raise ValueError("--strength must lie in (0, 1]")
    if args.mask_erode < 0:
        raise ValueError("--mask_erode must be >= 0")
    if args.resamples < 1 or args.jump_length < 1:
        raise ValueError("--resamples and --jump_length must be >= 1")
    if args.resamples > 1 and args.mask is None and not args.mask_span and not args.extend_minutes > 0:
        raise ValueError("--resamples > 1 needs --mask, --mask_span or --extend_minutes")
    if not args.extend_minutes >= 0:
        raise ValueError("--extend_minutes must be >= 0")
    if args.hypnogram is not None and args.class_label is not None:
        raise ValueError("pass --hypnogram or --class_label, not both")
    for s in args.mask_span:
        parse_span(s)
    if args.pixel:
        if not args.config_file:
            raise ValueError("--pixel needs --config_file")
    elif not (args.best_model_path and args.autoencoderkl_config_file_path and args.ldm_config_file_path):
        raise ValueError("the LDM needs --best_model_path, --autoencoderkl_config_file_path and --ldm_config_file_path (or pass --pixel)")


def parse_span(text):
    """"START:STOP" -> (start, stop), 0 <= start < stop"""
    try:
        a, b = (int(v) for v in text.split(":"))
    except ValueError:
        raise ValueError(f"--mask_span {text!r}: expected START:STOP") from None
    if not 0 <= a < b:
        raise ValueError(f"--mask_span {text!r}: needs 0 <= START < STOP")
    return a, b


def spans_to_mask(n, spans):
    """float32 (n,): 1 = keep, 0 inside every [start, stop) of `spans` (input samples; a stop past the end is an error)"""
    m = np.ones(int(n), np.float32)
    for a, b in spans:
        if not 0 <= a < b <= n:
            raise ValueError(f"span {a}:{b} outside the input's {n} samples")
        m[a:b] = 0.0
    return m


def plan_edit(n, window_len, down, margin=None, ramp=None, extend_minutes=0.0, crop=CROP, sfreq=SFREQ):
    """The planning arithmetic, pure integers.  n input samples (no pads), windows of window_len positions of `down` samples ->
    dict(layout = the LongLayout of the run (input and extension), kept_windows = W0, the largest W with down * ((W - 1) * S + L) - 2 * crop
    <= n, used = the input samples those windows hold, left_out = n - used trailing samples, extension = samples appended).  The extension
    adds the fewest windows that cover extend_minutes more minutes."""
    m = 2 * crop // down if margin is None else int(margin)
    r = 4 * crop // down if ramp is None else int(ramp)
    one = long_layout(1, window_len, m, r)
    S, L = one.stride, one.window_len
    first = down * L - 2 * crop
    if n < first:
        raise ValueError(f"the input has {n} samples: one window needs {first}")
    W0 = (n - first) // (down * S) + 1
    used = down * ((W0 - 1) * S + L) - 2 * crop
    extra = int(math.ceil(float(extend_minutes) * 60.0 * sfreq / (down * S))) if extend_minutes > 0 else 0
    lay = long_layout(W0 + extra, window_len, m, r)
    return dict(layout=lay, kept_windows=W0, used=used, left_out=n - used, extension=extra * down * S)


def build_inputs(x, mask, plan, down, crop=CROP):
    """x (R, n) input samples, mask (R, n) or None -> (init (R, 1, down * Lc), mask (R, 1, down * Lc) or None): `crop` zeros, the used input
    samples, then zeros (the extension and the far pad).  The mask is 1 over the leading pad and -- without an extension -- the trailing one
    (the zeros are what a training window holds there), the given mask over the input, 0 over the extension.  No mask and no extension:
    None, the whole recording is varied."""
    R, used, total = x.shape[0], plan["used"], plan["layout"].canvas_len * down
    init = np.zeros((R, 1, total), np.float32)
    init[:, 0, crop:crop + used] = x[:, :used]
    if mask is None and not plan["extension"]:
        return init, None
    mk = np.zeros((R, 1, total), np.float32)
    mk[:, 0, :crop] = 1.0
    mk[:, 0, crop:crop + used] = 1.0 if mask is None else mask[:, :used]
    if not plan["extension"]:
        mk[:, 0, crop + used:] = 1.0
    return init, mk


def load_input(path):
    x = np.asarray(np.load(path), np.float32)
    if x.ndim == 3 and x.shape[1] == 1:
        x = x[:, 0]
    if x.ndim == 1:
        x = x[None]
    if x.ndim != 2:
        raise ValueError(f"{path}: shape {x.shape}, expected (n,), (R, n) or (R, 1, n)")
    return x


def main(args):
    check_args(args)
    x = load_input(args.input)
    R, n = x.shape
    mask = None
    if args.mask is not None:
        mask = load_input(args.mask)
        if mask.shape != x.shape:
            raise ValueError(f"--mask has shape {mask.shape}, the input {x.shape}")
    if args.mask_span:
        spans = np.broadcast_to(spans_to_mask(n, [parse_span(s) for s in args.mask_span]), x.shape)
        mask = spans.copy() if mask is None else np.minimum(mask, spans)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    name = f"edit_long_dm_{args.spe}_{args.type_dataset}" if args.pixel else f"edit_long_ldm_{args.latent_channels}_{args.spe}_{args.type_dataset}"
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
    plan = plan_edit(n, window_len, down, args.margin, args.ramp, args.extend_minutes)
    lay = plan["layout"]
    print(f"{n} input samples: {plan['kept_windows']} windows hold {plan['used']}, {plan['left_out']} trailing samples left out; "
          f"{lay.n_windows - plan['kept_windows']} windows ({plan['extension']} samples) appended")
    init, mk = build_inputs(x, mask, plan, down)
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
    noise = randn(unet.ctx, (R, unet.x_channels, lay.canvas_len), seed=args.seed)
    info = {}
    rec, _canvas = sample_long(unet, stage1, sched, noise, lay.n_windows, margin=lay.margin, ramp=lay.ramp, scale_factor=scale_factor, crop=CROP,
                               labels=labels, guidance_scale=args.guidance_scale if guided else 1.0, null_class=args.null_class if guided else None,
                               init=torch.from_numpy(init), strength=args.strength, mask=None if mk is None else torch.from_numpy(mk),
                               composite=False if (args.no_composite or mk is None) else None, mask_erode=args.mask_erode,
                               resamples=args.resamples, jump_length=args.jump_length, seed=args.seed, info=info,
                               blend=not args.no_blend)
    np.save(os.path.join(out, f"edit_long_{args.seed}.npy"), rec.cpu().numpy())
    used_mask = np.zeros_like(init) if mk is None else mk
    np.save(os.path.join(out, f"edit_long_{args.seed}_mask.npy"), used_mask[:, :, CROP:-CROP])
    if labels is not None:
        np.save(os.path.join(out, f"edit_long_{args.seed}_labels.npy"), labels)
    with open(os.path.join(out, f"edit_long_{args.seed}_layout.json"), "w") as f:
        extra = dict(resamples=args.resamples, jump_length=args.jump_length, forwards=info["forwards"]) if args.resamples > 1 else {}
        json.dump(dict(layout_json(lay, down), input_samples=n, left_out=plan["left_out"], kept_windows=plan["kept_windows"], **extra), f)
    return out


if __name__ == "__main__":
    main(parse_args())
