"""Pixel-space diffusion training directly on the (B,1,3072) windows -- counterpart of
/root/reference/src/train_pure_ldm.py + src/training/training_diffusion.py::train_epoch_diffusion (config_dm.yaml; BASELINE C5):
UNet with in/out channels forced to 1 (train_pure_ldm.py:113-115), DDPMScheduler("linear_beta", 0.0015, 0.0195) (:123-124),
Adam 1e-4 (:136), loss = mse(noise_pred, noise) [+ 1e-6 * JukeboxLoss(sum) with --spe spectral (:128-132, :157-158)].
One process per GPU under torch.distributed.run for data parallelism."""
import argparse
import os
import time

import torch

from .. import distributed as D
from ..models import UNetModel
from ..schedulers import DDPMScheduler
from ..training import EMA, Adam, GradScaler, NoiseLevelLoss, dm_train_step, randint, randn
from .common import (accum_factor, accum_plan, add_context_args, add_device_loader_args, add_ema_args, add_grad_clip_args, add_loss_weighting_args, append_noise_level_record, context_entry,
                     context_resume, cpu_state, ema_checkpoint_entry, ema_resume,
                     format_clip_stats, format_noise_level_table, grad_clip_entry, grad_clip_resume, load_config, loss_weighting_resume, rng_seed, setup_run_dir, step_weighting,
                     window_loader)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config_file", required=True)
    p.add_argument("--path_train_ids", default=None); p.add_argument("--path_valid_ids", default=None)
    p.add_argument("--path_cached_data", default=None); p.add_argument("--path_pre_processed", default=None)
    p.add_argument("--spe", default="no-spectral"); p.add_argument("--type_dataset", default="edfx"); p.add_argument("--dataset", default="edfx")
    p.add_argument("--synthetic_windows", type=int, default=0); p.add_argument("--dtype", default="float32")
    p.add_argument("--max_steps", type=int, default=0); p.add_argument("--output_dir", default=None)
    p.add_argument("--grad_scaler", action="store_true", help="dynamic loss scaling as training_diffusion.py:37 does (always on with --dtype float16)")
    p.add_argument("--deterministic", action="store_true", help="bit-reproducible steps (eegldm.set_deterministic(): ordered reductions instead of fp32 atomics; "
                   "what torch.use_deterministic_algorithms(True) would be for the reference's loop)")
    add_ema_args(p)
    add_loss_weighting_args(p)
    add_grad_clip_args(p)
    add_device_loader_args(p)
    add_context_args(p)
    return p.parse_args(argv)


def main(args):
    if getattr(args, "deterministic", False):
        from .._lib import set_deterministic
        set_deterministic(True)
    rank, local, world = D.init_from_env()
    torch.cuda.set_device(local)
    config = load_config(args.config_file)
    torch.manual_seed(config.train.seed)
    run_dir, resume = setup_run_dir(config, args)
    if resume:                                 # (ahead of the model: a run trained with --context has another first conv)
        context_resume(args, torch.load(os.path.join(run_dir, "checkpoint.pth"), map_location="cpu"))
    context_entry(args, 1)            # the flags' own refusals, before any model exists (span_max <= L is checked once the data gives L)
    up = dict(config.model.params.unet_config.params)
    up["in_channels"] = up["out_channels"] = 1                                  # train_pure_ldm.py:113-115
    if args.context:                           # [x | m * x | m]: the pixel model's context is the masked window itself
        up["in_channels"] = 3
    unet = UNetModel(**up, dtype=args.dtype, device=local, **({"context_channels": 2} if args.context else {}))
    D.broadcast_flat(unet.flat); unet.sync_weights()
    sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195, device=local)
    ema = EMA(unet, decay=args.ema_decay, warmup=not args.ema_no_warmup) if args.ema_decay is not None else None      # after the broadcast
    opt = Adam(unet, lr=1e-4, ema=ema, max_grad_norm=args.max_grad_norm)
    # training_diffusion.py:37,149-151 pairs its fp16 autocast with a GradScaler: fp16 activation gradients under- / overflow without the loss scale
    scaler = GradScaler(enabled=args.grad_scaler or str(args.dtype) in ("float16", "fp16", "half"))
    spectral = args.spe == "spectral"
    bs = max(1, config.train.batch_size // world)
    train = window_loader(args, args.path_pre_processed, bs, args.synthetic_windows, seed=rng_seed(config.train.seed, 8, rank, world), drop_last=config.train.drop_last,
                          path_ids=args.path_train_ids, dataset=args.type_dataset, shard=(rank, world))
    s_t, s_noise = rng_seed(config.train.seed, 1, rank, world), rng_seed(config.train.seed, 3, rank, world)
    s_mask, centry, cspec = rng_seed(config.train.seed, 11, rank, world), None, None
    dev, ctx = unet.device, unet.ctx
    loss = torch.zeros(1, device=dev)
    gsync = D.OverlappedGradSync(unet.flat_grad, ctx=unet.ctx, comm=D.make_comm(unet.ctx))   # no-op with one process; EEGLDM_NATIVE_COLLECTIVES=1: RCCL through the C ABI
    steps, t0, seen, best, start_epoch, gstep = 0, time.time(), 0, float("inf"), 0, 0      # gstep: steps over all invocations (RNG offsets)
    if resume:      # continue from {run_dir}/checkpoint.pth
        ck = torch.load(os.path.join(run_dir, "checkpoint.pth"), map_location="cpu")
        unet.load_state_dict(ck["diffusion"]); opt.load_state_dict(ck["optimizer"])
        if "scaler" in ck:
            scaler.load_state_dict(ck["scaler"])
        start_epoch, best, gstep = int(ck["epoch"]), float(ck["best_loss"]), int(ck.get("steps", 0))
        loss_weighting_resume(args, ck)
        grad_clip_resume(args, ck, rank)
        if args.max_grad_norm != opt.max_grad_norm:
            opt.set_max_grad_norm(args.max_grad_norm)
        if ema is not None:
            ema_resume(ema, ck, rank)
        if rank == 0:
            print(f"Resuming from epoch {start_epoch} (best loss {best:.5f})")
    save_weighting = args.loss_weighting is not None             # (after the resume: a restored setting is written again)
    wkw = step_weighting(args)                                   # {} without the flags: the plain MSE, as before
    GA = int(args.grad_accum_steps or 1)                         # micro-batches per optimizer step
    K = int(args.loss_by_noise_level)                            # this script has no validation split: the table is the epoch's training steps
    train_levels = NoiseLevelLoss(sched.num_train_timesteps, K) if K else None
    for epoch in range(start_epoch, config.train.n_epochs):
        unet.train()
        if train_levels is not None:
            train_levels.reset()
        left = args.max_steps - steps if args.max_steps else None
        for i, batch in enumerate(train):
            zero, last, k = accum_plan(i, len(train), GA, left)
            x = batch["eeg"].to(dev)
            B = x.shape[0]
            t = randint(ctx, B, sched.num_train_timesteps, seed=s_t, offset=gstep * B)
            noise = randn(ctx, tuple(x.shape), seed=s_noise, offset=gstep * x.numel())
            if zero:
                opt.zero_grad()
            if train_levels is not None:
                wkw["per_sample_out"] = torch.empty(B, device=dev)
            ckw = {}
            if args.context:               # the step draws the masks in registers: no mask buffer, no second pass
                if centry is None:
                    centry = context_entry(args, 1, x.shape[2])
                    cspec = {k: centry[k] for k in ("p_none", "p_prefix", "span_min", "span_max")}
                ckw = dict(context_mask=cspec, mask_seed=s_mask, mask_offset=gstep * B)
            dm_train_step(unet, sched, x, noise, t, spectral_weight=1e-6, spectral_loss=spectral, loss_out=loss, grad_sync=gsync if last else None,
                          grad_scale=scaler.get_scale() / GA, **wkw, **ckw)
            if train_levels is not None:
                train_levels.add(wkw["per_sample_out"], t, ctx=ctx)
            if last:                       # one all-reduce and one optimizer step per group; a short group counts its k micro-batches K / k
                gsync.wait()
                scaler.step(opt, accum_factor(GA, k)); scaler.update()
            steps += 1; gstep += 1; seen += B * world
            if args.max_steps and steps >= args.max_steps:
                break
        if K:                                  # every rank joins the sums; rank 0 prints and writes
            record = {"epoch": epoch + 1, "steps": gstep, "prediction_type": sched.prediction_type, "bins": K,
                      "train": train_levels.merge(like=loss).table(), "valid": None, "valid_ema": None}
        if rank == 0:
            print(f"epoch {epoch}: loss {float(loss):.5f} | {seen/(time.time()-t0):.1f} windows/s" + (format_clip_stats(opt) if opt.max_grad_norm is not None else ""), flush=True)
            if K:
                print(format_noise_level_table("train", record["train"]), flush=True)
                append_noise_level_record(run_dir, record)
            cur = float(loss)
            if cur <= best:
                best = cur
                torch.save({k: v.cpu() for k, v in unet.state_dict().items()}, os.path.join(run_dir, "best_model.pth"))
                if ema is not None:            # selection is on the last training loss here: no loss of the averaged weights exists
                    torch.save(cpu_state(ema.state_dict()), os.path.join(run_dir, "best_model_ema.pth"))
            ck_out = {"epoch": epoch + 1, "diffusion": {k: v.cpu() for k, v in unet.state_dict().items()}, "optimizer": opt.state_dict(),
                      "best_loss": best, "steps": gstep, "scaler": scaler.state_dict()}
            if ema is not None:
                ck_out["ema"] = ema_checkpoint_entry(ema, best)
            if save_weighting:
                ck_out["loss_weighting"] = {"weighting": args.loss_weighting, "snr_gamma": float(args.snr_gamma)}
            if grad_clip_entry(args) is not None:
                ck_out["grad_clip"] = grad_clip_entry(args)
            if centry is not None:
                ck_out["context"] = centry
            torch.save(ck_out, os.path.join(run_dir, "checkpoint.pth"))
        if args.max_steps and steps >= args.max_steps:
            break
    if rank == 0:
        torch.save({k: v.cpu() for k, v in unet.state_dict().items()}, os.path.join(run_dir, "final_model.pth"))
        if ema is not None:
            torch.save(cpu_state(ema.state_dict()), os.path.join(run_dir, "final_model_ema.pth"))
    return run_dir


if __name__ == "__main__":
    main(parse_args())
