"""Latent-diffusion UNet training over frozen AutoencoderKL latents -- counterpart of
/root/reference/src/train_ldm.py + src/training/training.py::train_ldm (flags, yaml schema, checkpoint keys
training.py:381-397).  One process per GPU under torch.distributed.run for data parallelism."""
import argparse
import hashlib
import os
import time

import torch

from .. import distributed as D
from ..models import AutoencoderKL, UNetModel
from ..schedulers import DDPMScheduler
from ..training import EMA, Adam, GradScaler, NoiseLevelLoss, context_mask, context_window, ldm_train_step, randint, randn
from .common import (ParseListAction, accum_factor, accum_plan, add_context_args, add_device_loader_args, add_ema_args, add_grad_clip_args, add_loss_weighting_args, append_noise_level_record,
                     context_entry, context_resume, cpu_state, ema_checkpoint_entry,
                     ema_resume, format_clip_stats, format_noise_level_table, grad_clip_entry, grad_clip_resume, load_config, loss_weighting_resume, rng_seed, setup_run_dir, step_weighting,
                     window_loader)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config_file", required=True)
    p.add_argument("--path_train_ids", default=None); p.add_argument("--path_valid_ids", default=None)
    p.add_argument("--path_cached_data", default=None); p.add_argument("--path_pre_processed", default=None)
    p.add_argument("--num_channels", action=ParseListAction, default=None)
    p.add_argument("--autoencoderkl_config_file_path", required=True); p.add_argument("--best_model_path", default=None)
    p.add_argument("--spe", default="no-spectral"); p.add_argument("--latent_channels", type=int, default=1)
    p.add_argument("--type_dataset", default="edfx"); p.add_argument("--dataset", default="edfx")
    p.add_argument("--synthetic_windows", type=int, default=0); p.add_argument("--dtype", default="float32")
    p.add_argument("--max_steps", type=int, default=0); p.add_argument("--output_dir", default=None)
    p.add_argument("--prediction_type", default="epsilon")
    p.add_argument("--schedule", default="linear_beta", choices=["linear_beta", "scaled_linear_beta"],
                   help="training noise schedule; the reference builds DDPMScheduler(beta_schedule='linear') = plain linspace (train_ldm.py:199-200)")
    p.add_argument("--grad_scaler", action="store_true", help="dynamic loss scaling as in the reference loop (training.py:334,441-443); always on with --dtype float16 (the reference's autocast dtype), bf16/fp32 do not need it")
    p.add_argument("--deterministic", action="store_true", help="bit-reproducible steps (eegldm.set_deterministic(): ordered reductions instead of fp32 atomics; "
                   "what torch.use_deterministic_algorithms(True) would be for the reference's loop)")
    p.add_argument("--num_classes", type=int, default=None, help="class-conditional UNet (overrides unet_config.params.num_classes): "
                   "labels from the loader's stage files (R.stages.npy beside each recording, or under --path_stages)")
    p.add_argument("--path_stages", default=None)
    p.add_argument("--p_uncond", type=float, default=0.0, help="classifier-free guidance training: probability of replacing a label by --null_class")
    p.add_argument("--null_class", type=int, default=None, help="the unconditional class (default: num_classes - 1 when --p_uncond > 0)")
    add_ema_args(p)
    add_loss_weighting_args(p)
    add_grad_clip_args(p)
    add_device_loader_args(p)
    add_context_args(p)
    return p.parse_args(argv)


def context_latents(unet, stage1, x, mask, scale_factor):
    """The LDM's context source, in training and in sampling alike: scale_factor * the posterior mean of the MASKED window's encoding (a
    second run of the frozen encoder), so that no latent next to a hole carries what the encoder saw inside it.  mask: (B, Ll), 1 = keep."""
    from ..sampling import _encode_windows
    return _encode_windows(unet, stage1, context_window(unet.ctx, x, mask, stage1.down), scale_factor, True)


@torch.no_grad()
def validate(unet, stage1, sched, loader, scale_factor, seeds, latent_channels, by_level=None, context=None):
    """eval_ldm (training.py:455-497): mean epsilon-MSE over the validation windows, fixed noise stream (a class-conditional UNet is
    scored with each window's own label).  `seeds` = the three Philox
    keys (timesteps, posterior eps, diffusion noise), each from `rng_seed` with its own role.  Returns (sum of per-window losses,
    number of windows) so that data-parallel ranks can add their shards up.
    by_level (a NoiseLevelLoss): also receives every window's loss against the prediction type's OWN target (eegldm_diffusion_loss,
    unweighted) -- the returned sum, the model-selection criterion, is unchanged.
    context ((draw parameters, Philox key) for a context model): every window is scored under a mask drawn from that FIXED key at the
    window's index in this rank's shard, so that every epoch scores the same masks.  Key and index are per rank, like the validation noise
    (`seeds`): a run with another world size scores other masks."""
    from .._lib import lib, check, ptr
    unet.eval()
    tot, n, dev, ctx = 0.0, 0, unet.device, unet.ctx
    s_t, s_eps, s_noise = seeds
    out = torch.zeros(1, device=dev)
    seen = 0
    for batch in loader:
        x = batch["eeg"].to(dev); B = x.shape[0]
        Ll = x.shape[2] // stage1.down
        per = latent_channels * Ll                      # random numbers per window: offsets never overlap, whatever latent_channels is
        t = randint(ctx, B, sched.num_train_timesteps, seed=s_t, offset=seen)
        eps = randn(ctx, (B, latent_channels, Ll), seed=s_eps, offset=seen * per)
        noise = randn(ctx, eps.shape, seed=s_noise, offset=seen * per)
        e = stage1.encode_stage_2_inputs(x, eps=eps, scale_factor=scale_factor)
        ckw = {}
        if context is not None:
            m = context_mask(ctx, B, Ll, context[0], seed=context[1], offset=seen)
            ckw["context"] = torch.cat([m[:, None, :] * context_latents(unet, stage1, x, m, scale_factor), m[:, None, :]], 1)
        pred = unet(sched.add_noise(original_samples=e, noise=noise, timesteps=t), timesteps=t, y=batch.get("label"), **ckw)
        check(lib.eegldm_mse_loss(ctx.h, ptr(pred), ptr(noise), ptr(out), None, pred.numel(), 1.0))
        if by_level is not None:
            from .._lib import PRED
            per, own = torch.empty(B, device=dev), torch.zeros(1, device=dev)
            check(lib.eegldm_diffusion_loss(ctx.h, ptr(pred), ptr(e), ptr(noise), ptr(t), ptr(sched._acp_dev), None, PRED[sched.prediction_type],
                                            B, pred[0].numel(), 1.0, ptr(own), ptr(per), None))
            by_level.add(per, t, ctx=ctx)
        tot += float(out) * B; n += B; seen += B
    unet.train()
    return tot, n


LAST_RUN = {}      # what the most recent main() ended with (rank-local): read by the multi-rank tests


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
    context_entry(args, args.latent_channels)      # the flags' own refusals, before any model exists (span_max <= L is checked once the data gives L)
    ae_cfg = dict(load_config(args.autoencoderkl_config_file_path).autoencoderkl.params)
    if args.num_channels is not None:
        ae_cfg["num_channels"] = args.num_channels
    ae_cfg["latent_channels"] = args.latent_channels
    stage1 = AutoencoderKL(**ae_cfg, dtype=args.dtype, device=local)
    if args.best_model_path:
        stage1.load_state_dict(torch.load(os.path.join(args.best_model_path, "best_model.pth"), map_location="cpu"))
    stage1.eval()
    up = dict(config.model.params.unet_config.params)
    up["in_channels"] = up["out_channels"] = args.latent_channels            # train_ldm.py:184-187
    if args.num_classes is not None:
        up["num_classes"] = args.num_classes
    cond = up.get("num_classes") is not None                                  # UNetModel(**parameters) takes it from the yaml too
    null_class = args.null_class if args.null_class is not None else (int(up["num_classes"]) - 1 if cond and args.p_uncond > 0 else None)
    if args.context:
        up["in_channels"] = 2 * args.latent_channels + 1
    unet = UNetModel(**up, dtype=args.dtype, device=local, **({"context_channels": args.latent_channels + 1} if args.context else {}))
    D.broadcast_flat(unet.flat); unet.sync_weights(); D.broadcast_flat(stage1.flat); stage1.sync_weights()
    # train_ldm.py:199-200: monai-generative DDPMScheduler(beta_schedule="linear", 0.0015, 0.0195) = plain linspace of the betas
    # (alpha_bar[999] = 2.57e-5).  The sqrt-space "linear" of the reference's local models/ldm.py is a different table and is not
    # what train_ldm uses; --schedule scaled_linear_beta selects it deliberately.
    sched = DDPMScheduler(num_train_timesteps=1000, schedule=args.schedule, beta_start=0.0015, beta_end=0.0195,
                          prediction_type=args.prediction_type, device=local)
    # (after the broadcast: every rank's shadow starts from the same weights and, gradients being averaged before Adam.step, stays identical)
    ema = EMA(unet, decay=args.ema_decay, warmup=not args.ema_no_warmup) if args.ema_decay is not None else None
    opt = Adam(unet, lr=config.train.get("base_lr", 1e-4), ema=ema, max_grad_norm=args.max_grad_norm)
    scaler = GradScaler(enabled=args.grad_scaler or str(args.dtype) in ("float16", "fp16", "half"))      # fp16 activations: the loss scale is what keeps their gradients out of the subnormal range
    bs = max(1, config.train.batch_size // world)
    train = window_loader(args, args.path_pre_processed, bs, args.synthetic_windows, seed=rng_seed(config.train.seed, 8, rank, world), drop_last=config.train.drop_last,
                          path_ids=args.path_train_ids, dataset=args.type_dataset, shard=(rank, world), stages=cond, path_stages=args.path_stages)
    # validation: every rank scores its own shard (equal lengths, wrap-around: a recording may be scored twice when N % world != 0)
    # and the (sum, count) pairs are added over ranks -- model selection sees the WHOLE validation split, as the reference's does
    valid = window_loader(args, args.path_pre_processed, bs, 0, sampling="recording", seed=rng_seed(config.train.seed, 9, 0, world), shuffle=False, path_ids=args.path_valid_ids,
                          dataset=args.type_dataset, shard=(rank, world), stages=cond, path_stages=args.path_stages) if args.path_valid_ids else None
    v_seeds = tuple(rng_seed(config.train.seed, role, rank, world) for role in (5, 6, 7))
    s_t, s_eps, s_noise = (rng_seed(config.train.seed, role, rank, world) for role in (1, 2, 3))
    s_lab = rng_seed(config.train.seed, 10, rank, world)
    dev, ctx = unet.device, unet.ctx
    first = next(iter(train))["eeg"].to(dev)
    centry = context_entry(args, args.latent_channels, first.shape[2] // stage1.down)       # None without --context
    cspec = None if centry is None else {k: centry[k] for k in ("p_none", "p_prefix", "span_min", "span_max")}
    s_mask, v_context = rng_seed(config.train.seed, 11, rank, world), (None if centry is None else (cspec, rng_seed(config.train.seed, 12, rank, world)))
    z = stage1.encode_stage_2_inputs(first)
    # train_ldm.py:203-204 (unbiased std of one batch).  The reference is ONE process: one value for all replicas.  Here the loader is
    # rank-sharded, so every rank sees a different first batch -- rank 0's value is broadcast (and is the one checkpointed below)
    scale_factor = D.broadcast_scalar(1.0 / float(z.std()), src=0, like=z)
    if rank == 0:
        print(f"Scaling factor set to {scale_factor}")
    loss = torch.zeros(1, device=dev)
    gsync = D.OverlappedGradSync(unet.flat_grad, ctx=unet.ctx, comm=D.make_comm(unet.ctx))   # no-op with one process; EEGLDM_NATIVE_COLLECTIVES=1: RCCL through the C ABI
    steps, t0, seen, best, start_epoch, gstep = 0, time.time(), 0, float("inf"), 0, 0      # gstep: steps over all invocations (RNG offsets)
    best_ema = float("inf")
    if resume:
        # continue from {run_dir}/checkpoint.pth (keys as written below = training.py:381-387).  The reference computes `resume`
        # but always restarts at epoch 0 (train_ldm.py:113,210-211); here the run really continues, with the saved scale_factor
        ck = torch.load(os.path.join(run_dir, "checkpoint.pth"), map_location="cpu")
        unet.load_state_dict(ck["diffusion"]); opt.load_state_dict(ck["optimizer"])
        if "scaler" in ck:
            scaler.load_state_dict(ck["scaler"])
        start_epoch, best, scale_factor = int(ck["epoch"]), float(ck["best_loss"]), float(ck["scale_factor"])
        gstep = int(ck.get("steps", 0))
        loss_weighting_resume(args, ck)
        grad_clip_resume(args, ck, rank)
        if args.max_grad_norm != opt.max_grad_norm:
            opt.set_max_grad_norm(args.max_grad_norm)
        if ema is not None:
            best_ema = ema_resume(ema, ck, rank)
        if rank == 0:
            print(f"Resuming from epoch {start_epoch} (best loss {best:.5f}, scale factor {scale_factor})")
    save_weighting = args.loss_weighting is not None             # (after the resume: a restored setting is written again)
    wkw = step_weighting(args)                                   # {} without the flags: the plain exports, as before
    GA = int(args.grad_accum_steps or 1)                         # micro-batches per optimizer step
    K = int(args.loss_by_noise_level)
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
            eps = randn(ctx, (B, args.latent_channels, x.shape[2] // stage1.down), seed=s_eps, offset=gstep * z[0].numel() * B)
            noise = randn(ctx, eps.shape, seed=s_noise, offset=gstep * z[0].numel() * B)
            e = stage1.encode_stage_2_inputs(x, eps=eps, scale_factor=scale_factor)
            if zero:
                opt.zero_grad()
            lab = dict(labels=batch["label"].to(dev), p_uncond=args.p_uncond, null_class=null_class, seed=s_lab, offset=gstep * B) if cond else {}
            if train_levels is not None:
                wkw["per_sample_out"] = torch.empty(B, device=dev)
            if centry is not None:         # draw the masks, mask the windows, encode them once more: the context the model will see at repair time
                m = context_mask(ctx, B, e.shape[2], cspec, seed=s_mask, offset=gstep * B)
                lab = dict(lab, context_mask=m, context_latents=context_latents(unet, stage1, x, m, scale_factor))
            ldm_train_step(unet, sched, e, noise, t, loss_out=loss, grad_scale=scaler.get_scale() / GA, grad_sync=gsync if last else None, **lab, **wkw)
            if train_levels is not None:
                train_levels.add(wkw["per_sample_out"], t, ctx=ctx)
            if last:                       # one all-reduce and one optimizer step per group; a short group counts its k micro-batches K / k
                gsync.wait()
                scaler.step(opt, accum_factor(GA, k)); scaler.update()
            steps += 1; gstep += 1; seen += B * world
            if args.max_steps and steps >= args.max_steps:
                break
        do_eval = (epoch + 1) % config.train.get("eval_freq", 1) == 0 or bool(args.max_steps and steps >= args.max_steps)
        cur = float(loss)
        lv, lv_ema = (NoiseLevelLoss(sched.num_train_timesteps, K), NoiseLevelLoss(sched.num_train_timesteps, K)) if K else (None, None)
        if do_eval and valid is not None:      # model selection on the validation split (training.py:356-380), epsilon MSE over its windows
            v_sum, v_n = D.allreduce_sum_scalars(validate(unet, stage1, sched, valid, scale_factor, v_seeds, args.latent_channels, by_level=lv, context=v_context), like=loss)
            cur = v_sum / max(1.0, v_n)
        cur_ema = None                         # no validation split: no loss of the averaged weights exists
        if do_eval and valid is not None and ema is not None:      # the same windows and noise, scored with the averaged weights
            with ema.applied():
                e_sum, e_n = D.allreduce_sum_scalars(validate(unet, stage1, sched, valid, scale_factor, v_seeds, args.latent_channels, by_level=lv_ema, context=v_context), like=loss)
            cur_ema = e_sum / max(1.0, e_n)
        if K and do_eval:                      # every rank joins the sums; rank 0 prints and writes
            record = {"epoch": epoch + 1, "steps": gstep, "prediction_type": sched.prediction_type, "bins": K,
                      "train": train_levels.merge(like=loss).table(),
                      "valid": lv.merge(like=loss).table() if valid is not None else None,
                      "valid_ema": lv_ema.merge(like=loss).table() if valid is not None and ema is not None else None}
        if rank == 0:
            print(f"epoch {epoch}: loss {float(loss):.5f} | {seen/(time.time()-t0):.1f} windows/s" + (format_clip_stats(opt) if opt.max_grad_norm is not None else ""), flush=True)
            if K and do_eval:
                for name in ("train", "valid", "valid_ema"):
                    if record[name] is not None:
                        print(format_noise_level_table(name, record[name]), flush=True)
                append_noise_level_record(run_dir, record)
            if do_eval:
                new_best = cur <= best
                if new_best:
                    best = cur
                    torch.save({k: v.cpu() for k, v in unet.state_dict().items()}, os.path.join(run_dir, "best_model.pth"))
                ck_out = {"epoch": epoch + 1, "diffusion": {k: v.cpu() for k, v in unet.state_dict().items()}, "optimizer": opt.state_dict(),
                          "best_loss": best, "scale_factor": torch.tensor(scale_factor, dtype=torch.float64), "scaler": scaler.state_dict(), "steps": gstep}
                # (float64: the Python float the run multiplies its latents with, exactly -- a resumed run then continues bit for bit)
                if ema is not None:            # its own best on its own validation loss; without one, whenever best_model.pth is written
                    if cur_ema is not None:
                        new_best = cur_ema <= best_ema
                        best_ema = min(best_ema, cur_ema)
                    if new_best:
                        torch.save(cpu_state(ema.state_dict()), os.path.join(run_dir, "best_model_ema.pth"))
                    ck_out["ema"] = ema_checkpoint_entry(ema, best_ema)
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
    LAST_RUN.clear(); LAST_RUN.update(rank=rank, world=world, scale_factor=scale_factor, steps=steps, param_sum=float(unet.flat.double().sum()),
                                     loss_weighting=args.loss_weighting, snr_gamma=args.snr_gamma, opt_steps=opt.step_count, sync_rounds=gsync.rounds,
                                     flat_sha1=hashlib.sha1(unet.flat.cpu().numpy().tobytes()).hexdigest(),
                                     grad_norm_bits=None if opt.max_grad_norm is None else int(opt.grad_norm.view(torch.int32)))
    return run_dir


if __name__ == "__main__":
    main(parse_args())
