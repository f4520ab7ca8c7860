"""Cost of global gradient-norm clipping on the config_ldm UNet (bf16, 30.5 M parameters), one JSON line per measurement.  All variants
of a measurement alternate inside one process; every figure is the median of --iters calls, repeated --rounds times (the spread of
the round medians is what a difference has to exceed to mean anything):

  optimizer   (a) Adam.step                                              (no clipping: adam_step + sync_weights)
              (b) Adam(max_grad_norm=...).step                           (grad_norm + adam_step_clip + sync_weights)
              (c) grad_norm + grad_scale_by + adam_step + sync_weights   (the composed form)
              (d) torch.nn.utils.clip_grad_norm_ on flat_grad, then (a)
              and the kernels alone (with the GB/s each reaches), without sync_weights
  train       (e) whole LDM train step at B = 256, L = 768 (zero_grad, ldm_train_step, optimizer step) without / with clipping

    python tools/grad_clip_timing.py [--iters 100] [--rounds 5] [--only optimizer|train] [--parent_lib /path/to/libeegldm.so]

--parent_lib: measures (a) in this process and, in a child process each, on the in-tree library and on a library built from the
parent commit (EEGLDM_LIB), so that the unclipped step can be held against the parent's spread.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def grad_holder(gbuf):
    """torch.nn.utils.clip_grad_norm_ reads the .grad of parameters: a parameter of gbuf's shape (a view of it: no second buffer) whose
    .grad IS gbuf, so that the torch variant clips the flat gradient in place."""
    import torch
    holder = torch.nn.Parameter(gbuf.detach(), requires_grad=False)
    holder.grad = gbuf
    return holder


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, choices=[None, "optimizer", "train", "adam_plain"])
    ap.add_argument("--parent_lib", default=None)
    args = ap.parse_args()
    if args.parent_lib:          # fresh child processes (the library is chosen at import), alternated: in-tree, parent, in-tree, parent
        for which in ("in-tree", "parent") * 2:
            env = dict(os.environ)
            env.pop("EEGLDM_LIB", None)
            if which == "parent":
                env["EEGLDM_LIB"] = os.path.abspath(args.parent_lib)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "adam_plain", "--iters", str(args.iters), "--rounds", str(args.rounds)],
                           env=env, check=True)
        return
    import torch
    from eegldm._lib import lib, check, ptr
    from eegldm.models import UNetModel
    from eegldm.schedulers import DDPMScheduler
    from eegldm.training import Adam, ldm_train_step, randint, randn
    from make_golden_cases import UNET_FULL
    torch.manual_seed(0)
    net = UNetModel(**UNET_FULL[0], dtype="bfloat16")
    g = torch.Generator().manual_seed(42)
    net.load_state_dict({k: (torch.randn(v.shape, generator=g) * 0.02 if float(v.abs().sum()) == 0.0 else v) for k, v in net.state_dict().items()})
    ctx, dev, n = net.ctx, net.device, net.flat.numel()
    net.flat_grad.copy_(torch.randn(n, generator=g).to(dev) * 1e-3)
    plain = Adam(net, lr=1e-4)
    hyper = (1e-4, 0.9, 0.999, 1e-8)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def timed(fn):
        ctx.timer_start(); fn(); return ctx.timer_stop_ms()

    def measure(variants, bytes_moved=None):
        for fn in variants.values():
            for _ in range(3):
                fn()
        rounds = {k: [] for k in variants}; every = {k: [] for k in variants}
        for _ in range(args.rounds):
            ts = {k: [] for k in variants}
            for _ in range(args.iters):
                for k, fn in variants.items():
                    ts[k].append(timed(fn))
            for k in variants:
                rounds[k].append(sorted(ts[k])[len(ts[k]) // 2]); every[k] += ts[k]
        out = {}
        for k in variants:
            med = sorted(every[k])[len(every[k]) // 2]
            out[k] = dict(median_ms=round(med, 4), round_medians_ms=[round(min(rounds[k]), 4), round(max(rounds[k]), 4)], min_ms=round(min(every[k]), 4),
                          max_ms=round(max(every[k]), 4))
            if bytes_moved and k in bytes_moved:
                out[k]["GB_per_s"] = round(bytes_moved[k] / (med * 1e-3) / 1e9, 1)
        return out

    def adam_kernel():
        plain.step_count += 1
        check(lib.eegldm_adam_step(ctx.h, ptr(net.flat), ptr(net.flat_grad), ptr(plain.m), ptr(plain.v), n, *hyper, plain.step_count, 1.0))

    if args.only == "adam_plain":
        emit(what="adam_step_plus_sync_weights", n=n, iters=args.iters, rounds=args.rounds, lib=os.environ.get("EEGLDM_LIB", "in-tree"),
             **measure({"a_adam_sync": plain.step, "adam_kernel_alone": adam_kernel}))
        return

    from eegldm.training import EMA
    clip = Adam(net, lr=1e-4, max_grad_norm=1.0)
    clip.m, clip.v = plain.m, plain.v                  # one set of moments: the variants touch the same bytes
    state = clip._clip
    ema = EMA(net, decay=0.9999)

    def norm_kernel():
        check(lib.eegldm_grad_norm(ctx.h, ptr(net.flat_grad), n, 1.0, 1e9, ptr(state)))      # (max_norm far above the norm: scale_by leaves the gradient as it is)

    def scale_kernel():
        check(lib.eegldm_grad_scale_by(ctx.h, ptr(net.flat_grad), n, ptr(state)))

    def clip_kernel():
        plain.step_count += 1
        check(lib.eegldm_adam_step_clip(ctx.h, ptr(net.flat), ptr(net.flat_grad), ptr(plain.m), ptr(plain.v), None, n, *hyper, plain.step_count, 1.0,
                                        0.0, ptr(state)))

    def ema_kernel():
        check(lib.eegldm_ema_update(ctx.h, ptr(ema.shadow), ptr(net.flat), n, 1e-4))

    def clipped_step():
        clip.step_count = plain.step_count; clip.step(); plain.step_count = clip.step_count

    def composed_step():
        norm_kernel(); scale_kernel(); adam_kernel(); net.sync_weights()

    def torch_clip_step():
        _torch_clip(net.flat_grad, 1e9)
        plain.step()

    holder = grad_holder(net.flat_grad)

    def _torch_clip(_gbuf, max_norm):
        torch.nn.utils.clip_grad_norm_([holder], max_norm)

    if args.only in (None, "optimizer"):
        emit(what="optimizer_step", n=n, iters=args.iters, rounds=args.rounds,
             **measure({"a_adam_sync": plain.step, "b_clip_native_sync": clipped_step, "c_composed_sync": composed_step, "d_torch_clip_sync": torch_clip_step}))
        fb = 4 * n
        emit(what="optimizer_kernels_alone", n=n, iters=args.iters, rounds=args.rounds,
             **measure({"adam": adam_kernel, "adam_clip": clip_kernel, "grad_norm": norm_kernel, "grad_scale_by": scale_kernel, "ema_update": ema_kernel,
                        "sync_weights": net.sync_weights},
                       bytes_moved={"adam": 7 * fb, "adam_clip": 7 * fb, "grad_norm": fb, "grad_scale_by": 2 * fb, "ema_update": 3 * fb}))

    if args.only in (None, "train"):
        sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195, device=0)
        B, L = 256, 768
        lat = randn(ctx, (B, 1, L), seed=1); nz = randn(ctx, (B, 1, L), seed=2)
        loss = torch.zeros(1, device=dev)
        count = [0]

        def step(clipped):
            def run():
                count[0] += 1
                t = randint(ctx, B, 1000, seed=3, offset=count[0] * B)
                plain.zero_grad()
                ldm_train_step(net, sched, lat, nz, t, loss_out=loss)
                if clipped:
                    clipped_step()
                else:
                    plain.step()
            return run
        train_iters = max(5, args.iters // 5)
        saved, args.iters = args.iters, train_iters
        emit(what="ldm_train_step_b256_bf16", iters=train_iters, rounds=args.rounds, **measure({"e_no_clip": step(False), "e_clip": step(True)}))
        args.iters = saved


if __name__ == "__main__":
    main()
