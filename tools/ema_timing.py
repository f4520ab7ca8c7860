"""Cost of the weight EMA on the config_ldm UNet (bf16, 30.5 M parameters), one JSON line per measurement.  All variants of a
measurement alternate inside one process; every figure is the median of --iters calls, repeated --rounds times (the spread of the
round medians is what a difference has to exceed to mean anything):

  optimizer   (a) Adam.step = adam_step + sync_weights          (the path without EMA)
              (b) adam_step_ema + sync_weights                  (Adam(ema=...).step, EMA fused into the Adam pass)
              (c) adam_step + ema_update + sync_weights         (the composed form)
              and the three kernels alone, without sync_weights
  train       (d) whole LDM train step at B = 256, L = 768 (zero_grad, ldm_train_step, optimizer step) without / with EMA
  applied     (e) EMA.applied() enter + exit (two exchanges + two sync_weights)

    python tools/ema_timing.py [--iters 20] [--rounds 5] [--only optimizer|train|applied|adam_plain]

`--only adam_plain` needs nothing of the EMA entry points: it measures (a) alone, also on a library built from an earlier commit
(EEGLDM_LIB=/path/to/libeegldm.so).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, choices=[None, "optimizer", "train", "applied", "adam_plain"])
    args = ap.parse_args()
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

    def measure(variants):
        """{name: fn} -> {name: {"median_ms", "round_medians_ms": [min, max], "min_ms", "max_ms"}}, variants alternated call by call."""
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
        return {k: dict(median_ms=round(sorted(every[k])[len(every[k]) // 2], 4), round_medians_ms=[round(min(rounds[k]), 4), round(max(rounds[k]), 4)],
                        min_ms=round(min(every[k]), 4), max_ms=round(max(every[k]), 4)) for k in variants}

    def adam_kernel():
        plain.step_count += 1
        check(lib.eegldm_adam_step(ctx.h, ptr(net.flat), ptr(net.flat_grad), ptr(plain.m), ptr(plain.v), n, *hyper, plain.step_count, 1.0))

    if args.only == "adam_plain":
        emit(what="adam_step_plus_sync_weights", n=n, iters=args.iters, rounds=args.rounds, lib=os.environ.get("EEGLDM_LIB", "in-tree"),
             **measure({"a_adam_sync": plain.step, "adam_kernel_alone": adam_kernel}))
        return

    from eegldm.training import EMA
    ema = EMA(net, decay=0.9999)
    with_ema = Adam(net, lr=1e-4, ema=ema)
    with_ema.m, with_ema.v = plain.m, plain.v          # one set of moments: the variants touch the same bytes

    def fused_kernel():
        plain.step_count += 1
        check(lib.eegldm_adam_step_ema(ctx.h, ptr(net.flat), ptr(net.flat_grad), ptr(plain.m), ptr(plain.v), ptr(ema.shadow), n, *hyper,
                                       plain.step_count, 1.0, 1e-4))

    def ema_kernel():
        check(lib.eegldm_ema_update(ctx.h, ptr(ema.shadow), ptr(net.flat), n, 1e-4))

    def composed_kernels():
        adam_kernel(); ema_kernel()

    def composed_step():
        composed_kernels(); net.sync_weights()

    def fused_step():
        with_ema.step_count = plain.step_count; with_ema.step(); plain.step_count = with_ema.step_count

    if args.only in (None, "optimizer"):
        emit(what="optimizer_step", n=n, iters=args.iters, rounds=args.rounds,
             **measure({"a_adam_sync": plain.step, "b_fused_sync": fused_step, "c_composed_sync": composed_step}))
        emit(what="optimizer_kernels_alone", n=n, iters=args.iters, rounds=args.rounds,
             **measure({"adam": adam_kernel, "adam_ema_fused": fused_kernel, "adam_then_ema": composed_kernels, "ema_update": ema_kernel,
                        "sync_weights": net.sync_weights}))

    if args.only in (None, "applied"):
        def enter_exit():
            with ema.applied():
                pass
        emit(what="ema_applied_enter_exit", n=n, iters=args.iters, rounds=args.rounds, **measure({"e_applied": enter_exit}))

    if args.only in (None, "train"):
        sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195, device=0)
        B, L = 256, 768
        lat = randn(ctx, (B, 1, L), seed=1); nz = randn(ctx, (B, 1, L), seed=2)
        loss = torch.zeros(1, device=dev)
        count = [0]

        def step(opt):
            def run():
                count[0] += 1
                t = randint(ctx, B, 1000, seed=3, offset=count[0] * B)
                opt.zero_grad()
                ldm_train_step(net, sched, lat, nz, t, loss_out=loss)
                if opt is with_ema:
                    fused_step()
                else:
                    opt.step()
            return run
        emit(what="ldm_train_step_b256_bf16", iters=args.iters, rounds=args.rounds, **measure({"d_no_ema": step(plain), "d_ema": step(with_ema)}))


if __name__ == "__main__":
    main()
