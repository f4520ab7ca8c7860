"""Cost of the weighted diffusion loss inside the LDM train step: config_ldm UNet, bf16, B = 256, L = 768, device events around the whole
native step (zero_grad + ldm_train_step), one JSON line per measurement.  The variants of a measurement alternate call by call inside
one process; every figure is the median of --iters calls, repeated --rounds times (the spread of the round medians is what a
difference has to exceed to mean anything):

  old         ldm_train_step()                              add_noise -> forward -> [get_velocity] -> mse_loss -> backward
  none        ldm_train_step(loss_weighting="none")         ... -> diffusion_loss (wtab NULL) -> backward
  min_snr     ldm_train_step(loss_weighting="min_snr")      ... -> diffusion_loss (Min-SNR table, per-sample losses) -> backward

for epsilon and for v_prediction, and the loss launches alone (mse_loss [+ get_velocity] against diffusion_loss).

    python tools/loss_weighting_timing.py [--iters 100] [--rounds 5]
    python tools/loss_weighting_timing.py --parent_lib /path/to/parent/libeegldm.so

--parent_lib: the old export on this tree's library and on a library built from the parent commit, alternated RUN by run (a process
binds one library: EEGLDM_LIB selects it; each run is a fresh child process with `--only old`).
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


def measure(ctx, variants, iters, rounds):
    """{name: fn} -> {name: {"median_ms", "round_medians_ms": [min, max], "min_ms", "max_ms"}}, variants alternated call by call."""
    def timed(fn):
        ctx.timer_start(); fn(); return ctx.timer_stop_ms()
    for fn in variants.values():
        for _ in range(3):
            fn()
    per_round = {k: [] for k in variants}; every = {k: [] for k in variants}
    for _ in range(rounds):
        ts = {k: [] for k in variants}
        for _ in range(iters):
            for k, fn in variants.items():
                ts[k].append(timed(fn))
        for k in variants:
            per_round[k].append(sorted(ts[k])[len(ts[k]) // 2]); every[k] += ts[k]
    return {k: dict(median_ms=round(sorted(every[k])[len(every[k]) // 2], 4), round_medians_ms=[round(min(per_round[k]), 4), round(max(per_round[k]), 4)],
                    min_ms=round(min(every[k]), 4), max_ms=round(max(every[k]), 4)) for k in variants}


def run(args):
    import torch
    from eegldm._lib import PRED, lib, check, ptr
    from eegldm.models import UNetModel
    from eegldm.schedulers import DDPMScheduler
    from eegldm.training import ldm_train_step, randint, randn
    from make_golden_cases import UNET_FULL
    torch.manual_seed(0)
    net = UNetModel(**UNET_FULL[0], dtype="bfloat16")
    g = torch.Generator().manual_seed(42)
    net.load_state_dict({k: (torch.randn(v.shape, generator=g) * 0.02 if float(v.abs().sum()) == 0.0 else v) for k, v in net.state_dict().items()})
    net.train()
    ctx, dev = net.ctx, net.device
    B, L = 256, 768
    lat = randn(ctx, (B, 1, L), seed=1); nz = randn(ctx, (B, 1, L), seed=2)
    loss, per = torch.zeros(1, device=dev), torch.empty(B, device=dev)
    count = [0]
    lib_name = os.environ.get("EEGLDM_LIB", "in-tree")
    for pred in ("epsilon", "v_prediction"):
        sched = DDPMScheduler(num_train_timesteps=1000, schedule="linear_beta", beta_start=0.0015, beta_end=0.0195, prediction_type=pred, device=0)

        def step(**kw):
            def fn():
                count[0] += 1
                t = randint(ctx, B, 1000, seed=3, offset=count[0] * B)
                net.zero_grad()
                ldm_train_step(net, sched, lat, nz, t, loss_out=loss, **kw)
            return fn
        variants = {"old": step()}
        if args.only != "old":
            variants.update(none=step(loss_weighting="none"), min_snr=step(loss_weighting="min_snr", per_sample_out=per))
        print(json.dumps(dict(what="ldm_train_step_b256_bf16", prediction_type=pred, lib=lib_name, iters=args.iters, rounds=args.rounds,
                              **measure(ctx, variants, args.iters, args.rounds))), flush=True)
        if args.only == "old":
            continue
        from eegldm.schedulers import device_loss_weights
        wtab = device_loss_weights(sched, "min_snr", 5.0)
        t = randint(ctx, B, 1000, seed=4)
        pr, tgt, dp = randn(ctx, (B, 1, L), seed=5), torch.empty(B, 1, L, device=dev), torch.empty(B, 1, L, device=dev)
        n = pr.numel()

        def old_loss():
            target = nz
            if pred == "v_prediction":
                check(lib.eegldm_get_velocity(ctx.h, ptr(lat), ptr(nz), ptr(t), ptr(sched._acp_dev), ptr(tgt), B, L)); target = tgt
            check(lib.eegldm_mse_loss(ctx.h, ptr(pr), ptr(target), ptr(loss), ptr(dp), n, 1.0))

        def new_loss():
            check(lib.eegldm_diffusion_loss(ctx.h, ptr(pr), ptr(lat), ptr(nz), ptr(t), ptr(sched._acp_dev), ptr(wtab), PRED[pred], B, L, 1.0, ptr(loss),
                                            ptr(per), ptr(dp)))
        print(json.dumps(dict(what="loss_launches_alone_b256", prediction_type=pred, iters=args.iters, rounds=args.rounds,
                              **measure(ctx, {"old_mse": old_loss, "diffusion_loss": new_loss}, args.iters, args.rounds))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, choices=[None, "old"], help="old: the old export alone (works on a library without the new symbols)")
    ap.add_argument("--parent_lib", default=None, help="libeegldm.so built from the parent commit: alternate the old export against it")
    ap.add_argument("--runs", type=int, default=2, help="runs per library with --parent_lib")
    args = ap.parse_args()
    if args.parent_lib is None:
        return run(args)
    for i in range(args.runs):
        for name, path in (("parent", os.path.abspath(args.parent_lib)), ("this", None)):
            env = dict(os.environ)
            env.pop("EEGLDM_LIB", None)
            if path:
                env["EEGLDM_LIB"] = path
            print(json.dumps(dict(run=i, library=name)), flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "old", "--iters", str(args.iters), "--rounds", str(args.rounds)],
                           check=True, env=env, timeout=900)


if __name__ == "__main__":
    main()
