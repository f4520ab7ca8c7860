"""Cost of resampled repair (RePaint jumps), one JSON line per measurement.  Device events; the variants of a measurement alternate inside
one process; every figure is the median of --iters x --rounds (5 x 5 = 25) timed calls, and the spread of the five round medians is what
a difference has to exceed to mean anything (as tools/sampler_timing.py).

  jump     eegldm_edit_jump with the draw in registers (fresh = NULL) against the composed form (eegldm_randn into a buffer, then the jump
           with fresh = that buffer), with a mask, in place, at n = 256 * 768 and n = 768.  A timed call is --reps launches back to back;
           the figures are per jump.  Achieved GB/s at the large n, from the bytes each form has to move: x, known, noise, mask in and x
           out (5 n floats) for the fused form, plus the noise buffer written and read (7 n floats) for the composed one.
  call     the whole sample(init_latents, mask) call (config_ldm UNet, bf16, DPM-Solver++ 2M-20, decode included) at B = 256 and B = 1:
             repair_r1      resamples = 1: the call made before resampling existed (eegldm_sample_edit)
             resample_j2_r3 jump_length 2, resamples 3: 56 forwards and 18 jumps, reported beside 56 / 20 times repair_r1
  --parent_lib PATH   runs `--only call --plain_only` in fresh child processes, alternating PATH (EEGLDM_LIB: a library built at the parent
           commit, which serves resamples = 1 through the old export) and the tree's own library, --ab_rounds times: the new library's
           repair_r1 has to sit inside the parent's own spread of round medians.

    python tools/resample_timing.py [--parent_lib libeegldm_parent.so] > profiles/resample_timing.txt
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="jump launches per timed call")
    ap.add_argument("--only", default=None, choices=[None, "jump", "call"])
    ap.add_argument("--plain_only", action="store_true", help="call: resamples = 1 only (what a parent library can serve)")
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--ab_rounds", type=int, default=2)
    args = ap.parse_args()
    if args.parent_lib:
        for _ in range(args.ab_rounds):
            for tag, lib in (("parent", os.path.abspath(args.parent_lib)), ("this tree", None)):
                env = dict(os.environ)
                env.pop("EEGLDM_LIB", None)
                if lib:
                    env["EEGLDM_LIB"] = lib
                subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "call", "--plain_only", "--tag", tag, "--iters", str(args.iters),
                                "--rounds", str(args.rounds)], env=env, check=True)
        return
    import torch
    import eegldm
    from eegldm._lib import check, lib, ptr
    from eegldm.training import randn

    ctx = eegldm.default_context(0)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def measure(variants):
        def timed(fn):
            ctx.timer_start(); fn(); return ctx.timer_stop_ms()
        for fn in variants.values():
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

    if args.only != "call":
        for n in (256 * 768, 768):
            x, known, noise, fresh = (randn(ctx, (n,), seed=s) for s in (1, 2, 3, 4))
            mask = (torch.arange(n, device=x.device) % 7 < 4).float()
            q = (n + 3) // 4

            def fused():
                for k in range(args.reps):
                    check(lib.eegldm_edit_jump(ctx.h, ptr(x), 0.999, 0.0447, None, 11, k * q, ptr(known), ptr(noise), ptr(mask), 0.5, ptr(x), None, n))

            def composed():
                for k in range(args.reps):
                    check(lib.eegldm_randn(ctx.h, ptr(fresh), n, 11, k * q))
                    check(lib.eegldm_edit_jump(ctx.h, ptr(x), 0.999, 0.0447, ptr(fresh), 0, 0, ptr(known), ptr(noise), ptr(mask), 0.5, ptr(x), None, n))

            res = measure({"fused_draw": fused, "randn_then_jump": composed})
            per = {k: {kk: ([round(1e3 * t / args.reps, 3) for t in vv] if isinstance(vv, list) else round(1e3 * vv / args.reps, 3)) for kk, vv in v.items()}
                   for k, v in res.items()}
            per = {k: {kk.replace("_ms", "_us"): vv for kk, vv in v.items()} for k, v in per.items()}
            extra = {}
            if n >= 1 << 16:
                extra = dict(fused_GBps=round(5 * 4 * n / (per["fused_draw"]["median_us"] * 1e-6) / 1e9, 1),
                             composed_GBps=round(7 * 4 * n / (per["randn_then_jump"]["median_us"] * 1e-6) / 1e9, 1))
            emit(what="edit_jump", n=n, reps=args.reps, iters=args.iters, rounds=args.rounds, unit="us per jump",
                 composed_over_fused=round(per["randn_then_jump"]["median_us"] / per["fused_draw"]["median_us"], 3), **extra, **per)
    if args.only == "jump":
        return

    from eegldm.models import AutoencoderKL, UNetModel
    from eegldm.sampling import make_sampling_scheduler, sample
    from make_golden_cases import UNET_FULL

    def seeded(net, seed):
        g = torch.Generator().manual_seed(seed)
        net.load_state_dict({k: (torch.randn(v.shape, generator=g) * 0.02 if float(v.abs().sum()) == 0.0 else v) for k, v in net.state_dict().items()})
        return net

    torch.manual_seed(0)
    unet = seeded(UNetModel(**UNET_FULL[0], dtype="bfloat16"), 42)
    ae = AutoencoderKL(spatial_dims=1, in_channels=1, out_channels=1, num_channels=[32, 32, 64], latent_channels=1, num_res_blocks=2,
                       norm_num_groups=1, attention_levels=[False] * 3, dtype="bfloat16")
    L, N = 768, 20
    sched = make_sampling_scheduler(N, sampler="dpmpp_2m")
    for B in (256, 1):
        noise = randn(unet.ctx, (B, 1, L), seed=7)
        z0 = randn(unet.ctx, (B, 1, L), seed=9)
        mask = torch.ones(B, 1, 4 * L, device=unet.device)
        mask[:, :, 1000:1600] = 0.0
        v = {"repair_r1": lambda: sample(unet, ae, sched, noise, init_latents=z0, mask=mask)}
        info = {}
        if not args.plain_only:
            v["resample_j2_r3"] = lambda: sample(unet, ae, sched, noise, init_latents=z0, mask=mask, resamples=3, jump_length=2, info=info)
        res = measure(v)
        extra = {}
        if not args.plain_only:
            p = res["repair_r1"]["median_ms"]
            extra = dict(forwards=info["forwards"], by_forward_count_ms=round(p * info["forwards"] / N, 3),
                         measured_over_forward_count=round(res["resample_j2_r3"]["median_ms"] / (p * info["forwards"] / N), 4))
        emit(what="sample_init_mask", library=args.tag, sampler=f"dpmpp_2m_{N}", B=B, iters=args.iters, rounds=args.rounds, **extra, **res)


if __name__ == "__main__":
    main()
