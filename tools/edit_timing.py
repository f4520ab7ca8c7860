"""Cost of sampling from an input (init / strength / mask) on the config_ldm UNet (bf16), one JSON line per measurement.  All variants of
a measurement alternate inside one process; every figure is the median of --iters x --rounds calls (device events around the whole native
sampling call, decode included); the spread of the round medians is what a difference has to exceed to mean anything.

  edit     per sampler (DDIM-50, DPM-Solver++ 2M-20), B = 256 and B = 1, plain and guided (w = 3 on a class-conditional UNet):
             plain          sample() from noise, the existing export
             edit_s1        init_latents + mask, strength 1: the same number of steps, every step launch with the blend
             edit_s05       the same at strength 0.5 (half the steps)
             edit_s1_win    init (windows) + mask, strength 1: encode, mask pooling and composite included
  plain    sample() from noise only, tagged with --tag: run once per library (EEGLDM_LIB) to compare two builds
  --parent_lib PATH   runs `--only plain` in fresh child processes, alternating PATH (EEGLDM_LIB) and the tree's own library, --ab_rounds times

    python tools/edit_timing.py [--iters 5] [--rounds 5] [--only edit|plain] [--parent_lib libeegldm_parent.so] > profiles/edit_timing.txt
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
    ap.add_argument("--only", default=None, choices=[None, "edit", "plain"])
    ap.add_argument("--tag", default="this tree")
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--ab_rounds", type=int, default=3)
    args = ap.parse_args()
    if args.parent_lib:
        for _ in range(args.ab_rounds):
            for tag, lib in (("parent", os.path.abspath(args.parent_lib)), ("this tree", None)):
                env = dict(os.environ)
                env.pop("EEGLDM_LIB", None)
                if lib:
                    env["EEGLDM_LIB"] = lib
                subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "plain", "--tag", tag, "--iters", str(args.iters), "--rounds",
                                str(args.rounds)], env=env, check=True)
        return
    import torch
    from eegldm.models import AutoencoderKL, UNetModel
    from eegldm.sampling import make_sampling_scheduler, sample
    from eegldm.training import randn
    from make_golden_cases import UNET_FULL

    def seeded(net, seed):
        g = torch.Generator().manual_seed(seed)
        net.load_state_dict({k: (torch.randn(v.shape, generator=g) * 0.02 if float(v.abs().sum()) == 0.0 else v) for k, v in net.state_dict().items()})
        return net

    torch.manual_seed(0)
    unet = seeded(UNetModel(**UNET_FULL[0], dtype="bfloat16"), 42)
    cond = seeded(UNetModel(**UNET_FULL[0], num_classes=6, dtype="bfloat16"), 43)
    ae = AutoencoderKL(spatial_dims=1, in_channels=1, out_channels=1, num_channels=[32, 32, 64], latent_channels=1, num_res_blocks=2,
                       norm_num_groups=1, attention_levels=[False] * 3, dtype="bfloat16")
    ctx, L = unet.ctx, 768

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
        return {k: dict(median_ms=round(sorted(every[k])[len(every[k]) // 2], 3), round_medians_ms=[round(min(rounds[k]), 3), round(max(rounds[k]), 3)],
                        min_ms=round(min(every[k]), 3), max_ms=round(max(every[k]), 3)) for k in variants}

    for B in (256, 1):
        noise = randn(ctx, (B, 1, L), seed=7)
        for guided in (False, True):
            net = cond if guided else unet
            g = dict(labels=[b % 5 for b in range(B)], guidance_scale=3.0, null_class=5) if guided else {}
            for sampler, N in (("ddim", 50), ("dpmpp_2m", 20)):
                sched = make_sampling_scheduler(N, sampler=sampler)
                v = {"plain": lambda: sample(net, ae, sched, noise, **g)}
                if args.only != "plain":
                    init = randn(ctx, (B, 1, 4 * L), seed=8) * 0.5
                    z0 = randn(ctx, (B, 1, L), seed=9)
                    mask = torch.ones(B, 1, 4 * L, device=unet.device)
                    mask[:, :, 1000:1600] = 0.0
                    v["edit_s1"] = lambda: sample(net, ae, sched, noise, init_latents=z0, mask=mask, strength=1.0, **g)
                    v["edit_s05"] = lambda: sample(net, ae, sched, noise, init_latents=z0, mask=mask, strength=0.5, **g)
                    v["edit_s1_win"] = lambda: sample(net, ae, sched, noise, init=init, mask=mask, strength=1.0, **g)
                res = measure(v)
                p = res["plain"]
                extra = {}
                if args.only != "plain":
                    spread = p["round_medians_ms"][1] - p["round_medians_ms"][0]
                    excess = res["edit_s1"]["median_ms"] - p["median_ms"]
                    extra = dict(plain_spread_ms=round(spread, 3), edit_s1_excess_ms=round(excess, 3), excess_per_step_us=round(1e3 * excess / N, 2),
                                 inside_plain_spread=bool(abs(excess) <= spread), s05_over_s1=round(res["edit_s05"]["median_ms"] / res["edit_s1"]["median_ms"], 4))
                emit(what="plain_sampling" if args.only == "plain" else "edit_vs_plain", library=args.tag, sampler=f"{sampler}_{N}", B=B, guided=guided,
                     iters=args.iters, rounds=args.rounds, **extra, **res)


if __name__ == "__main__":
    main()
