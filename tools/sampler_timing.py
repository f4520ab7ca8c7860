"""Cost and convergence of the DPM-Solver++ (2M) sampler on the config_ldm UNet (bf16), one JSON line per measurement.  All variants
of a measurement alternate inside one process; every figure is the median of --iters calls (device events around the whole native
sampling call, decode included), repeated --rounds times -- the spread of the round medians is what a difference has to exceed to mean
anything:

  cost        2M at N = 50 against DDIM-50, at B = 256 and B = 1, without and with guidance (w = 3 on a class-conditional UNet)
  times       2M at N = 15, 20, 25 beside DDIM-50 and DDIM-200, with the implied windows/s
  convergence err_1(N), err_2(N) = RMS(x_N - x_ref) / RMS(x_ref) on the final latents, x_ref = first order at N = 1000 on the linspace
              grid, N in {10, 15, 20, 25, 50, 100}; the smallest N with err_2(N) <= err_1(50).  The weights are the seeded random ones of
              the timing runs unless --weights names a state dict (e.g. the one tools/soak_ldm.py leaves): the output says which.

    python tools/sampler_timing.py [--iters 5] [--rounds 5] [--only cost|times|convergence] [--weights unet.pth] > profiles/sampler_timing.txt
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, choices=[None, "cost", "times", "convergence"])
    ap.add_argument("--weights", default=None)
    ap.add_argument("--conv_batch", type=int, default=8)
    args = ap.parse_args()
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
    ae = AutoencoderKL(spatial_dims=1, in_channels=1, out_channels=1, num_channels=[32, 32, 64], latent_channels=1, num_res_blocks=2,
                       norm_num_groups=1, attention_levels=[False] * 3, dtype="bfloat16")
    ctx, L = unet.ctx, 768

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def measure(variants):
        """{name: fn} -> {name: {"median_ms", "round_medians_ms": [min, max], "min_ms", "max_ms"}}, variants alternated call by call."""
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

    def runner(net, sampler, N, noise, **kw):
        sched = make_sampling_scheduler(N, sampler=sampler)
        return lambda: sample(net, ae, sched, noise, **kw)

    def with_rate(res, B):
        for v in res.values():
            v["windows_per_s"] = round(1e3 * B / v["median_ms"], 1)
        return res

    cond = None
    if args.only in (None, "cost"):
        cond = seeded(UNetModel(**UNET_FULL[0], num_classes=6, dtype="bfloat16"), 43)
    for B in (256, 1):
        noise = randn(ctx, (B, 1, L), seed=7)
        if args.only in (None, "cost"):
            res = measure({"ddim_50": runner(unet, "ddim", 50, noise), "dpmpp_2m_50": runner(unet, "dpmpp_2m", 50, noise)})
            d, m = res["ddim_50"], res["dpmpp_2m_50"]
            spread = d["round_medians_ms"][1] - d["round_medians_ms"][0]
            emit(what="cost_per_step_equal_N", B=B, guided=False, iters=args.iters, rounds=args.rounds, ddim_spread_ms=round(spread, 3),
                 excess_ms=round(m["median_ms"] - d["median_ms"], 3), within_twice_the_spread=bool(m["median_ms"] - d["median_ms"] <= 2 * spread), **res)
            g = dict(labels=[b % 5 for b in range(B)], guidance_scale=3.0, null_class=5)
            res = measure({"ddim_50": runner(cond, "ddim", 50, noise, **g), "dpmpp_2m_50": runner(cond, "dpmpp_2m", 50, noise, **g)})
            d, m = res["ddim_50"], res["dpmpp_2m_50"]
            spread = d["round_medians_ms"][1] - d["round_medians_ms"][0]
            emit(what="cost_per_step_equal_N", B=B, guided=True, iters=args.iters, rounds=args.rounds, ddim_spread_ms=round(spread, 3),
                 excess_ms=round(m["median_ms"] - d["median_ms"], 3), within_twice_the_spread=bool(m["median_ms"] - d["median_ms"] <= 2 * spread), **res)
        if args.only in (None, "times"):
            v = {"ddim_50": runner(unet, "ddim", 50, noise), "ddim_200": runner(unet, "ddim", 200, noise)}
            v.update({f"dpmpp_2m_{N}": runner(unet, "dpmpp_2m", N, noise) for N in (15, 20, 25)})
            emit(what="sampling_call", B=B, guided=False, iters=args.iters, rounds=args.rounds, **with_rate(measure(v), B))

    if args.only in (None, "convergence"):
        weights = "seeded random (N(0, 0.02) in the zero-initialised layers, the constructor's draw elsewhere)"
        if args.weights:
            unet.load_state_dict(torch.load(args.weights, map_location="cpu")); weights = os.path.basename(args.weights)
        noise = randn(ctx, (args.conv_batch, 1, L), seed=11)
        rms = lambda t: float(t.double().pow(2).mean().sqrt())

        def latents(N, order):
            return sample(unet, None, make_sampling_scheduler(N, sampler="dpmpp_2m", solver_order=order), noise, crop=0)[1]
        ref = latents(1000, 1)
        err = {N: [rms(latents(N, o) - ref) / rms(ref) for o in (1, 2)] for N in (10, 15, 20, 25, 50, 100)}
        reach = [N for N in sorted(err) if err[N][1] <= err[50][0]]
        emit(what="convergence", weights=weights, B=args.conv_batch, dtype="bfloat16", reference="first order, N = 1000, linspace grid",
             err1={N: round(e[0], 5) for N, e in err.items()}, err2={N: round(e[1], 5) for N, e in err.items()},
             smallest_N_with_err2_le_err1_at_50=reach[0] if reach else None,
             note="a convergence measure towards this network's own ODE solution, not sample quality on sleep data")


if __name__ == "__main__":
    main()
