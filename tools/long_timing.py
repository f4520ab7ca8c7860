"""Cost of long-recording sampling (sample_long: overlapped windows on one canvas) beside plain window sampling at the same number of
forward rows, config_ldm UNet, bf16, DPM-Solver++ 2M at 20 steps, one JSON line per measurement.  Variants alternate call by call inside
one process; every figure is the median of --iters calls (device events around the whole native call, decode included), repeated
--rounds times -- the spread of the round medians is what a difference has to exceed to mean anything:

  long_vs_plain   sample_long with R * W rows against sample at B = R * W, for R * W = 21 (one 10-minute recording) and 256 (16 x 16)
  canvas_step     eegldm_canvas_step alone at those shapes, with the bytes it moves (model output in, canvas and history in and out,
                  window rows out) and the implied GB/s

    python tools/long_timing.py [--iters 25] [--rounds 5] > profiles/long_timing.txt
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
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from eegldm._lib import check, lib, ptr
    from eegldm.models import AutoencoderKL, UNetModel
    from eegldm.sampling import long_layout, make_sampling_scheduler, sample, sample_long
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
    ctx, L, m, r = unet.ctx, 768, 18, 36
    sched = make_sampling_scheduler(args.steps, sampler="dpmpp_2m")

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

    for R, W in ((1, 21), (16, 16)):
        lay = long_layout(W, L, m, r)
        B = R * W
        cnoise, wnoise = randn(ctx, (R, 1, lay.canvas_len), seed=7), randn(ctx, (B, 1, L), seed=8)
        res = measure({"sample_long": lambda: sample_long(unet, ae, sched, cnoise, W, margin=m, ramp=r),
                       "sample_plain": lambda: sample(unet, ae, sched, wnoise)})
        lg, pl = res["sample_long"], res["sample_plain"]
        emit(what="long_vs_plain", R=R, W=W, rows=B, steps=args.steps, iters=args.iters, rounds=args.rounds, canvas_len=lay.canvas_len,
             seconds_per_recording=round((lay.canvas_len * 4 - 72) / 100.0, 2), excess_ms=round(lg["median_ms"] - pl["median_ms"], 4),
             plain_spread_ms=round(pl["round_medians_ms"][1] - pl["round_medians_ms"][0], 4), **res)
        # the step kernel alone
        n, nw = R * lay.canvas_len, B * L
        mo, canvas, hist, win = (randn(ctx, (k,), seed=9 + i) for i, k in enumerate((nw, n, n, nw)))

        def step():
            for _ in range(10):
                check(lib.eegldm_canvas_step(ctx.h, ptr(mo), 0.0, 0, ptr(canvas), ptr(hist), 0.5, 0, 0, 0.9, 0.3, -0.1, R, 1, W, L, m, r, ptr(canvas),
                                             ptr(win), None, None))
        st = measure({"canvas_step_x10": step})["canvas_step_x10"]
        moved = 4 * (nw + 2 * n + 2 * n + nw)          # model_out read, canvas + history read and written, window rows written
        emit(what="canvas_step", R=R, W=W, rows=B, bytes=moved, us_per_launch=round(100.0 * st["median_ms"], 3),
             gb_per_s=round(moved / (st["median_ms"] * 1e-4) / 1e9, 1), round_medians_ms_x10=st["round_medians_ms"])


if __name__ == "__main__":
    main()
