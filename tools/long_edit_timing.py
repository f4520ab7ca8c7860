"""Cost of repairing / extending a real recording on the canvas (sample_long with init + mask) beside plain sample_long, config_ldm UNet,
bf16, DPM-Solver++ 2M at 20 steps, one JSON line per measurement.  Variants alternate call by call inside one process; every figure is
the median of --iters calls (device events around the whole call: for the edited call that includes the encode of the input, the mask
pooling and the composite), repeated --rounds times -- the spread of the round medians is what a difference has to exceed to mean anything:

  edit_vs_plain   sample_long(init=, mask=) against sample_long at R * W = 21 (one 10-minute recording) and 256 (16 x 16)
  step_kernels    eegldm_canvas_edit_step (with a mask) and eegldm_canvas_step alone at those shapes, alternated, with the bytes each
                  moves and the implied GB/s
  canvas_step     (--only step) eegldm_canvas_step alone, tagged with --tag: run once per library (EEGLDM_LIB) to compare two builds
  --parent_lib PATH   runs `--only step` in fresh child processes, alternating PATH (EEGLDM_LIB) and the tree's own library, --ab_rounds times

    python tools/long_edit_timing.py [--iters 25] [--rounds 5] [--parent_lib /path/to/parent/libeegldm.so] > profiles/long_edit_timing.txt
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

SHAPES = ((1, 21), (16, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, choices=[None, "step"])
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
                subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "step", "--tag", tag, "--iters", str(args.iters), "--rounds",
                                str(args.rounds)], env=env, check=True)
        return
    import torch
    from eegldm._lib import check, lib, ptr
    from eegldm.sampling import long_layout
    from eegldm.training import randn
    import eegldm

    ctx, L, m, r = eegldm.default_context(0), 768, 18, 36

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

    def step_buffers(R, W):
        lay = long_layout(W, L, m, r)
        n, nw = R * lay.canvas_len, R * W * L
        return lay, n, nw, [randn(ctx, (k,), seed=9 + i) for i, k in enumerate((nw, n, n, nw, n, n))] + [torch.rand(n, device=f"cuda:{ctx.device}")]

    def plain_step(R, W, mo, canvas, hist, win):
        def go():
            for _ in range(10):
                check(lib.eegldm_canvas_step(ctx.h, ptr(mo), 0.0, 0, ptr(canvas), ptr(hist), 0.5, 0, 0, 0.9, 0.3, -0.1, R, 1, W, L, m, r, ptr(canvas),
                                             ptr(win), None, None))
        return go

    if args.only == "step":
        for R, W in SHAPES:
            lay, n, nw, (mo, canvas, hist, win, _k, _z, _m) = step_buffers(R, W)
            st = measure({"canvas_step_x10": plain_step(R, W, mo, canvas, hist, win)})["canvas_step_x10"]
            emit(what="canvas_step", lib=args.tag, R=R, W=W, us_per_launch=round(100.0 * st["median_ms"], 3), round_medians_ms_x10=st["round_medians_ms"])
        return

    from eegldm.models import AutoencoderKL, UNetModel
    from eegldm.sampling import make_sampling_scheduler, sample_long
    from make_golden_cases import UNET_FULL

    def seeded(net, seed):
        g = torch.Generator().manual_seed(seed)
        net.load_state_dict({k: (torch.randn(v.shape, generator=g) * 0.02 if float(v.abs().sum()) == 0.0 else v) for k, v in net.state_dict().items()})
        return net

    torch.manual_seed(0)
    unet = seeded(UNetModel(**UNET_FULL[0], dtype="bfloat16"), 42)
    ae = AutoencoderKL(spatial_dims=1, in_channels=1, out_channels=1, num_channels=[32, 32, 64], latent_channels=1, num_res_blocks=2,
                       norm_num_groups=1, attention_levels=[False] * 3, dtype="bfloat16")
    sched = make_sampling_scheduler(args.steps, sampler="dpmpp_2m")
    for R, W in SHAPES:
        lay, n, nw, (mo, canvas, hist, win, known, nz, mask) = step_buffers(R, W)
        cnoise = randn(ctx, (R, 1, lay.canvas_len), seed=7)
        init = randn(ctx, (R, 1, 4 * lay.canvas_len), seed=8) * 0.3
        keep = torch.ones(R, 1, 4 * lay.canvas_len, device=init.device)
        keep[:, :, 4 * lay.canvas_len // 2:] = 0.0               # the first half is real, the second is generated: the continuation case
        res = measure({"sample_long_edit": lambda: sample_long(unet, ae, sched, cnoise, W, margin=m, ramp=r, init=init, mask=keep),
                       "sample_long": lambda: sample_long(unet, ae, sched, cnoise, W, margin=m, ramp=r)})
        ed, pl = res["sample_long_edit"], res["sample_long"]
        emit(what="edit_vs_plain", R=R, W=W, rows=R * W, steps=args.steps, iters=args.iters, rounds=args.rounds, canvas_len=lay.canvas_len,
             excess_ms=round(ed["median_ms"] - pl["median_ms"], 4), plain_spread_ms=round(pl["round_medians_ms"][1] - pl["round_medians_ms"][0], 4), **res)

        def edit_step():
            for _ in range(10):
                check(lib.eegldm_canvas_edit_step(ctx.h, ptr(mo), 0.0, 0, ptr(canvas), ptr(hist), 0.5, 0.6, 0, 0, 0.9, 0.3, -0.1, R, 1, W, L, m, r, ptr(known),
                                                  ptr(nz), ptr(mask), ptr(canvas), ptr(win), None, None))
        st = measure({"canvas_edit_step_x10": edit_step, "canvas_step_x10": plain_step(R, W, mo, canvas, hist, win)})
        moved = 4 * (nw + 2 * n + 2 * n + nw)          # model_out read, canvas + history read and written, window rows written
        for k, b in (("canvas_edit_step_x10", moved + 4 * 3 * n), ("canvas_step_x10", moved)):      # + known, noise and mask read
            emit(what=k[:-4], R=R, W=W, rows=R * W, bytes=b, us_per_launch=round(100.0 * st[k]["median_ms"], 3),
                 gb_per_s=round(b / (st[k]["median_ms"] * 1e-4) / 1e9, 1), round_medians_ms_x10=st[k]["round_medians_ms"])


if __name__ == "__main__":
    main()
