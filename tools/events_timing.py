"""Time of the micro-structure primitives (csrc/events.hip) with device events: eegldm_fir_same against torch.nn.functional.conv1d in fp32 on
the same data (zero padding, plain mode), as the call chooses its register blocking and for every blocking R the kernel is built with
(EEGLDM_FIR_R = 4, 8, 12); eegldm_threshold_events on a band envelope (it has no counterpart); and the whole eegldm.metrics.detect_spindles.  The variants alternate
inside one process; every figure is the median of --iters calls (25), repeated --rounds times (5): the spread of the round medians is what a
difference has to exceed to mean anything.

    python tools/events_timing.py [--iters 25] [--rounds 5] [--out profiles/events_timing.txt]

Shapes (B, L, M): (4096, 3072, 165), a 2-Hz-transition band-pass over a chunk of the held-out set, and (4096, 3072, 1101), a 0.3-Hz transition.
The GFLOP/s figure counts 2 B L M FLOP per call; the fp32 vector ALU of the MI355X peaks at 157 TF/s.  No rate is a gate: the numbers are
written down whichever way they fall."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(4096, 3072, 165), (4096, 3072, 1101)]
F32_VALU_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_timing.txt"))
    ap.add_argument("--shapes", default=None, help="e.g. 4096,3072,165;256,3000,1101")
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from eegldm import metrics as M
    from eegldm._lib import check, default_context, lib, ptr
    shapes = SHAPES if not args.shapes else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    lines = []

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    def timed(fn):
        ctx.timer_start(); fn(); return ctx.timer_stop_ms()

    def set_r(r):
        if r:
            os.environ["EEGLDM_FIR_R"] = str(r)
        else:
            os.environ.pop("EEGLDM_FIR_R", None)
        lib.eegldm_debug_reload_env()

    def measure(variants):
        """{name: (median over all calls, smallest and largest round median)}; the variants alternate call by call."""
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        rounds = {n: [] for n in variants}; every = {n: [] for n in variants}
        for _ in range(args.rounds):
            ts = {n: [] for n in variants}
            for _ in range(args.iters):
                for n, fn in variants.items():
                    ts[n].append(timed(fn))
            for n in variants:
                rounds[n].append(sorted(ts[n])[len(ts[n]) // 2]); every[n] += ts[n]
        return {n: (sorted(every[n])[len(every[n]) // 2], min(rounds[n]), max(rounds[n])) for n in variants}

    for b, length, m in shapes:
        g = torch.Generator(device=dev).manual_seed(b + length + m)
        x = torch.randn(b, length, device=dev, generator=g)
        taps = torch.from_numpy(M.fir_design(100.0, 11.0, 16.0, 330.0 / (m - 0.5)).astype(np.float32)).to(dev)
        assert taps.numel() == m, (taps.numel(), m)
        y, ty = torch.empty_like(x), None
        w = taps.view(1, 1, m)                                    # conv1d is a correlation: the same sum, taps are symmetric anyway

        def native(r):
            def run():
                set_r(r)
                check(lib.eegldm_fir_same(ctx.h, ptr(x), length, ptr(taps), m, ptr(y), length, b, length, 0, 0))
            return run

        def torch_conv():
            nonlocal ty
            ty = F.conv1d(x.view(b, 1, length), w, padding=m // 2)

        tf32 = torch.backends.cudnn.allow_tf32
        torch.backends.cudnn.allow_tf32 = False
        variants = {"native_fir_same": native(0), "native_fir_same_R12": native(12), "native_fir_same_R8": native(8), "native_fir_same_R4": native(4), "torch_conv1d_fp32": torch_conv}
        res = measure(variants)
        set_r(0)
        torch.backends.cudnn.allow_tf32 = tf32
        native(0)(); torch.cuda.synchronize()
        rel = float((y - ty.view(b, length)).abs().max() / ty.abs().max())
        flop = 2.0 * b * length * m
        for n, (med, lo, hi) in res.items():
            emit(shape=dict(B=b, L=length, M=m), variant=n, median_ms=round(med, 3), round_medians_ms=[round(lo, 3), round(hi, 3)],
                 GFLOP_per_s=round(flop / (med * 1e-3) / 1e9, 1), share_of_f32_valu_157TF=round(flop / (med * 1e-3) / 1e12 / F32_VALU_TF, 3),
                 iters=args.iters, rounds=args.rounds, max_rel_difference_native_vs_torch=float(f"{rel:.3e}"))
    set_r(0)

    # the run extraction and the whole detector on 18-Hz-low-passed noise, threshold at mean + 1.5 sd of its own envelope
    b, length = shapes[0][0], 3000
    g = torch.Generator(device=dev).manual_seed(1)
    white = torch.randn(b, 1, length + 82, device=dev, generator=g)
    lp = torch.from_numpy(M.fir_design(100.0, hi=18.0, trans_hz=4.0).astype(np.float32)).to(dev)
    x = F.conv1d(white, lp.view(1, 1, -1))[:, 0].contiguous()
    band, env = M.band_envelope(x, 11.0, 16.0)
    thr = float(env.double().mean() + 1.5 * env.double().std())
    thr_d = torch.full((b,), thr, device=dev)
    counts = torch.zeros(b, 2, dtype=torch.int32, device=dev); ev_i = torch.zeros(b, 32, 6, dtype=torch.int32, device=dev)
    ev_f = torch.zeros(b, 32, 4, device=dev)

    def events():
        check(lib.eegldm_threshold_events(ctx.h, ptr(env), length, ptr(band), length, ptr(thr_d), b, length, 50, 300, 10, 1, 32, ptr(counts), ptr(ev_i), ptr(ev_f)))

    found = {}

    def detector():
        found["table"] = M.detect_spindles(x, thr)

    res = measure({"native_threshold_events": events, "detect_spindles_whole": detector})
    torch.cuda.synchronize()
    for n, (med, lo, hi) in res.items():
        emit(shape=dict(B=b, L=length), variant=n, median_ms=round(med, 3), round_medians_ms=[round(lo, 3), round(hi, 3)],
             windows_per_s=round(b / (med * 1e-3)), events_kept=int(counts[:, 0].sum()), raw_runs=int(counts[:, 1].sum()), iters=args.iters, rounds=args.rounds,
             note="device events around the call; detect_spindles includes its host side (table copies, numpy)" if n.startswith("detect") else "no counterpart")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
