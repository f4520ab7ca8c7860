"""Time of the signal-complexity primitives (csrc/complexity.hip) with device events: eegldm_row_moments, eegldm_ordinal_counts (order 3 and 5)
and eegldm_template_matches (m = 2, scales 1 and 20, r = 0.2 sd) at (B, L) = (4096, 3000) and (8, 3000).  The template kernel is timed beside
a torch composition on the device that computes the same two counts: coarse-grain, `unfold` into templates, a Chebyshev compare of all
template pairs in chunks of rows, sums.  That composition needs c * T * T * (m + 1) floats per chunk of c rows, so it runs on the first
--torch_rows rows (64) only; both are reported per row as well.  The variants alternate inside one process; every figure is the median of
--iters calls (25), repeated --rounds times (5): the spread of the round medians is what a difference has to exceed to mean anything.

    python tools/complexity_timing.py [--iters 25] [--rounds 5] [--out profiles/complexity_timing.txt]

Pairs per second counts the (N - m)(N - m - 1) / 2 template pairs of a row once, whatever m.  No rate is a gate: the numbers are written down
whichever way they fall."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(4096, 3000), (8, 3000)]
M_LEN, SCALES = 2, (1, 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch_rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "complexity_timing.txt"))
    ap.add_argument("--shapes", default=None, help="e.g. 4096,3000;8,3000")
    args = ap.parse_args()
    import torch
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

    def torch_counts(x, r, m, scale, rows=2):
        b, length = x.shape
        n = length // scale
        y = x[:, :n * scale].reshape(b, n, scale).sum(2) / float(scale)
        t = y.unfold(1, m + 1, 1)[:, :n - m]                       # (b, T, m + 1): the templates with their next sample
        out = torch.empty(b, 2, dtype=torch.int64, device=x.device)
        for s in range(0, b, rows):
            d = (t[s:s + rows, :, None, :] - t[s:s + rows, None, :, :]).abs()
            mb = d[..., :m].amax(-1) <= r[s:s + rows, None, None]
            ma = mb & (d[..., m] <= r[s:s + rows, None, None])
            out[s:s + rows, 0] = (mb.sum((1, 2)) - (n - m)) // 2    # finite data: the diagonal matches, the matrix is symmetric
            out[s:s + rows, 1] = (ma.sum((1, 2)) - (n - m)) // 2
        return out

    for b, length in shapes:
        g = torch.Generator(device=dev).manual_seed(b + length)
        x = torch.randn(b, length, device=dev, generator=g)
        mom = torch.empty(b, 8, dtype=torch.float64, device=dev)
        cnt = torch.empty(b, 120, dtype=torch.int32, device=dev); skp = torch.empty(b, dtype=torch.int32, device=dev)
        tm = {s: torch.empty(b, 2, dtype=torch.int64, device=dev) for s in SCALES}
        check(lib.eegldm_row_moments(ctx.h, ptr(x), length, b, length, ptr(mom)))
        r = (0.2 * torch.sqrt(mom[:, 1] / length)).float()
        bt = min(b, args.torch_rows)
        held = {}

        def moments():
            check(lib.eegldm_row_moments(ctx.h, ptr(x), length, b, length, ptr(mom)))

        def ordinal(order):
            return lambda: check(lib.eegldm_ordinal_counts(ctx.h, ptr(x), length, b, length, order, 1, ptr(cnt), ptr(skp)))

        def native(scale):
            return lambda: check(lib.eegldm_template_matches(ctx.h, ptr(x), length, b, length, M_LEN, scale, ptr(r), ptr(tm[scale])))

        def composed(scale):
            def run():
                held[scale] = torch_counts(x[:bt], r[:bt], M_LEN, scale)
            return run

        variants = {"native_row_moments": moments, "native_ordinal_counts_o3": ordinal(3), "native_ordinal_counts_o5": ordinal(5)}
        for s in SCALES:
            variants[f"native_template_matches_s{s}"] = native(s)
            variants[f"torch_unfold_chebyshev_s{s}_first_{bt}_rows"] = composed(s)
        res = measure(variants)
        torch.cuda.synchronize()
        for n, (med, lo, hi) in res.items():
            rec = dict(shape=dict(B=b, L=length), variant=n, median_ms=round(med, 4), round_medians_ms=[round(lo, 4), round(hi, 4)], iters=args.iters,
                       rounds=args.rounds)
            if "template" in n or "chebyshev" in n:
                s = int(n.split("_s")[1].split("_")[0])
                rows = bt if n.startswith("torch") else b
                t = length // s - M_LEN
                rec.update(m=M_LEN, scale=s, rows=rows, us_per_row=round(med * 1e3 / rows, 3), template_pairs_per_s=float(f"{rows * t * (t - 1) / 2 / (med * 1e-3):.4g}"))
                if n.startswith("torch"):
                    rec["counts_equal_native"] = bool(torch.equal(held[s], tm[s][:bt]))
            else:
                rec.update(us_per_row=round(med * 1e3 / b, 3), note="no counterpart")
            emit(**rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
