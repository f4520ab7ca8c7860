"""Time of eegldm_knn_update against the torch composition (torch.cdist + topk + running merge over corpus steps) on the same device, with
device events.  The composition runs twice: in steps of 1024 corpus rows (a 16 MB distance block at Nq = 4096, the nearest it comes to the
native call's ~1 MB workspace, and dominated by its ~1500 small launches per call) and in steps of 16384 rows (268 MB, the fairer
comparison); report both.  The variants alternate inside one process; every figure is the median of --iters calls (25), repeated
--rounds times (5): the spread of the round medians is what a difference has to exceed to mean anything.

    python tools/knn_timing.py [--iters 25] [--rounds 5] [--out profiles/knn_timing.txt]

Shapes (Nq, Nc, D, k): (4096, 262144, 3000, 1), the signal-space audit, and (4096, 262144, 302, 3), the feature-space radii.  The TF/s
figure counts 2 Nq Nc D FLOP per call; the f32-input MFMA of the MI355X measures 155 TF at its best.  No rate is a gate: the numbers are
written down whichever way they fall."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(4096, 262144, 3000, 1), (4096, 262144, 302, 3)]
F32_MFMA_TF = 155.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_timing.txt"))
    ap.add_argument("--shapes", default=None, help="e.g. 4096,262144,302,3;1024,65536,3000,1")
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

    for nq, nc, d, k in shapes:
        g = torch.Generator(device=dev).manual_seed(nq + nc + d + k)
        q = torch.randn(nq, d, device=dev, generator=g)
        x = torch.randn(nc, d, device=dev, generator=g)
        xb = torch.empty(nc, device=dev)
        check(lib.eegldm_rows_sqnorm(ctx.h, ptr(x), d, nc, d, ptr(xb)))
        best_s = torch.empty(nq, k, device=dev); best_i = torch.empty(nq, k, dtype=torch.int64, device=dev)
        rows = 1024
        t_s = torch.empty(nq, k, device=dev); t_i = torch.empty(nq, k, dtype=torch.int64, device=dev)

        def native():
            best_s.fill_(float("inf")); best_i.fill_(-1)
            check(lib.eegldm_knn_update(ctx.h, ptr(q), d, ptr(x), d, ptr(xb), nq, nc, d, k, 0, -1, ptr(best_s), ptr(best_i)))

        def composed(rows_per_step):
            def run():
                t_s.fill_(float("inf")); t_i.fill_(-1)
                for s in range(0, nc, rows_per_step):
                    dist = torch.cdist(q, x[s:s + rows_per_step]).square_()
                    v, i = torch.topk(dist, min(k, dist.shape[1]), dim=1, largest=False)
                    cat_v, cat_i = torch.cat([t_s, v], 1), torch.cat([t_i, i + s], 1)
                    v2, o = torch.topk(cat_v, k, dim=1, largest=False)
                    t_s.copy_(v2); t_i.copy_(torch.gather(cat_i, 1, o))
            return run

        variants = {"native_knn_update": native, f"torch_cdist_topk_{rows}_rows": composed(rows), "torch_cdist_topk_16384_rows": composed(16384)}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        agree = float((best_i == t_i).float().mean())
        rounds = {n: [] for n in variants}; every = {n: [] for n in variants}
        for _ in range(args.rounds):
            ts = {n: [] for n in variants}
            for _ in range(args.iters):
                for n, fn in variants.items():
                    ts[n].append(timed(fn))
            for n in variants:
                rounds[n].append(sorted(ts[n])[len(ts[n]) // 2]); every[n] += ts[n]
        flop = 2.0 * nq * nc * d
        for n in variants:
            med = sorted(every[n])[len(every[n]) // 2]
            emit(shape=dict(Nq=nq, Nc=nc, D=d, k=k), variant=n, median_ms=round(med, 3),
                 round_medians_ms=[round(min(rounds[n]), 3), round(max(rounds[n]), 3)], TF_per_s=round(flop / (med * 1e-3) / 1e12, 2),
                 share_of_f32_mfma_155TF=round(flop / (med * 1e-3) / 1e12 / F32_MFMA_TF, 3), iters=args.iters, rounds=args.rounds,
                 index_agreement_with_native=round(agree, 5))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
