"""Time of eegldm_kernel_matmul (R = K(A, B) V, csrc/kmm.hip) against the torch fp32 composition (a @ b.T) -> kernel function -> @ v on the same
device, with device events.  The composition runs in row blocks of A of 1024 (a 32 MB kernel block at Nb = 8192) and of 8192 rows (the
whole kernel matrix at once where Na <= 8192: the fairer comparison, and the memory the native call never needs); report both.  The
variants alternate inside one process; every figure is the median of --iters calls (25), repeated --rounds times (5): the spread of the
round medians is what a difference has to exceed to mean anything.

    python tools/kmm_timing.py [--iters 25] [--rounds 5] [--out profiles/kmm_timing.txt]

Shapes (Na, Nb, D, P): (8192, 8192, 302, 64), a permutation test on U-Sleep features, and (4096, 4096, 3000, 64), the same on raw windows;
both kernels (cubic polynomial; rbf with three bandwidths).  The TF/s figure counts 2 Na Nb (D + P) FLOP per call; the f32-input MFMA of the
MI355X measures 155 TF at its best.  No rate is a gate: the numbers are written down whichever way they fall."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(8192, 8192, 302, 64), (4096, 4096, 3000, 64)]
F32_MFMA_TF = 155.0
NO_DIAG = -(1 << 63)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmm_timing.txt"))
    ap.add_argument("--shapes", default=None, help="e.g. 8192,8192,302,64;1024,4096,3000,8")
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

    for na, nb, d, p in shapes:
        g = torch.Generator(device=dev).manual_seed(na + nb + d + p)
        a = torch.randn(na, d, device=dev, generator=g)
        b = torch.randn(nb, d, device=dev, generator=g)
        v = (torch.rand(nb, p, device=dev, generator=g) < 0.5).float()
        asq, bsq = torch.empty(na, device=dev), torch.empty(nb, device=dev)
        check(lib.eegldm_rows_sqnorm(ctx.h, ptr(a), d, na, d, ptr(asq)))
        check(lib.eegldm_rows_sqnorm(ctx.h, ptr(b), d, nb, d, ptr(bsq)))
        sig = [(0.5 * (2 * d) ** 0.5), (2 * d) ** 0.5, 2 * (2 * d) ** 0.5]
        betas = [1.0 / (2.0 * s * s) for s in sig]
        betas_c = (ctypes.c_float * 3)(*betas)
        out = torch.empty(na, p, dtype=torch.float64, device=dev)
        t_out = torch.empty(na, p, dtype=torch.float64, device=dev)
        for kernel in ("poly", "rbf"):
            def native():
                check(lib.eegldm_kernel_matmul(ctx.h, ptr(a), d, ptr(asq), ptr(b), d, ptr(bsq), ptr(v), p, na, nb, d, p, 1 if kernel == "rbf" else 0, 3,
                                               1.0 / d, 1.0, betas_c, 3, NO_DIAG, 0, ptr(out), p))

            def composed(rows):
                def run():
                    for s in range(0, na, rows):
                        dot = a[s:s + rows] @ b.T
                        if kernel == "poly":
                            k = (dot / d + 1.0) ** 3
                        else:
                            d2 = (asq[s:s + rows, None] + bsq[None, :] - 2.0 * dot).clamp_min_(0.0)
                            k = sum(torch.exp(-bt * d2) for bt in betas) / 3.0
                        t_out[s:s + rows] = (k @ v).double()
                return run

            variants = {"native_kernel_matmul": native, "torch_fp32_1024_rows": composed(1024), "torch_fp32_8192_rows": composed(8192)}
            for fn in variants.values():
                fn()
            torch.cuda.synchronize()
            rel = float(((out - t_out).abs().max() / t_out.abs().max()))
            rounds = {n: [] for n in variants}; every = {n: [] for n in variants}
            for _ in range(args.rounds):
                ts = {n: [] for n in variants}
                for _ in range(args.iters):
                    for n, fn in variants.items():
                        ts[n].append(timed(fn))
                for n in variants:
                    rounds[n].append(sorted(ts[n])[len(ts[n]) // 2]); every[n] += ts[n]
            flop = 2.0 * na * nb * (d + p)
            for n in variants:
                med = sorted(every[n])[len(every[n]) // 2]
                emit(shape=dict(Na=na, Nb=nb, D=d, P=p), kernel=kernel, variant=n, median_ms=round(med, 3),
                     round_medians_ms=[round(min(rounds[n]), 3), round(max(rounds[n]), 3)], TF_per_s=round(flop / (med * 1e-3) / 1e12, 2),
                     share_of_f32_mfma_155TF=round(flop / (med * 1e-3) / 1e12 / F32_MFMA_TF, 3), iters=args.iters, rounds=args.rounds,
                     max_rel_difference_native_vs_torch=float(f"{rel:.3e}"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
