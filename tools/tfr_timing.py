"""Time of eegldm_stft_power (csrc/tfr.hip) with device events, full spectrogram and bands only, against the torch.stft composition on the
device: K calls of torch.stft (one per taper, reflect padding, the taper centred in n_fft), |.|^2, the weighted sum, the one-sided factor,
and for the band variant the range sums.  torch.stft has no detrend, so the native calls are timed without it too (detrend costs the native
kernel one pass over the staged frame; the `native_full_detrend` line shows it).  The variants alternate inside one process; every figure is
the median of --iters calls (25), repeated --rounds times (5): the spread of the round medians is what a difference has to exceed to mean
anything.

    python tools/tfr_timing.py [--iters 25] [--rounds 5] [--out profiles/tfr_timing.txt]

Shapes (B, L, n_win, n_fft, hop, K): (4096, 3000, 200, 256, 50, 3), a chunk of 30-s windows, and (8, 2 880 000, 200, 256, 50, 3), eight nights.
No rate is a gate: the numbers are written down whichever way they fall."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(4096, 3000, 200, 256, 50, 3), (8, 2880000, 200, 256, 50, 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tfr_timing.txt"))
    ap.add_argument("--shapes", default=None, help="e.g. 4096,3000,200,256,50,3;8,2880000,200,256,50,3")
    args = ap.parse_args()
    import numpy as np
    import torch
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

    def measure(variants):
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

    for b, length, n_win, n_fft, hop, k in shapes:
        g = torch.Generator(device=dev).manual_seed(b + n_win)
        x = torch.randn(b, length, device=dev, generator=g)
        tp64, w = M.spectrogram_tapers(n_win, "dpss", n_tapers=k)
        tapers = torch.from_numpy(tp64.astype(np.float32)).to(dev)
        names, ranges = M.band_bin_ranges(M.BANDS, 100.0, n_fft)
        nb, nbin = len(ranges), n_fft // 2 + 1
        f = M.stft_num_frames(length, n_win, hop, True)
        scale = 1.0 / (100.0 * k)
        power = torch.empty(b, f, nbin, device=dev); bands = torch.empty(b, f, nb, device=dev)
        w2 = (C.c_float * k)(*([1.0] * k))
        bh = (C.c_int * (2 * nb))(*[int(v) for r in ranges for v in r])
        out = {}

        def native(want_power, want_bands, detrend):
            def run():
                check(lib.eegldm_stft_power(ctx.h, ptr(x), length, b, length, ptr(tapers), w2, k, n_win, n_fft, hop, 1, 1, detrend, 1, scale, 0, nbin,
                                            ptr(power) if want_power else None, bh, nb, ptr(bands) if want_bands else None))
            return run

        ck = torch.ones(nbin, device=dev); ck[1:n_fft // 2] = 2.0

        def torch_full():
            p = None
            for t in range(k):
                s = torch.stft(x, n_fft, hop_length=hop, win_length=n_win, window=tapers[t], center=True, pad_mode="reflect", return_complex=True)
                a = s.real * s.real + s.imag * s.imag
                p = a if p is None else p + a
            out["p"] = (p * (scale * ck)[:, None]).transpose(1, 2)[:, :f]     # (B, F, nbin); torch.stft adds a frame at t = L when hop divides L
            return out["p"]

        def torch_bands():
            p = torch_full()
            out["b"] = torch.stack([p[:, :, lo:hi].sum(-1) for lo, hi in ranges], dim=-1)

        res = measure({"native_full": native(True, False, 0), "native_bands_only": native(False, True, 0), "native_full_and_bands": native(True, True, 0),
                       "native_full_detrend": native(True, False, 1), "torch_stft_full": torch_full, "torch_stft_bands": torch_bands})
        native(True, True, 0)(); torch_bands(); torch.cuda.synchronize()
        assert out["p"].shape == power.shape, (out["p"].shape, power.shape)
        rel_p = float((power - out["p"]).abs().max() / out["p"].abs().max())
        rel_b = float((bands - out["b"]).abs().max() / out["b"].abs().max())
        frames = b * f
        for n, (med, lo, hi) in res.items():
            emit(shape=dict(B=b, L=length, n_win=n_win, n_fft=n_fft, hop=hop, K=k, frames=frames, bands=nb), variant=n, median_ms=round(med, 3),
                 round_medians_ms=[round(lo, 3), round(hi, 3)], frames_per_s=round(frames / (med * 1e-3)), iters=args.iters, rounds=args.rounds,
                 max_rel_difference_native_vs_torch=dict(power=float(f"{rel_p:.3e}"), bands=float(f"{rel_b:.3e}")))
        del power, bands, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
