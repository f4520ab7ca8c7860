"""Time of preparing a night (csrc/resample.hip, eegldm.recordings) with device events: eegldm_resample_fir on one channel of 8 h at 125 Hz
(int16 and fp32 rows), at 256 Hz and at 100 Hz (int16), as the call chooses its geometry and for every outputs-per-thread count the kernel is
built with (EEGLDM_RS_R = 1, 2, 4, 8); eegldm_epoch_stats on the 100 Hz result.  The variants alternate round by round inside one process (a
variant's switch is set before its --iters (25) calls of a round, outside every timed region); every figure is the median of all calls over
--rounds (5) rounds: the spread of the round medians is what a difference has to exceed to mean anything.  An event pair around ONE call on
an idle device holds the launch latency; `back_to_back_ms` is 20 calls inside one event pair divided by 20, which leaves it out.

    python tools/prepare_timing.py [--iters 25] [--rounds 5] [--hours 8] [--out profiles/prepare_timing.txt]

TB/s counts the bytes the call has to move, rows in plus rows out (the taps are re-read per workgroup from cache and not counted).  The host
baseline is scipy.signal.upfirdn in float32 on the same taps, where scipy is importable: one call on one thread, and the row cut into 16
overlapping pieces on a pool of 16 threads (pieces not stitched: a timing only); medians of 3.  A baseline, never a target.
The last line is the wall time of one eegldm.recordings.prepare_recording call on an EDF file of the same night written to a temporary
directory, file read included, so that the device's share of preparing a night can be read off.  No rate is a gate."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = [(125, "int16"), (125, "fp32"), (256, "int16"), (100, "int16")]


def _pad(v, n):
    return str(v).encode("latin-1").ljust(n)


def write_edf(path, label, data, spr, duration, annotations=None):
    """A one-signal EDF (int16 `data`, spr samples per record) or, with `annotations` = [(onset, duration, text)], a one-record EDF+C file whose
    signal is the annotation list."""
    if annotations is not None:
        tal = b"+0\x14\x14\x00" + b"".join(b"+%d\x15%d\x14%s\x14\x00" % (o, d, t.encode()) for o, d, t in annotations)
        tal += b"\x00" * (len(tal) % 2)
        label, spr, duration, body, nrec, reserved = "EDF Annotations", len(tal) // 2, "0", tal, 1, "EDF+C"
    else:
        body, nrec, reserved = data.astype("<i2").tobytes(), len(data) // spr, ""
    head = (_pad("0", 8) + _pad("X", 80) + _pad("Startdate X", 80) + _pad("01.01.89", 8) + _pad("22.00.00", 8) + _pad(512, 8) + _pad(reserved, 44) + _pad(nrec, 8)
            + _pad(duration, 8) + _pad(1, 4))
    head += _pad(label, 16) + _pad("", 80) + _pad("uV", 8) + _pad(-200, 8) + _pad(200, 8) + _pad(-2048, 8) + _pad(2047, 8) + _pad("", 80) + _pad(spr, 8) + _pad("", 32)
    with open(path, "wb") as f:
        f.write(head + body)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hours", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from eegldm import recordings as rec
    from eegldm._lib import check, default_context, lib, ptr
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
            os.environ["EEGLDM_RS_R"] = str(r)
        else:
            os.environ.pop("EEGLDM_RS_R", None)
        lib.eegldm_debug_reload_env()

    def measure(variants):
        for setup, fn in variants.values():
            setup(); fn()
        torch.cuda.synchronize()
        rounds = {n: [] for n in variants}; every = {n: [] for n in variants}
        for _ in range(args.rounds):
            for n, (setup, fn) in variants.items():
                setup()
                ts = [timed(fn) for _ in range(args.iters)]
                rounds[n].append(sorted(ts)[len(ts) // 2]); every[n] += ts
        out = {}
        for n, (setup, fn) in variants.items():
            setup()
            ctx.timer_start()
            for _ in range(20):
                fn()
            out[n] = (sorted(every[n])[len(every[n]) // 2], min(rounds[n]), max(rounds[n]), ctx.timer_stop_ms() / 20.0)
        return out

    try:
        from scipy.signal import upfirdn
    except ImportError:
        upfirdn = None
    rng = np.random.default_rng(0)
    gain, offset = np.float32(400.0 / 4095 * 1e-6), np.float32(4.88e-8)
    y100 = None
    for fin, kind in CASES:
        L = int(args.hours * 3600 * fin)
        u, d, taps = rec.lowpass_resample_design(fin, 100)
        lout = -(-L * u // d)
        digital = rng.integers(-2048, 2048, L).astype(np.int16)
        x = torch.from_numpy(digital if kind == "int16" else digital.astype(np.float32) * gain + offset).to(dev).view(1, L)
        td = torch.from_numpy(taps.astype(np.float32)).to(dev)
        gd, od = torch.full((1,), float(gain), device=dev), torch.full((1,), float(offset), device=dev)
        y = torch.empty(1, lout, device=dev)

        def run():
            check(lib.eegldm_resample_fir(ctx.h, ptr(x), L, 1 if kind == "int16" else 0, ptr(gd), ptr(od), ptr(td), taps.size, u, d, ptr(y), lout, 1, L, 1))

        def native(r):
            return (lambda: set_r(r)), run
        res = measure({"resample_fir": native(0), "resample_fir_R1": native(1), "resample_fir_R2": native(2), "resample_fir_R4": native(4), "resample_fir_R8": native(8)})
        set_r(0)
        nbytes = L * (2 if kind == "int16" else 4) + lout * 4
        for n, (med, lo, hi, b2b) in res.items():
            emit(case=dict(hours=args.hours, sfreq_in=fin, input=kind, L=L, U=u, D=d, taps=int(taps.size), terms_per_output=-(-taps.size // u)), variant=n,
                 median_ms=round(med, 4), round_medians_ms=[round(lo, 4), round(hi, 4)], back_to_back_ms=round(b2b, 4), bytes_moved=nbytes,
                 TB_per_s_back_to_back=round(nbytes / (b2b * 1e-3) / 1e12, 4), GFLOP_per_s_back_to_back=round(2.0 * lout * taps.size / u / (b2b * 1e-3) / 1e9, 1),
                 iters=args.iters, rounds=args.rounds)
        if fin == 100:
            y100 = y.clone()
        if upfirdn is not None and kind == "int16":
            xf = digital.astype(np.float32) * gain + offset
            t32 = taps.astype(np.float32)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                ref = upfirdn(t32, xf, u, d)
                ts.append((time.perf_counter() - t0) * 1e3)
            c = (taps.size - 1) // 2
            run(); torch.cuda.synchronize()
            got = y[0].cpu().numpy()
            # upfirdn is the causal convolution: its output i is output m of the centred definition where i D = m D + c, so only c % D == 0 lines up;
            # the ends differ anyway (zeros there, reflection here)
            if c % d:
                note = "phases differ: not compared"
            else:
                inner = slice(taps.size, lout - taps.size)
                note = float(f"{np.abs(ref[c // d:c // d + lout][inner] - got[inner]).max() / np.abs(got).max():.3e}")
            from concurrent.futures import ThreadPoolExecutor
            pad = -(-taps.size // u)
            cuts = [L * i // 16 for i in range(17)]
            pieces = [xf[max(0, a - pad):min(L, b + pad)] for a, b in zip(cuts, cuts[1:])]
            tp = []
            with ThreadPoolExecutor(16) as pool:
                for _ in range(3):
                    t0 = time.perf_counter()
                    list(pool.map(lambda piece: upfirdn(t32, piece, u, d), pieces))
                    tp.append((time.perf_counter() - t0) * 1e3)
            emit(case=dict(hours=args.hours, sfreq_in=fin, input="fp32 host", L=L, U=u, D=d, taps=int(taps.size)), variant="scipy_upfirdn_fp32_host",
                 median_ms_one_thread=round(sorted(ts)[1], 2), median_ms_16_threads_16_pieces=round(sorted(tp)[1], 2), calls=3,
                 max_rel_difference_to_native_away_from_edges=note)

    n_ep = y100.shape[1] // 3000
    stats = torch.empty(1, n_ep, 4, device=dev)
    res = measure({"epoch_stats": ((lambda: None), lambda: check(lib.eegldm_epoch_stats(ctx.h, ptr(y100), y100.shape[1], 1, y100.shape[1], 3000, ptr(stats))))})
    med, lo, hi, b2b = res["epoch_stats"]
    emit(case=dict(L=int(y100.shape[1]), E=3000, epochs=n_ep), variant="epoch_stats", median_ms=round(med, 4), round_medians_ms=[round(lo, 4), round(hi, 4)],
         back_to_back_ms=round(b2b, 4), iters=args.iters, rounds=args.rounds)

    # one whole prepare_recording call on a written file: read, upload, resample, cut, statistics, download
    with tempfile.TemporaryDirectory() as tmp:
        n_rec = int(args.hours * 3600)
        d125 = rng.integers(-2048, 2048, n_rec * 125).astype(np.int16)
        psg = write_edf(os.path.join(tmp, "SC4001E0-PSG.edf"), "EEG Fpz-Cz", d125, 125, "1")
        n_ep = n_rec // 30
        hyp = write_edf(os.path.join(tmp, "SC4001EC-Hypnogram.edf"), None, None, 0, "0",
                        annotations=[(0, 1800, "Sleep stage W"), (1800, (n_ep - 120) * 30, "Sleep stage 2"), ((n_ep - 60) * 30, 1800, "Sleep stage W")])
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = rec.prepare_recording(psg, hyp, ["EEG Fpz-Cz"], ctx=ctx)
            ts.append((time.perf_counter() - t0) * 1e3)
        sig = out["EEG Fpz-Cz"][0]
        emit(variant="prepare_recording_wall", case=dict(hours=args.hours, sfreq_in=125, file_MB=round(os.path.getsize(psg) / 1e6, 1), samples_out=int(sig.shape[1])),
             wall_ms=[round(t, 1) for t in ts], note="host wall time of three calls in a row on a file just written (in the page cache)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
