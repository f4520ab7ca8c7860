"""Time of making a training batch ready on the device: the host loader (entry/common.py: WindowLoader -- per-item numpy crop, np.stack,
pageable upload) against the device-resident bank (eegldm.data: one eegldm_window_batch launch per batch), and the AEKL / GAN training
loop end to end fed by each.

    python tools/loader_timing.py [--recordings 64] [--samples 2400000] [--batch 256] [--iters 25] [--rounds 5] [--out profiles/loader_timing.txt]

Recordings are written to a temporary directory (float32 .npy with hypnograms) and read once by both loaders before anything is timed: the
host loader caches normalised recordings in memory, the bank holds them in device memory.  The variants alternate round by round inside
one process; every figure is the median over --rounds rounds of --iters batches, with the lowest and highest round median beside it: a
difference has to exceed that spread to mean anything.
  batch_ready   host wall time from asking for a batch to the batch lying in device memory (torch.cuda.synchronize() inside the timed
                region), with and without stage labels.  host = WindowLoader + .to(device); device = DeviceWindowLoader.
  window_batch  eegldm_window_batch alone between device events, and 20 launches inside one event pair divided by 20 (which leaves the
                launch latency out), against the bytes it has to move: B * window * 4 read + B * (window + 2 border) * 4 written.
  aekl_loop     windows/s of the AEKL / GAN training loop of entry/train_autoencoderkl.py (AutoencoderKL [2, 2, 4] + PatchDiscriminator(64, 3
                layers), spectral loss, both Adam steps; bf16) over whole epochs of each loader, host wall time.
No figure is a gate."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--samples", type=int, default=2400000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader_timing.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from eegldm._lib import default_context
    from eegldm.data import DeviceWindowLoader, WindowBank
    from eegldm.entry.common import BORDER, WINDOW, WindowLoader, stages_path
    from eegldm.models import AutoencoderKL, PatchDiscriminator
    from eegldm.training import Adam, aekl_train_step, randn
    ctx = default_context(0)
    dev = torch.device("cuda", ctx.device)
    B, lines = args.batch, []

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    def med(v):
        return sorted(v)[len(v) // 2]

    def summary(rounds):
        """rounds: per variant, a list of per-round lists of ms -> median of everything, lowest / highest round median."""
        out = {}
        for name, rs in rounds.items():
            ms = [med(r) for r in rs]
            out[name] = dict(median_ms=round(med([t for r in rs for t in r]), 4), round_medians_ms=[round(min(ms), 4), round(max(ms), 4)])
        return out

    wpr = -(-args.iters * B // args.recordings)              # an epoch holds at least --iters batches
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        n_ep = args.samples // 3000
        for r in range(args.recordings):
            f = os.path.join(tmp, f"rec{r:03d}.npy")
            np.save(f, (rng.standard_normal(args.samples) * 1e-5).astype(np.float32))
            np.save(stages_path(f), rng.integers(-1, 5, n_ep + 1))       # one sixth of the epochs unscored: the host loader redraws there
        case = dict(recordings=args.recordings, samples=args.samples, B=B, window=WINDOW, border=BORDER, windows_per_recording=wpr,
                    iters=args.iters, rounds=args.rounds)

        def host_batches(loader, labelled):
            def gen():
                while True:
                    for b in loader:
                        x = b["eeg"].to(dev)
                        y = b["label"].to(dev) if labelled else None
                        yield x, y
            return gen()

        def device_batches(loader, labelled):
            def gen():
                while True:
                    for b in loader:
                        yield b["eeg"], (b["label"] if labelled else None)
            return gen()

        for labelled in (False, True):
            t0 = time.perf_counter()
            host = WindowLoader(tmp, B, seed=1, windows_per_recording=wpr, stages=labelled)
            for r in range(args.recordings):                  # read and normalise every recording before the clock starts
                host._recording(r)
            t_host = time.perf_counter() - t0
            t0 = time.perf_counter()
            bank = WindowBank(host.files, host.stage_files)
            torch.cuda.synchronize()
            t_bank = time.perf_counter() - t0
            emit(what="setup", labelled=labelled, case=case, host_read_and_normalise_s=round(t_host, 2), bank_read_upload_normalise_s=round(t_bank, 2),
                 bank_MB=round(bank.total * 4 / 1e6, 1), segments=[bank.table_a.n_seg, bank.table_b.n_seg])
            modes = ["recording", "uniform"] + (["balanced"] if labelled else [])
            gens = {"host": host_batches(host, labelled)}
            for m in modes:
                gens["device_" + m] = device_batches(DeviceWindowLoader(bank, B, seed=1, sampling=m, windows_per_recording=wpr), labelled)
            for g in gens.values():                           # warm-up: allocator, first launches
                for _ in range(3):
                    next(g)
            torch.cuda.synchronize()
            rounds = {n: [] for n in gens}
            for _ in range(args.rounds):
                for n, g in gens.items():
                    ts = []
                    for _i in range(args.iters):
                        t0 = time.perf_counter()
                        x, _y = next(g)
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    assert x.shape == (B, 1, WINDOW + 2 * BORDER) and x.is_cuda
                    rounds[n].append(ts)
            for n, s in summary(rounds).items():
                emit(what="batch_ready", labelled=labelled, variant=n, **s, windows_per_s=round(B / (s["median_ms"] * 1e-3)))

            if labelled:
                continue
            # the kernel alone
            out = torch.empty(B, 1, WINDOW + 2 * BORDER, device=dev)
            count = [0]

            def launch():
                bank.batch(B, seed=3, offset=count[0] * B, out=out); count[0] += 1

            launch(); torch.cuda.synchronize()
            rs = []
            for _ in range(args.rounds):
                ts = []
                for _i in range(args.iters):
                    ctx.timer_start(); launch(); ts.append(ctx.timer_stop_ms())
                rs.append(ts)
            ctx.timer_start()
            for _ in range(20):
                launch()
            b2b = ctx.timer_stop_ms() / 20.0
            nbytes = B * WINDOW * 4 + B * (WINDOW + 2 * BORDER) * 4
            emit(what="window_batch", variant="eegldm_window_batch", **summary({"k": rs})["k"], back_to_back_ms=round(b2b, 4), bytes_moved=nbytes,
                 TB_per_s_back_to_back=round(nbytes / (b2b * 1e-3) / 1e12, 4),
                 note="labels_out written too (8 B per window); the figure includes the Python call and one torch.empty for the labels")

            # the AEKL / GAN loop of entry/train_autoencoderkl.py, whole epochs
            ae = AutoencoderKL(spatial_dims=1, in_channels=1, out_channels=1, num_channels=[2, 2, 4], latent_channels=1, num_res_blocks=2,
                               norm_num_groups=1, attention_levels=[False, False, False], dtype="bfloat16", device=ctx.device)
            disc = PatchDiscriminator(spatial_dims=1, num_layers_d=3, num_channels=64, in_channels=1, out_channels=1, kernel_size=3,
                                      norm="BATCH", bias=False, padding=1, dtype="bfloat16", device=ctx.device)
            og, od = Adam(ae, lr=5e-3), Adam(disc, lr=5e-4)
            losses = torch.zeros(6, device=dev)
            steps = [0]

            def epoch(loader):
                seen = 0
                for b in loader:
                    x = b["eeg"].to(dev)
                    Ll = x.shape[2] // ae.down
                    eps = randn(ctx, (x.shape[0], ae.latent_channels, Ll), seed=5, offset=steps[0] * x.shape[0] * Ll * ae.latent_channels)
                    og.zero_grad(); od.zero_grad()
                    aekl_train_step(ae, disc, x, eps, 0.01, 1e-9, 1e4, True, losses_out=losses)
                    og.step(); od.step()
                    steps[0] += 1; seen += x.shape[0]
                torch.cuda.synchronize()
                return seen

            loaders = {"host": host, "device_recording": DeviceWindowLoader(bank, B, seed=1, windows_per_recording=wpr)}
            for ld in loaders.values():
                epoch(ld)
            rates = {n: [] for n in loaders}
            for _ in range(args.rounds):
                for n, ld in loaders.items():
                    t0 = time.perf_counter()
                    seen = epoch(ld)
                    rates[n].append(seen / (time.perf_counter() - t0))
            for n, v in rates.items():
                emit(what="aekl_loop", variant=n, windows_per_s=round(med(v)), round_windows_per_s=[round(min(v)), round(max(v))],
                     windows_per_epoch=args.recordings * wpr, epochs=args.rounds, final_losses=[round(float(t), 5) for t in losses.cpu()])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
