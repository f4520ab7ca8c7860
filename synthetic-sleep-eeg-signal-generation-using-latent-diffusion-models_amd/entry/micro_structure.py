"""Sleep micro-structure of generated windows against held-out real windows: do the windows contain sleep spindles and slow waves, at a
plausible rate, duration, amplitude and frequency, overall and stage by stage?
`python -m eegldm.entry.micro_structure --samples 'samples/sample_*.npy' --path_test_ids ids/ids_shhs_test.csv --path_pre_processed ...
 [--holdout_npy real.npy] [--labels_from_samples] [--real_stages] [--thr_factor 1.5] [--min_amp X] --output micro_structure.json`

Spindles: band-pass 11-16 Hz, moving RMS over 0.2 s, runs above ONE absolute threshold (mean + --thr_factor * sd of the REAL set's envelope,
applied to both sets), 0.5-3 s.  Slow waves: low-pass 4 Hz, negative half-waves of 0.3-1 s paired with the positive half-wave that follows,
half-waves gated by --min_amp (default: the 0.75 quantile of the real set's negative half-wave peaks, again applied to both sets).  The filters
and the run extraction run on the device (eegldm.metrics.detect_spindles / detect_half_waves), the statistics are float64 numpy.  Reported
(micro_structure.json): the thresholds, the real and the synthetic event summaries (density per minute; mean, sd and quartiles
of duration, amplitude, frequency), per stage with --labels_from_samples (sample_{i}_label.npy) / --real_stages (R.stages.npy), the
real-vs-synthetic comparison per feature (KS statistic, Wasserstein distance), and the same comparison REAL-VS-REAL on two seeded halves of
the held-out windows: the floor to read the others against.

The detector defaults are the literature's for scalp EEG; nobody has validated them on this project's 18-Hz-low-passed data, and a matching
event density is not evidence of realism on its own."""
import argparse
import glob
import json
import os

import numpy as np
import torch

from ..metrics import (_windows2d, compare_events, detect_half_waves, detect_spindles, envelope_threshold, event_summary, pair_half_waves)
from .audit_memorisation import load_synthetic, window_chunks
from .common import WindowLoader

CAVEAT = ("The detector defaults are the literature's for scalp EEG; nobody has validated them on this 18-Hz-low-passed data. "
          "A matching event density is not evidence of realism on its own.")
WINDOW_S = 30.0


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Spindle and slow-wave statistics of generated against held-out real windows, with the real-vs-real floor.",
                                epilog=CAVEAT)
    p.add_argument("--samples", required=True, help="glob of generated windows, each (n, 1, 3000) float32, e.g. 'samples/sample_*.npy'")
    p.add_argument("--path_test_ids", default=None); p.add_argument("--path_pre_processed", default=None); p.add_argument("--path_stages", default=None)
    p.add_argument("--type_dataset", default="shhs"); p.add_argument("--windows_per_recording", type=int, default=1)
    p.add_argument("--holdout_npy", default=None, help="held-out real windows as one array instead of an id list")
    p.add_argument("--labels_from_samples", action="store_true", help="per-stage summaries of the synthetic set from sample_{i}_label.npy")
    p.add_argument("--real_stages", action="store_true", help="per-stage summaries of the real set from R.stages.npy (needs --path_test_ids)")
    p.add_argument("--thr_factor", type=float, default=1.5, help="spindle threshold = mean + thr_factor * sd of the real set's band envelope")
    p.add_argument("--min_amp", type=float, default=None, help="least half-wave peak; default: the 0.75 quantile of the real negative half-wave peaks")
    p.add_argument("--sfreq", type=float, default=100.0); p.add_argument("--chunk", type=int, default=4096)
    p.add_argument("--seed", type=int, default=42); p.add_argument("--output", default="micro_structure.json")
    return p.parse_args(argv)


def _concat(tables, offsets):
    """Event tables of consecutive chunks as one table (window indices shifted by the chunk's first window)."""
    out = {}
    for k, v in tables[0].items():
        if isinstance(v, np.ndarray):
            out[k] = np.concatenate([t[k] + (o if k == "window" else 0) for t, o in zip(tables, offsets)])
        else:
            out[k] = v
    out["n_windows"] = int(sum(t["n_windows"] for t in tables))
    if "truncated" in out:
        out["truncated"] = int(sum(t["truncated"] for t in tables))
    return out


def _detect(windows, chunk, fn):
    tables, offsets = [], []
    for s in range(0, windows.shape[0], chunk):
        tables.append(fn(windows[s:s + chunk])); offsets.append(s)
    return _concat(tables, offsets)


def _subset(table, keep_windows):
    """The events of the windows in `keep_windows` (sorted indices), renumbered 0..len - 1."""
    pos = np.full(table["n_windows"], -1, np.int64)
    pos[keep_windows] = np.arange(len(keep_windows))
    pick = pos[table["window"]] >= 0
    out = {k: (v[pick] if isinstance(v, np.ndarray) else v) for k, v in table.items()}
    out["window"] = pos[table["window"][pick]]
    out["n_windows"] = int(len(keep_windows))
    return out


def load_real(args):
    """(windows (N, L) float32 tensor, labels (N,) or None)."""
    if args.real_stages:
        if not args.path_test_ids:
            raise ValueError("--real_stages needs --path_test_ids: the stages come from R.stages.npy beside each recording")
        loader = WindowLoader(args.path_pre_processed, args.chunk, seed=args.seed, shuffle=False, path_ids=args.path_test_ids, dataset=args.type_dataset,
                              windows_per_recording=args.windows_per_recording, stages=True, path_stages=args.path_stages)
        eeg, lab = zip(*[(b["eeg"], b["label"].numpy()) for b in loader])
        return _windows2d(torch.cat(eeg, 0), "holdout"), np.concatenate(lab)
    return _windows2d(torch.cat(list(window_chunks(args, args.holdout_npy, args.path_test_ids, args.chunk)), 0), "holdout"), None


def load_samples(args):
    files = sorted(f for f in glob.glob(args.samples) if not f.endswith("_label.npy"))
    if not files:
        raise FileNotFoundError(f"no generated windows match {args.samples!r}")
    labels = None
    if args.labels_from_samples:
        labels = []
        for f in files:
            lf = f[:-4] + "_label.npy"
            if not os.path.exists(lf):
                raise FileNotFoundError(f"{f} has no label file {lf}")
            n = load_synthetic([f]).shape[0]
            y = np.load(lf).reshape(-1)
            if len(y) != n:
                raise ValueError(f"{lf}: {len(y)} labels for {n} windows")
            labels.append(y.astype(np.int64))
        labels = np.concatenate(labels)
    return torch.from_numpy(load_synthetic(files)), labels, files


def main(args):
    if not np.isfinite(args.thr_factor):
        raise ValueError("--thr_factor must be finite")
    if args.min_amp is not None and not args.min_amp >= 0:
        raise ValueError("--min_amp must be non-negative")
    if args.chunk < 1:
        raise ValueError("--chunk must be >= 1")
    synthetic, syn_labels, files = load_samples(args)
    real, real_labels = load_real(args)
    if real.shape[0] < 4 or synthetic.shape[0] < 1:
        raise ValueError(f"at least 4 held-out and 1 synthetic windows are needed, got {real.shape[0]} and {synthetic.shape[0]}")
    if real.shape[1] != synthetic.shape[1]:
        raise ValueError(f"window lengths differ: real {real.shape[1]}, synthetic {synthetic.shape[1]}")
    sf = args.sfreq
    window_s = real.shape[1] / sf
    thr = envelope_threshold(real, factor=args.thr_factor, batch_size=args.chunk, sfreq=sf)

    def spindles(w):
        return _detect(w, args.chunk, lambda c: detect_spindles(c, thr, sfreq=sf))

    def half(w, polarity, min_amp):
        return _detect(w, args.chunk, lambda c: detect_half_waves(c, polarity=polarity, sfreq=sf, min_amp=min_amp))

    min_amp = args.min_amp
    if min_amp is None:
        peaks = half(real, -1, None)["amplitude"]
        min_amp = float(np.quantile(peaks, 0.75)) if peaks.size else 0.0

    def slow_waves(w):
        return pair_half_waves(half(w, -1, min_amp), half(w, 1, min_amp))

    tables = {"real": {"spindles": spindles(real), "slow_waves": slow_waves(real)},
              "synthetic": {"spindles": spindles(synthetic), "slow_waves": slow_waves(synthetic)}}
    labels = {"real": real_labels, "synthetic": syn_labels}
    order = np.random.default_rng(args.seed).permutation(real.shape[0])
    half_n = real.shape[0] // 2
    idx_a, idx_b = np.sort(order[:half_n]), np.sort(order[half_n:])
    res = {"args": {k: v for k, v in vars(args).items()}, "thresholds": {"spindle_envelope": thr, "half_wave_min_amp": min_amp},
           "n_real": int(real.shape[0]), "n_synthetic": int(synthetic.shape[0]), "window_s": window_s}
    for side in ("real", "synthetic"):
        res[side] = {kind: event_summary(t, t["n_windows"], window_s, labels=labels[side]) for kind, t in tables[side].items()}
        res[side]["spindles"]["windows_with_more_events_than_slots"] = tables[side]["spindles"]["truncated"]
    res["real_vs_synthetic"] = {kind: compare_events(tables["real"][kind], tables["synthetic"][kind]) for kind in ("spindles", "slow_waves")}
    res["real_vs_real"] = {kind: compare_events(_subset(tables["real"][kind], idx_a), _subset(tables["real"][kind], idx_b)) for kind in ("spindles", "slow_waves")}
    res["real_vs_real"]["n"] = [int(len(idx_a)), int(len(idx_b))]
    res["files"] = [os.path.basename(f) for f in files]
    res["caveat"] = CAVEAT
    with open(args.output, "w") as f:
        json.dump(res, f, indent=1)
    rs, ss = res["real"], res["synthetic"]
    print(f"{res['n_synthetic']} synthetic against {res['n_real']} held-out windows: spindles {ss['spindles']['density_per_min']:.3g} / min "
          f"(real {rs['spindles']['density_per_min']:.3g}), slow waves {ss['slow_waves']['density_per_min']:.3g} / min "
          f"(real {rs['slow_waves']['density_per_min']:.3g}) -> {args.output}\n{CAVEAT}")
    return res


if __name__ == "__main__":
    main(parse_args())
