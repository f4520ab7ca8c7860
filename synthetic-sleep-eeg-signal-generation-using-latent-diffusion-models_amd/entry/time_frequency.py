"""How the spectrum of generated windows moves in time, against held-out real windows, and whether their spindles ride on the slow oscillation.
`python -m eegldm.entry.time_frequency --samples 'samples/sample_*.npy' --path_test_ids ids/ids_shhs_test.csv --path_pre_processed ...
 [--holdout_npy real.npy] [--labels_from_samples] [--real_stages] [--win_s 2] [--step_s 0.5] --output time_frequency.json`
`python -m eegldm.entry.time_frequency --recording long_0.npy [--save_spectrogram] --output_dir out/`

Windows: a multitaper spectrogram per window (eegldm.metrics.spectrogram, bands only: the spectrogram itself is never written), then per window
and band the temporal mean, the coefficient of variation and the lag-1 autocorrelation of log band power (band_course_stats): two windows
with the same average PSD can be steady sigma activity or three one-second bursts, and these numbers tell them apart.  Reported
(time_frequency.json): the band-course statistics of the real and the synthetic set, overall and per stage with
--labels_from_samples / --real_stages; their per-band, per-feature KS statistic and Wasserstein distance; the same comparison REAL-VS-REAL on
two seeded halves of the held-out windows, the floor to read the others against; and the coupling block: spindles detected as
entry.micro_structure detects them, the slow-oscillation phase at each spindle's envelope peak and the amplitude-weighted preferred phase over
peak +- 0.5 s, per set the circular mean, the resultant length and the Rayleigh test, and the two sets compared.

--recording takes one long recording (entry.sample_long's long_*.npy, any length) instead: it writes the band courses of every row as
<name>_band_power.npy (rows, frames, bands) with <name>_times.npy and <name>_bands.json, and with --save_spectrogram the spectrogram as
<name>_spectrogram.npy (rows, frames, freqs) with <name>_freqs.npy.

The default bands, window lengths and the slow-oscillation band are the literature's; they have not been validated on this project's
18-Hz-low-passed data, and matching statistics are not evidence of realism on their own."""
import argparse
import json
import os

import numpy as np

from ..metrics import (BANDS, COURSE_FEATURES, _feature_stats, band_course_stats, circular_summary, compare_band_courses, compare_coupling, detect_spindles,
                       envelope_threshold, spectrogram, spindle_so_coupling)
from .micro_structure import _detect, _subset, load_real, load_samples

CAVEAT = ("The default bands, window lengths and the slow-oscillation band are the literature's; they have not been validated on this "
          "18-Hz-low-passed data. Matching statistics are not evidence of realism on their own.")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Band-power time courses and spindle / slow-oscillation coupling of generated against held-out real windows, "
                                            "with the real-vs-real floor; or the spectrogram of one long recording.", epilog=CAVEAT)
    p.add_argument("--samples", default=None, help="glob of generated windows, each (n, 1, 3000) float32, e.g. 'samples/sample_*.npy'")
    p.add_argument("--path_test_ids", default=None); p.add_argument("--path_pre_processed", default=None); p.add_argument("--path_stages", default=None)
    p.add_argument("--type_dataset", default="shhs"); p.add_argument("--windows_per_recording", type=int, default=1)
    p.add_argument("--holdout_npy", default=None, help="held-out real windows as one array instead of an id list")
    p.add_argument("--labels_from_samples", action="store_true", help="per-stage statistics of the synthetic set from sample_{i}_label.npy")
    p.add_argument("--real_stages", action="store_true", help="per-stage statistics of the real set from R.stages.npy (needs --path_test_ids)")
    p.add_argument("--recording", default=None, help="one long recording (rows, 1, T) or (rows, T) or (T,): band courses (and spectrogram) instead of the comparison")
    p.add_argument("--save_spectrogram", action="store_true", help="with --recording: also write the spectrogram")
    p.add_argument("--output_dir", default=".", help="with --recording: where the .npy files go")
    p.add_argument("--win_s", type=float, default=2.0, help="frame length (the literature's default; not validated on this data)")
    p.add_argument("--step_s", type=float, default=0.5); p.add_argument("--half_nbw", type=float, default=2.0)
    p.add_argument("--window", default="dpss", choices=("dpss", "hann")); p.add_argument("--fmax", type=float, default=None)
    p.add_argument("--thr_factor", type=float, default=1.5, help="spindle threshold = mean + thr_factor * sd of the real set's band envelope")
    p.add_argument("--so_lo", type=float, default=0.5); p.add_argument("--so_hi", type=float, default=1.25); p.add_argument("--so_trans_hz", type=float, default=0.5)
    p.add_argument("--half_s", type=float, default=0.5, help="coupling interval: envelope peak +- half_s")
    p.add_argument("--sfreq", type=float, default=100.0); p.add_argument("--chunk", type=int, default=4096)
    p.add_argument("--seed", type=int, default=42); p.add_argument("--output", default="time_frequency.json")
    return p.parse_args(argv)


def _spec_kw(args):
    return dict(sfreq=args.sfreq, win_s=args.win_s, step_s=args.step_s, window=args.window, half_nbw=args.half_nbw, fmax=args.fmax)


def course_stats(windows, args):
    """`band_course_stats` of every window, chunk by chunk: ({"mean", "cv", "lag1"} (N, NB), band names)."""
    parts, names = [], list(BANDS)
    for s in range(0, windows.shape[0], args.chunk):
        sp = spectrogram(windows[s:s + args.chunk], keep_power=False, **_spec_kw(args))
        parts.append(band_course_stats(sp["band_power"]))
        names = sp["band_names"]
    return {f: np.concatenate([p[f] for p in parts], 0) for f in COURSE_FEATURES}, names


def summarise(stats, names, labels=None):
    """Per band and feature the mean, sd and quartiles over the windows (finite values); with labels the same per stage."""
    def block(pick):
        return {name: {f: _feature_stats(stats[f][pick, j][np.isfinite(stats[f][pick, j])]) for f in COURSE_FEATURES} for j, name in enumerate(names)}
    n = stats["mean"].shape[0]
    res = {"n_windows": int(n), "bands": block(np.ones(n, bool))}
    if labels is not None:
        lab = np.asarray(labels).reshape(-1)
        if lab.size != n:
            raise ValueError(f"{lab.size} labels for {n} windows")
        res["per_stage"] = {str(int(c)): {"n_windows": int(np.sum(lab == c)), "bands": block(lab == c)} for c in np.unique(lab)}
    return res


def _rows(stats, idx):
    return {f: v[idx] for f, v in stats.items()}


def recording(args):
    a = np.load(args.recording).astype(np.float32)
    a = a.reshape(-1, a.shape[-1])
    sp = spectrogram(a, keep_power=args.save_spectrogram, **_spec_kw(args))
    os.makedirs(args.output_dir, exist_ok=True)
    stem = os.path.join(args.output_dir, os.path.splitext(os.path.basename(args.recording))[0])
    np.save(stem + "_band_power.npy", sp["band_power"].cpu().numpy())
    np.save(stem + "_times.npy", sp["times"])
    with open(stem + "_bands.json", "w") as f:
        json.dump({"band_names": sp["band_names"], "bands_hz": {k: list(BANDS[k]) for k in sp["band_names"]}, "df": sp["df"], "n_fft": sp["n_fft"],
                   "win_s": args.win_s, "step_s": args.step_s, "unit": "V^2", "caveat": CAVEAT}, f, indent=1)
    if args.save_spectrogram:
        np.save(stem + "_spectrogram.npy", sp["power"].cpu().numpy())
        np.save(stem + "_freqs.npy", sp["freqs"])
    print(f"{a.shape[0]} row(s) of {a.shape[1]} samples: {sp['n_frames']} frames x {len(sp['band_names'])} bands -> {stem}_band_power.npy\n{CAVEAT}")
    return {"stem": stem, "n_frames": int(sp["n_frames"]), "band_names": sp["band_names"]}


def main(args):
    if args.chunk < 1:
        raise ValueError("--chunk must be >= 1")
    if args.recording:
        return recording(args)
    if not args.samples:
        raise ValueError("give --samples (with held-out windows) or --recording")
    if not np.isfinite(args.thr_factor):
        raise ValueError("--thr_factor must be finite")
    synthetic, syn_labels, files = load_samples(args)
    real, real_labels = load_real(args)
    if real.shape[0] < 4 or synthetic.shape[0] < 1:
        raise ValueError(f"at least 4 held-out and 1 synthetic windows are needed, got {real.shape[0]} and {synthetic.shape[0]}")
    if real.shape[1] != synthetic.shape[1]:
        raise ValueError(f"window lengths differ: real {real.shape[1]}, synthetic {synthetic.shape[1]}")
    sf = args.sfreq
    st_real, names = course_stats(real, args)
    st_syn, _names = course_stats(synthetic, args)
    order = np.random.default_rng(args.seed).permutation(real.shape[0])
    half_n = real.shape[0] // 2
    idx_a, idx_b = np.sort(order[:half_n]), np.sort(order[half_n:])
    res = {"args": {k: v for k, v in vars(args).items()}, "n_real": int(real.shape[0]), "n_synthetic": int(synthetic.shape[0]),
           "window_s": real.shape[1] / sf, "band_names": names, "bands_hz": {k: list(BANDS[k]) for k in names}}
    res["real"] = {"band_courses": summarise(st_real, names, real_labels)}
    res["synthetic"] = {"band_courses": summarise(st_syn, names, syn_labels)}
    res["real_vs_synthetic"] = {"band_courses": compare_band_courses(st_real, st_syn, names)}
    res["real_vs_real"] = {"band_courses": compare_band_courses(_rows(st_real, idx_a), _rows(st_real, idx_b), names), "n": [int(len(idx_a)), int(len(idx_b))]}

    thr = envelope_threshold(real, factor=args.thr_factor, batch_size=args.chunk, sfreq=sf)
    kw = dict(sfreq=sf, so_band=(args.so_lo, args.so_hi), so_trans_hz=args.so_trans_hz, half_s=args.half_s)

    def coupling(w, table=None):
        table = _detect(w, args.chunk, lambda c: detect_spindles(c, thr, sfreq=sf)) if table is None else table
        parts = []
        for s in range(0, w.shape[0], args.chunk):          # chunk by chunk: an event table per chunk, window indices local
            sub = _subset(table, np.arange(s, min(s + args.chunk, w.shape[0])))
            parts.append(spindle_so_coupling(w[s:s + args.chunk], sub, **kw))
        out = {"n_events": sum(p["n_events"] for p in parts), "n_dropped": sum(p["n_dropped"] for p in parts)}
        for k in ("peak_phase", "mvl", "phase"):
            out[k] = np.concatenate([np.asarray(p[k], np.float64) for p in parts])
        out["peak_phase_stats"], out["preferred_phase_stats"] = circular_summary(out["peak_phase"]), circular_summary(out["phase"])
        return out, table

    c_real, t_real = coupling(real)
    c_syn, _t = coupling(synthetic)
    c_a, _t = coupling(real[idx_a], _subset(t_real, idx_a))
    c_b, _t = coupling(real[idx_b], _subset(t_real, idx_b))
    res["thresholds"] = {"spindle_envelope": thr}
    res["real_vs_synthetic"]["coupling"] = compare_coupling(c_real, c_syn)
    res["real_vs_real"]["coupling"] = compare_coupling(c_a, c_b)
    res["files"] = [os.path.basename(f) for f in files]
    res["caveat"] = CAVEAT
    with open(args.output, "w") as f:
        json.dump(res, f, indent=1)
    cp = res["real_vs_synthetic"]["coupling"]
    print(f"{res['n_synthetic']} synthetic against {res['n_real']} held-out windows: {len(names)} band courses; coupled spindles "
          f"{cp['synthetic']['n_events']} (real {cp['real']['n_events']}), preferred-phase distance {cp['preferred_phase_distance']} rad -> {args.output}\n{CAVEAT}")
    return res


if __name__ == "__main__":
    main(parse_args())
