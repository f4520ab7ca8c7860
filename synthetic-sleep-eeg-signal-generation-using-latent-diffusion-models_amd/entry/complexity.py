"""Signal complexity of generated windows against held-out real windows: how REGULAR are the windows, overall and stage by stage?
`python -m eegldm.entry.complexity --samples 'samples/sample_*.npy' --path_test_ids ids/ids_shhs_test.csv --path_pre_processed ...
 [--holdout_npy real.npy] [--labels_from_samples] [--real_stages] [--orders 3 4 5] [--scales 1 2 5 10 20] [--m 2] [--r 0.2]
 --output complexity.json`

Per window: Hjorth activity, mobility and complexity, the rate of sign changes about the mean, line length per sample, normalised permutation
entropy at --orders and sample entropy (m, r times the window's standard deviation) at --scales, the multiscale entropy of Costa et al.  The
passes over the samples run on the device (eegldm.metrics.complexity_features), the statistics are float64 numpy.  Reported (complexity.json,
INTEGRATION.md): per feature the mean, sd and quartiles over the finite values of the real and of the synthetic set, per stage with
--labels_from_samples (sample_{i}_label.npy) / --real_stages (R.stages.npy), the real-vs-synthetic comparison per feature (KS statistic,
Wasserstein distance, counts of non-finite values), and the same comparison REAL-VS-REAL on two seeded halves of the held-out windows: the floor
to read the others against.

Nobody has measured what these features show on this project's 18-Hz-low-passed data; a matching distribution of a complexity feature is not
evidence of realism on its own."""
import argparse
import json
import os

import numpy as np

from ..metrics import _feature_stats, compare_features, complexity_features
from .micro_structure import load_real, load_samples

CAVEAT = ("Nobody has measured what these features show on this 18-Hz-low-passed data. "
          "A matching distribution of a complexity feature is not evidence of realism on its own.")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Hjorth parameters, permutation entropy and multiscale sample entropy of generated against held-out real "
                                            "windows, with the real-vs-real floor.", epilog=CAVEAT)
    p.add_argument("--samples", required=True, help="glob of generated windows, each (n, 1, 3000) float32, e.g. 'samples/sample_*.npy'")
    p.add_argument("--path_test_ids", default=None); p.add_argument("--path_pre_processed", default=None); p.add_argument("--path_stages", default=None)
    p.add_argument("--type_dataset", default="shhs"); p.add_argument("--windows_per_recording", type=int, default=1)
    p.add_argument("--holdout_npy", default=None, help="held-out real windows as one array instead of an id list")
    p.add_argument("--labels_from_samples", action="store_true", help="per-stage summaries of the synthetic set from sample_{i}_label.npy")
    p.add_argument("--real_stages", action="store_true", help="per-stage summaries of the real set from R.stages.npy (needs --path_test_ids)")
    p.add_argument("--orders", type=int, nargs="*", default=[3, 4, 5], help="orders of the permutation entropy (2..6)")
    p.add_argument("--delay", type=int, default=1, help="samples between the elements of an ordinal pattern")
    p.add_argument("--scales", type=int, nargs="+", default=[1, 2, 5, 10, 20], help="coarse-graining scales of the sample entropy (1..64)")
    p.add_argument("--m", type=int, default=2, help="template length of the sample entropy (1..4)")
    p.add_argument("--r", type=float, default=0.2, help="tolerance of the sample entropy, in standard deviations of the raw window")
    p.add_argument("--chunk", type=int, default=4096); p.add_argument("--seed", type=int, default=42)
    p.add_argument("--output", default="complexity.json")
    return p.parse_args(argv)


def _features(windows, args):
    parts, names = [], None
    for s in range(0, windows.shape[0], args.chunk):
        f, names = complexity_features(windows[s:s + args.chunk], orders=args.orders, delay=args.delay, m=args.m, r=args.r, r_mode="sd",
                                       scales=args.scales)
        parts.append(f)
    return np.concatenate(parts, 0), names


def feature_summary(features, names, labels=None):
    """Per column the mean, population sd and quartiles over its finite values and the count of non-finite ones; with labels (N,) the same per
    stage under "per_stage", keyed by the stage code."""
    f = np.asarray(features, np.float64)

    def block(pick):
        out = {"n_windows": int(pick.sum())}
        for k, name in enumerate(names):
            v = f[pick, k]
            out[name] = dict(_feature_stats(v[np.isfinite(v)]), n_nonfinite=int(np.sum(~np.isfinite(v))))
        return out

    res = block(np.ones(f.shape[0], bool))
    if labels is not None:
        lab = np.asarray(labels).reshape(-1)
        if lab.size != f.shape[0]:
            raise ValueError(f"{lab.size} labels for {f.shape[0]} windows")
        res["per_stage"] = {str(int(c)): block(lab == c) for c in np.unique(lab)}
    return res


def main(args):
    if args.chunk < 1:
        raise ValueError("--chunk must be >= 1")
    synthetic, syn_labels, files = load_samples(args)
    real, real_labels = load_real(args)
    if real.shape[0] < 4 or synthetic.shape[0] < 1:
        raise ValueError(f"at least 4 held-out and 1 synthetic windows are needed, got {real.shape[0]} and {synthetic.shape[0]}")
    f_real, names = _features(real, args)                 # (refuses bad --orders / --scales / --m / --r before anything is computed)
    f_syn, _ = _features(synthetic, args)
    if f_real.shape[1] != f_syn.shape[1]:
        raise ValueError("the two sets gave different feature lists")
    order = np.random.default_rng(args.seed).permutation(f_real.shape[0])
    half_n = f_real.shape[0] // 2
    idx_a, idx_b = np.sort(order[:half_n]), np.sort(order[half_n:])
    res = {"args": {k: v for k, v in vars(args).items()}, "features": list(names), "n_real": int(f_real.shape[0]), "n_synthetic": int(f_syn.shape[0]),
           "window_samples": {"real": int(_window_len(real)), "synthetic": int(_window_len(synthetic))},
           "real": feature_summary(f_real, names, real_labels), "synthetic": feature_summary(f_syn, names, syn_labels),
           "real_vs_synthetic": compare_features(f_real, f_syn, names),
           "real_vs_real": dict(compare_features(f_real[idx_a], f_real[idx_b], names), n=[int(len(idx_a)), int(len(idx_b))]),
           "files": [os.path.basename(f) for f in files], "caveat": CAVEAT}
    with open(args.output, "w") as f:
        json.dump(res, f, indent=1)
    worst = max(names, key=lambda n: res["real_vs_synthetic"][n]["ks"] or 0.0)
    print(f"{res['n_synthetic']} synthetic against {res['n_real']} held-out windows, {len(names)} complexity features: largest KS statistic "
          f"{res['real_vs_synthetic'][worst]['ks']} at {worst} (real-vs-real floor {res['real_vs_real'][worst]['ks']}) -> {args.output}\n{CAVEAT}")
    return res


def _window_len(windows):
    """Samples per window after the loader's zero pads are gone."""
    n = int(windows.shape[-1])
    return n - 72 if n == 3072 else n


if __name__ == "__main__":
    main(parse_args())
