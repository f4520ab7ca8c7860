"""Kernel two-sample statistics of generated windows against held-out real windows: are the two sets distinguishable at all, and is the
difference larger than real-vs-real?
`python -m eegldm.entry.two_sample --samples 'samples/sample_*.npy' --path_test_ids ids/ids_shhs_test.csv --path_pre_processed ...
 --usleep_weights best_model.pth --output two_sample.json`   (or --holdout_npy: an array of windows (N, 3000), (N, 1, 3000) or (N, 1, 3072))

--space features (default): the U-Sleep bottleneck features compute_fid uses (--usleep_weights); --space signal: the 3000 samples of a window
with their mean removed and divided by their L2 norm (eegldm_rows_standardize).  Reported (two_sample.json): KID (mean and
standard deviation of the unbiased cubic-kernel MMD^2 over --kid_subsets seeded subsets), the unbiased MMD^2 under --kernel with the p-value of
--n_perm seeded relabellings, the same three numbers for REAL-VS-REAL (the held-out windows split into two seeded halves: the floor to read
the others against), and the --witness_top synthetic windows with the most negative MMD witness value (the ones least like the real data
under the kernel).  Everything runs on the device through eegldm.metrics.kernel_matmul; no kernel matrix is ever formed.

A large p-value is not evidence that the sets are equal, and nothing here says a set is safe to release."""
import argparse
import glob
import json
import os

import numpy as np
import torch

from ..metrics import USleep, _windows2d, fid_features, kid, mmd_permutation_test, mmd_witness, median_bandwidth, rows_standardize
from .audit_memorisation import load_synthetic, window_chunks

CAVEAT = "A large p-value is not evidence that the sets are equal, and nothing here says a set is safe to release."


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="KID, MMD^2 and a permutation p-value of generated against held-out real windows, with the real-vs-real "
                                            "floor and the MMD witness ranking of the generated windows.", epilog=CAVEAT)
    p.add_argument("--samples", required=True, help="glob of generated windows, each (n, 1, 3000) float32, e.g. 'samples/sample_*.npy'")
    p.add_argument("--path_test_ids", default=None); p.add_argument("--path_pre_processed", default=None)
    p.add_argument("--type_dataset", default="shhs"); p.add_argument("--windows_per_recording", type=int, default=1)
    p.add_argument("--holdout_npy", default=None, help="held-out real windows as one array instead of an id list")
    p.add_argument("--space", default="features", choices=["features", "signal"])
    p.add_argument("--usleep_weights", default=None, help="U-Sleep state_dict for --space features; omitted = random initialisation (smoke runs only)")
    p.add_argument("--kernel", default="poly", choices=["poly", "rbf"], help="kernel of the MMD^2 test and the witness (KID is always the cubic kernel); "
                   "rbf: bandwidths (0.5, 1, 2) x the median pairwise distance")
    p.add_argument("--n_perm", type=int, default=1000); p.add_argument("--kid_subsets", type=int, default=100)
    p.add_argument("--kid_subset_size", type=int, default=1000); p.add_argument("--witness_top", type=int, default=20)
    p.add_argument("--chunk", type=int, default=65536); p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--seed", type=int, default=42); p.add_argument("--output", default="two_sample.json")
    return p.parse_args(argv)


def compare(x, y, args, sigmas):
    """The three numbers of one comparison: x plays the real side."""
    k = kid(x, y, subsets=args.kid_subsets, subset_size=args.kid_subset_size, seed=args.seed, chunk=args.chunk)
    t = mmd_permutation_test(x, y, n_perm=args.n_perm, seed=args.seed, kernel=args.kernel, sigmas=sigmas, chunk=args.chunk)
    return {"kid_mean": k["kid_mean"], "kid_std": k["kid_std"], "kid_subset_size": k["subset_size"], "mmd2": t["mmd2"], "p_value": t["p_value"],
            "n": int(x.shape[0]), "m": int(y.shape[0])}


def main(args):
    files = sorted(glob.glob(args.samples))
    if not files:
        raise FileNotFoundError(f"no generated windows match {args.samples!r}")
    if args.n_perm < 1 or args.kid_subsets < 1 or args.witness_top < 0:
        raise ValueError("n_perm and kid_subsets must be >= 1, witness_top >= 0")
    synthetic = torch.from_numpy(load_synthetic(files))
    holdout = _windows2d(torch.cat(list(window_chunks(args, args.holdout_npy, args.path_test_ids, args.chunk)), 0), "holdout")
    if holdout.shape[0] < 4 or synthetic.shape[0] < 2:
        raise ValueError(f"at least 4 held-out and 2 synthetic windows are needed, got {holdout.shape[0]} and {synthetic.shape[0]}")
    if args.space == "features":
        torch.manual_seed(args.seed)
        usleep = USleep(in_chans=2, sfreq=100, depth=12, with_skip_connection=True, n_classes=5, input_size_s=30, apply_softmax=False)
        if args.usleep_weights:
            usleep.load_state_dict(torch.load(args.usleep_weights, map_location="cpu"))
        usleep.eval()

        def rows(w):
            return torch.cat([fid_features(usleep, w[s:s + args.batch_size].unsqueeze(1)) for s in range(0, w.shape[0], args.batch_size)], 0)
    else:
        def rows(w):
            return torch.cat([rows_standardize(w[s:s + args.batch_size].cuda().float().contiguous()) for s in range(0, w.shape[0], args.batch_size)], 0)
    real, fake = rows(holdout), rows(synthetic)
    sigmas = None
    if args.kernel == "rbf":
        med = median_bandwidth(real, fake, seed=args.seed)
        sigmas = [0.5 * med, med, 2.0 * med]
    order = np.random.default_rng(args.seed).permutation(real.shape[0])
    half = real.shape[0] // 2
    idx_a, idx_b = torch.from_numpy(np.sort(order[:half])).to(real.device), torch.from_numpy(np.sort(order[half:])).to(real.device)
    res = {"space": args.space, "kernel": args.kernel, "sigmas": sigmas, "n_perm": args.n_perm, "kid_subsets": args.kid_subsets, "seed": args.seed,
           "n_real": int(real.shape[0]), "n_synthetic": int(fake.shape[0]), "dim": int(real.shape[1]),
           "real_vs_synthetic": compare(real, fake, args, sigmas),
           "real_vs_real": compare(real[idx_a], real[idx_b], args, sigmas)}
    w = mmd_witness(fake, real, fake, kernel=args.kernel, sigmas=sigmas, chunk=args.chunk)       # negative: more like its own set than like the real one
    top = np.argsort(w, kind="stable")[:args.witness_top]
    res["witness"] = {"definition": "mean_j k(p, real_j) - mean_j k(p, synthetic_j) at every synthetic window p; most negative first",
                      "index": top.tolist(), "value": w[top].tolist()}
    res["files"] = [os.path.basename(f) for f in files]
    res["caveat"] = CAVEAT
    with open(args.output, "w") as f:
        json.dump(res, f, indent=1)
    rs, rr = res["real_vs_synthetic"], res["real_vs_real"]
    print(f"{res['n_synthetic']} synthetic against {res['n_real']} held-out windows ({args.space}, {args.kernel}): KID {rs['kid_mean']:.6g} +- {rs['kid_std']:.3g}, "
          f"MMD^2 {rs['mmd2']:.6g}, p {rs['p_value']:.4g}; real-vs-real: KID {rr['kid_mean']:.6g} +- {rr['kid_std']:.3g}, MMD^2 {rr['mmd2']:.6g}, "
          f"p {rr['p_value']:.4g} -> {args.output}\n{CAVEAT}")
    return res


if __name__ == "__main__":
    main(parse_args())
