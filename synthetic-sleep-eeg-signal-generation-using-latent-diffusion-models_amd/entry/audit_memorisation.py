"""Memorisation audit of generated windows: how near does every synthetic window come to a training window, held against the same
distance for held-out real windows?
`python -m eegldm.entry.audit_memorisation --synthetic samples/ --path_train_ids ids/ids_shhs_train.csv --path_holdout_ids ids/ids_shhs_test.csv
 --path_pre_processed ... --output audit.json`   (or --train_npy / --holdout_npy: arrays of windows (N, 3000), (N, 1, 3000) or (N, 1, 3072))

--space signal (default): 1 - Pearson correlation on the 3000 samples, the minimum over the sample offsets --lags; --space features: squared
Euclidean distance of the U-Sleep bottleneck features compute_fid uses (--usleep_weights), and precision / recall / coverage of the synthetic
set against the training set on the same features.  The search runs on the device (eegldm.metrics.NearestNeighbours), the training set is
streamed --chunk windows at a time.  audit.json holds, per synthetic window, the nearest training distance and index, the
held-out distribution's quantiles, the threshold (its --quantile) and the windows below it.  A flag records where a window sits in the
held-out distribution; the script makes no claim about what that means, nor that an unflagged set is safe to release."""
import argparse
import glob
import json
import os

import numpy as np
import torch

from ..metrics import USleep, fid_features, memorisation_audit, precision_recall_coverage
from .common import WindowLoader


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--synthetic", required=True, help="directory with the sample_*.npy / long_*.npy files of sample_trials / sample_long")
    p.add_argument("--path_train_ids", default=None); p.add_argument("--path_holdout_ids", default=None)
    p.add_argument("--path_pre_processed", default=None); p.add_argument("--type_dataset", default="shhs")
    p.add_argument("--windows_per_recording", type=int, default=1)
    p.add_argument("--train_npy", default=None, help="training windows as one array instead of an id list")
    p.add_argument("--holdout_npy", default=None, help="held-out windows as one array instead of an id list")
    p.add_argument("--space", default="signal", choices=["signal", "features"])
    p.add_argument("--k", type=int, default=1); p.add_argument("--lags", type=int, nargs="+", default=[0], help="sample offsets, e.g. --lags -5 0 5")
    p.add_argument("--quantile", type=float, default=0.01); p.add_argument("--chunk", type=int, default=65536)
    p.add_argument("--usleep_weights", default=None, help="U-Sleep state_dict (.pt) for --space features; omitted = random initialisation (smoke runs only)")
    p.add_argument("--prc_k", type=int, default=3, help="neighbour rank of the precision / recall / coverage radii")
    p.add_argument("--seed", type=int, default=42); p.add_argument("--output", default="audit.json")
    return p.parse_args(argv)


def synthetic_files(directory):
    files = sorted(glob.glob(os.path.join(directory, "sample_*.npy")) + glob.glob(os.path.join(directory, "long_*.npy")))
    if not files:
        raise FileNotFoundError(f"no sample_*.npy / long_*.npy under {directory!r}")
    return files


def load_synthetic(files, window=3000):
    """sample_*.npy: (n, 1, 3000); long_*.npy: (n, 1, T) recordings, cut into consecutive 3000-sample windows (a remainder is dropped)."""
    out = []
    for f in files:
        a = np.load(f).astype(np.float32)
        a = a.reshape(-1, a.shape[-1])
        t = (a.shape[1] // window) * window
        if t == 0:
            raise ValueError(f"{f}: {a.shape[1]} samples, shorter than a window of {window}")
        out.append(a[:, :t].reshape(-1, window))
    return np.concatenate(out, 0)


def _array_chunks(path, chunk):
    a = np.load(path, mmap_mode="r")
    a = a.reshape(a.shape[0], -1)
    for s in range(0, a.shape[0], chunk):
        yield torch.from_numpy(np.array(a[s:s + chunk], np.float32))


def _loader_chunks(args, path_ids, chunk):
    loader = WindowLoader(args.path_pre_processed, chunk, seed=args.seed, shuffle=False, path_ids=path_ids, dataset=args.type_dataset,
                          windows_per_recording=args.windows_per_recording)
    for batch in loader:
        yield batch["eeg"]


def window_chunks(args, npy, path_ids, chunk):
    if npy:
        return _array_chunks(npy, chunk)
    if not path_ids:
        raise ValueError("give the windows as an array (--train_npy / --holdout_npy) or as an id list (--path_train_ids / --path_holdout_ids)")
    return _loader_chunks(args, path_ids, chunk)


def main(args):
    files = synthetic_files(args.synthetic)
    synthetic = torch.from_numpy(load_synthetic(files))
    holdout = torch.cat(list(window_chunks(args, args.holdout_npy, args.path_holdout_ids, args.chunk)), 0)
    usleep = None
    if args.space == "features":
        torch.manual_seed(args.seed)
        usleep = USleep(in_chans=2, sfreq=100, depth=12, with_skip_connection=True, n_classes=5, input_size_s=30, apply_softmax=False)
        if args.usleep_weights:
            usleep.load_state_dict(torch.load(args.usleep_weights, map_location="cpu"))
        usleep.eval()
    res = memorisation_audit(synthetic, window_chunks(args, args.train_npy, args.path_train_ids, args.chunk), holdout, space=args.space, k=args.k,
                             lags=tuple(args.lags), quantile=args.quantile, usleep=usleep)
    if args.space == "features":
        def feats(chunks):
            return torch.cat([fid_features(usleep, (w if w.dim() == 3 else w.unsqueeze(1))[s:s + 256]).cpu() for w in chunks
                              for s in range(0, w.shape[0], 256)], 0)
        res["precision_recall_coverage"] = precision_recall_coverage(feats(window_chunks(args, args.train_npy, args.path_train_ids, args.chunk)),
                                                                     feats([synthetic]), k=args.prc_k, chunk=args.chunk)
    res["files"] = [os.path.basename(f) for f in files]
    with open(args.output, "w") as f:
        json.dump(res, f, indent=1)
    print(f"{res['n_synthetic']} synthetic windows against {res['n_train']} training windows ({res['space']}): threshold {res['threshold']:.6g} = "
          f"{res['quantile']} quantile of {res['n_holdout']} held-out windows, {len(res['flagged'])} below it -> {args.output}")
    return res


if __name__ == "__main__":
    main(parse_args())
