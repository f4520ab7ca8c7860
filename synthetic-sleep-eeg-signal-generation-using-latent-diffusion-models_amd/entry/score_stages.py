"""Score windows with a trained U-Sleep stager (train_usleep.py).
`python -m eegldm.entry.score_stages --usleep_weights runs/stager/best_model.pth --samples 'samples/sample_*.npy'`
`python -m eegldm.entry.score_stages --usleep_weights runs/stager/best_model.pth --path_test_ids ids/test.csv --path_pre_processed data/`

--samples: generated windows of a class-conditional model, `sample_{i}.npy` (n, 1, 3000) float32 with the requested stage of every window in
`sample_{i}_label.npy` (n,) beside it (sample_trials.py): the report is the agreement between the stage that was asked for and the stage the
stager sees -- the check that "200 windows of N3" are N3.  --path_test_ids: real recordings with their hypnograms (R.stages.npy, as the
training script reads them): the stager's test score (the test half of train-on-synthetic, test-on-real).
Prints the report and writes it as JSON (--output, default stage_report.json beside the weights): eegldm.metrics.stage_report's fields
(confusion[true][predicted], accuracy, balanced_accuracy, per-class precision / recall / f1, kappa) plus "source" and "n".
What such a score means depends on the stager: no training recipe has been validated on sleep data here."""
import argparse
import glob
import json
import os

import numpy as np
import torch

from ..metrics import USleep, stage_report
from .common import WindowLoader


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--usleep_weights", required=True, help="state_dict written by train_usleep.py (best_model.pth / final_model.pth)")
    p.add_argument("--samples", default=None, help="glob of generated windows; sample_{i}_label.npy beside each file holds the requested stages")
    p.add_argument("--path_test_ids", default=None); p.add_argument("--path_pre_processed", default=None); p.add_argument("--path_stages", default=None)
    p.add_argument("--type_dataset", default="edfx"); p.add_argument("--windows_per_recording", type=int, default=1)
    p.add_argument("--batch_size", type=int, default=256); p.add_argument("--seed", type=int, default=42)
    p.add_argument("--depth", type=int, default=12); p.add_argument("--n_classes", type=int, default=5)
    p.add_argument("--sfreq", type=float, default=100.0); p.add_argument("--input_size_s", type=float, default=30.0)
    p.add_argument("--output", default=None)
    return p.parse_args(argv)


def main(args):
    if bool(args.samples) == bool(args.path_test_ids):
        raise ValueError("give exactly one of --samples (generated windows) and --path_test_ids (real recordings)")
    model = USleep(in_chans=2, sfreq=args.sfreq, depth=args.depth, with_skip_connection=True, n_classes=args.n_classes, input_size_s=args.input_size_s,
                   apply_softmax=False)
    model.load_state_dict(torch.load(args.usleep_weights, map_location="cpu"))
    model.eval()
    pred, true = [], []
    if args.samples:
        files = sorted(f for f in glob.glob(args.samples) if not f.endswith("_label.npy"))
        if not files:
            raise FileNotFoundError(f"no generated windows match {args.samples!r}")
        for f in files:
            lf = f[:-4] + "_label.npy"
            if not os.path.exists(lf):
                raise FileNotFoundError(f"{f} has no label file {lf}: the requested stage of each window is needed")
            x = np.load(f).astype(np.float32); y = np.load(lf).reshape(-1)
            x = x.reshape(-1, 1, x.shape[-1])
            if len(y) != len(x):
                raise ValueError(f"{lf}: {len(y)} labels for {len(x)} windows")
            p, _logits = model.predict(torch.from_numpy(x), batch_size=args.batch_size)
            pred.append(p.cpu().numpy()); true.append(y.astype(np.int64))
        source = args.samples
    else:
        loader = WindowLoader(args.path_pre_processed, args.batch_size, seed=args.seed, shuffle=False, path_ids=args.path_test_ids,
                              dataset=args.type_dataset, windows_per_recording=args.windows_per_recording, stages=True, path_stages=args.path_stages)
        for b in loader:
            p, _logits = model.predict(b["eeg"], batch_size=args.batch_size)
            pred.append(p.cpu().numpy()); true.append(b["label"].numpy())
        source = args.path_test_ids
    report = stage_report(np.concatenate(pred), np.concatenate(true), n_classes=args.n_classes)
    report["source"] = source
    print(f"{report['n']} windows from {source}: accuracy {report['accuracy']:.4f}, balanced accuracy {report['balanced_accuracy']:.4f}, "
          f"kappa {report['kappa']:.4f}")
    print("confusion (rows: requested / true stage, columns: predicted):")
    for row in report["confusion"]:
        print("  " + " ".join(f"{v:6d}" for v in row))
    out = args.output or os.path.join(os.path.dirname(os.path.abspath(args.usleep_weights)), "stage_report.json")
    with open(out, "w") as f:
        json.dump(report, f, indent=1)
    return report


if __name__ == "__main__":
    main(parse_args())
