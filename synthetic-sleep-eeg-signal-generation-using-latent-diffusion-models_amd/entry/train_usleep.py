"""Train a U-Sleep sleep stager on the device.
`python -m eegldm.entry.train_usleep --output_dir runs/stager --path_train_ids ids/train.csv --path_valid_ids ids/valid.csv --path_pre_processed data/`
`python -m eegldm.entry.train_usleep --output_dir runs/tstr --synthetic_dir samples/ --path_valid_ids ids/valid.csv --path_pre_processed data/`

The reference has no U-Sleep training script: its FID loads `/project/params.pt`, which it does not ship, and its utility experiment (train a
stager on synthetic windows, test it on real ones, src/testing/run_sleep_decode*.py) uses another stager.  This script makes the weights that
compute_fid.py --params_path, audit_memorisation.py --usleep_weights and score_stages.py --usleep_weights take.  NO training recipe (learning
rate, epochs, class weights) has been validated on sleep data here.

Data.  Real recordings: the id CSVs of the other entry scripts; every recording R.npy needs its hypnogram R.stages.npy (WindowLoader(stages=True):
one integer code per 30-s epoch, W 0, N1 1, N2 2, N3/N4 3, REM 4, negative = unscored); a window is labelled by the epoch under its centre.
Generated windows (--synthetic_dir): the files sample_trials.py writes for a conditional model, `sample_{i}.npy` (n, 1, 3000) float32 with
`sample_{i}_label.npy` (n,) integers beside each.  One label per window (S = 1).

Files written to --output_dir: checkpoint.pth (every epoch: {"epoch", "state_dict", "optimizer": {"step", "exp_avg", "exp_avg_sq", "lr"} as flat tensors, "ema": {"shadow", "num_updates"},
"best", "history"}; the run resumes
from it when it exists), best_model.pth (plain state_dict at the best validation balanced accuracy; without validation data, the last epoch),
final_model.pth (plain state_dict; the EMA weights when --ema_decay is given), report.json ({"args", "class_weight", "history": [{"epoch",
"train_loss", "valid": stage_report}], "best_epoch", "best_balanced_accuracy"})."""
import argparse
import glob
import json
import os

import numpy as np
import torch

from ..metrics import USleep, _stager_input, balanced_class_weights, stage_report
from ..training import Adam, EMA
from .common import add_device_loader_args, cpu_state, window_loader


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--output_dir", required=True)
    p.add_argument("--path_train_ids", default=None); p.add_argument("--path_valid_ids", default=None)
    p.add_argument("--path_pre_processed", default=None); p.add_argument("--path_stages", default=None)
    p.add_argument("--type_dataset", default="edfx")
    p.add_argument("--synthetic_dir", default=None, help="train on generated windows: sample_{i}.npy + sample_{i}_label.npy")
    p.add_argument("--valid_synthetic_dir", default=None, help="validate on a folder of the same layout instead of --path_valid_ids")
    p.add_argument("--windows_per_recording", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-3); p.add_argument("--n_epochs", type=int, default=10); p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--class_weights", choices=["none", "balanced"], default="none")
    p.add_argument("--max_grad_norm", type=float, default=None); p.add_argument("--ema_decay", type=float, default=None)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--depth", type=int, default=12); p.add_argument("--n_classes", type=int, default=5)
    p.add_argument("--sfreq", type=float, default=100.0); p.add_argument("--input_size_s", type=float, default=30.0)
    add_device_loader_args(p)
    return p.parse_args(argv)


def load_labelled_windows(folder):
    """sample_{i}.npy (n, 1, T) + sample_{i}_label.npy (n,) -> (windows (N, 1, T) float32, labels (N,) int64)."""
    files = sorted(f for f in glob.glob(os.path.join(folder, "sample_*.npy")) if not f.endswith("_label.npy"))
    if not files:
        raise FileNotFoundError(f"no sample_*.npy under {folder!r}")
    xs, ys = [], []
    for f in files:
        lf = f[:-4] + "_label.npy"
        if not os.path.exists(lf):
            raise FileNotFoundError(f"{f} has no label file {lf} (sample_trials.py writes one for a conditional model)")
        x = np.load(f).astype(np.float32); y = np.load(lf).reshape(-1)
        x = x.reshape(-1, 1, x.shape[-1])
        if not np.issubdtype(y.dtype, np.integer) or len(y) != len(x):
            raise ValueError(f"{lf}: {len(y)} labels of dtype {y.dtype} for {len(x)} windows")
        xs.append(x); ys.append(y.astype(np.int64))
    return np.concatenate(xs), np.concatenate(ys)


class ArrayBatches:
    """Shuffled {"eeg", "label"} batches over in-memory windows, the loader's batch contract."""

    def __init__(self, x, y, batch_size, seed, shuffle=True):
        self.x, self.y, self.bs, self.shuffle = x, y, batch_size, shuffle
        self.rng = np.random.default_rng(seed)

    def labels(self):
        return self.y

    def __iter__(self):
        order = self.rng.permutation(len(self.x)) if self.shuffle else np.arange(len(self.x))
        for k in range(0, len(order), self.bs):
            idx = np.sort(order[k:k + self.bs])
            yield {"eeg": torch.from_numpy(self.x[idx]), "label": torch.from_numpy(self.y[idx])}


def evaluate(model, batches, n_classes):
    pred, true = [], []
    for b in batches:
        p, _logits = model.predict(b["eeg"])
        pred.append(p.cpu().numpy()); true.append(b["label"].cpu().numpy())
    return stage_report(np.concatenate(pred), np.concatenate(true), n_classes=n_classes)


def averaged_state(model, ema):
    """The model's state_dict on the host, with the EMA weights in place of the live ones when there is an EMA (the running statistics are
    the model's: the EMA averages parameters only)."""
    if ema is None:
        return cpu_state(model.state_dict())
    with ema.applied():
        return cpu_state(model.state_dict())


def main(args):
    os.makedirs(args.output_dir, exist_ok=True)
    torch.manual_seed(args.seed)
    if bool(args.synthetic_dir) == bool(args.path_train_ids):
        raise ValueError("give exactly one of --synthetic_dir (generated windows) and --path_train_ids (real recordings)")
    if args.synthetic_dir and getattr(args, "device_loader", False):
        raise ValueError("--device_loader banks recordings (--path_train_ids), not the generated windows of --synthetic_dir")
    if args.synthetic_dir:
        train = ArrayBatches(*load_labelled_windows(args.synthetic_dir), args.batch_size, args.seed)
    else:
        train = window_loader(args, args.path_pre_processed, args.batch_size, seed=args.seed, path_ids=args.path_train_ids, dataset=args.type_dataset,
                              windows_per_recording=args.windows_per_recording, stages=True, path_stages=args.path_stages)
    valid = None
    if args.valid_synthetic_dir:
        valid = ArrayBatches(*load_labelled_windows(args.valid_synthetic_dir), args.batch_size, args.seed, shuffle=False)
    elif args.path_valid_ids:
        valid = window_loader(args, args.path_pre_processed, args.batch_size, sampling="recording", seed=args.seed + 1, shuffle=False, path_ids=args.path_valid_ids,
                              dataset=args.type_dataset, windows_per_recording=args.windows_per_recording, stages=True, path_stages=args.path_stages)
    model = USleep(in_chans=2, sfreq=args.sfreq, depth=args.depth, with_skip_connection=True, n_classes=args.n_classes, input_size_s=args.input_size_s,
                   apply_softmax=False)
    model.load_state_dict(model._default_init(torch.Generator().manual_seed(args.seed)))
    ema = EMA(model, decay=args.ema_decay) if args.ema_decay is not None else None
    opt = Adam(model, lr=args.lr, ema=ema, max_grad_norm=args.max_grad_norm)
    cw = None
    if args.class_weights == "balanced":
        # generated windows: the labels are in memory; recordings: one pass over the training loader's labels (the crops are random, so this
        # is the class balance of one epoch's draw)
        labels = train.labels() if isinstance(train, ArrayBatches) else np.concatenate([b["label"].cpu().numpy() for b in train])
        cw = balanced_class_weights(labels, args.n_classes)
    history, best, start = [], {"epoch": -1, "balanced_accuracy": -1.0}, 0
    ck_path = os.path.join(args.output_dir, "checkpoint.pth")
    if os.path.exists(ck_path):
        ck = torch.load(ck_path, map_location="cpu")
        model.load_state_dict(ck["state_dict"]); opt.load_state_dict(ck["optimizer"])
        if ema is not None and ck.get("ema") is not None:
            ema.shadow.copy_(ck["ema"]["shadow"]); ema.num_updates = int(ck["ema"]["num_updates"])
        history, best, start = ck["history"], ck["best"], ck["epoch"] + 1
        print(f"resuming from {ck_path} at epoch {start}")
    loss_dev = torch.zeros(1, device=model.device)
    for epoch in range(start, args.n_epochs):
        model.train()
        total, steps = 0.0, 0
        for b in train:
            x = _stager_input(model, b["eeg"])
            if x.shape[0] < 2 and model.depth >= 12:          # one window at depth 12: no batch statistics at the bottleneck (the step refuses it)
                continue
            opt.zero_grad()
            model.train_step(x, b["label"], class_weight=cw, loss_out=loss_dev)
            opt.step()
            total += float(loss_dev); steps += 1
        rec = {"epoch": epoch, "train_loss": total / max(steps, 1), "steps": steps}
        if valid is not None:
            if ema is not None:
                with ema.applied():
                    rec["valid"] = evaluate(model, valid, args.n_classes)
            else:
                rec["valid"] = evaluate(model, valid, args.n_classes)
        history.append(rec)
        score = rec["valid"]["balanced_accuracy"] if valid is not None else float(epoch)
        if score > best["balanced_accuracy"] or valid is None:
            best = {"epoch": epoch, "balanced_accuracy": score if valid is not None else -1.0}
            torch.save(averaged_state(model, ema), os.path.join(args.output_dir, "best_model.pth"))
        torch.save({"epoch": epoch, "state_dict": cpu_state(model.state_dict()),
                    "optimizer": {"step": opt.step_count, "exp_avg": opt.m.cpu(), "exp_avg_sq": opt.v.cpu(), "lr": opt.param_groups[0]["lr"]},
                    "ema": None if ema is None else {"shadow": ema.shadow.cpu(), "num_updates": ema.num_updates},
                    "best": best, "history": history}, ck_path)
        msg = f"epoch {epoch}: train loss {rec['train_loss']:.4f} ({steps} steps)"
        if valid is not None:
            msg += f", valid balanced accuracy {rec['valid']['balanced_accuracy']:.4f}, kappa {rec['valid']['kappa']:.4f}"
        print(msg)
    torch.save(averaged_state(model, ema), os.path.join(args.output_dir, "final_model.pth"))
    report = {"args": {k: v for k, v in vars(args).items()}, "class_weight": None if cw is None else [float(v) for v in cw], "history": history,
              "best_epoch": best["epoch"], "best_balanced_accuracy": best["balanced_accuracy"]}
    with open(os.path.join(args.output_dir, "report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report


if __name__ == "__main__":
    main(parse_args())
