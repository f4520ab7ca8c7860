"""Shared plumbing of the entry scripts: yaml config (PyYAML; attribute access like OmegaConf),
the reference's `--num_channels "[32,32,64]"` list argument (src/util.py:23-26), run-dir / resume convention
(src/util.py:29-43) and a numpy window loader honouring the loader's output contract
(src/dataset/dataset.py:10-30: dict batch, key 'eeg', float32 (B,1,3072), zero-padded 36 samples each side)."""
import argparse
import ast
import glob
import os

import numpy as np
import torch
import yaml


class Cfg(dict):
    """dict with attribute access, recursively (OmegaConf-like, read side only)."""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError as e:
            raise AttributeError(k) from e
        return Cfg(v) if isinstance(v, dict) else v


def load_config(path):
    with open(path) as f:
        return Cfg(yaml.safe_load(f))


class ParseListAction(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, ast.literal_eval(values))


def setup_run_dir(config, args, base_path=None):
    """{output_dir}/{run_dir}_{spe}_{dataset}; resume iff checkpoint.pth exists (util.py:29-43)."""
    name = f"{config.train.run_dir}_{getattr(args, 'spe', 'no-spectral')}_{getattr(args, 'dataset', getattr(args, 'type_dataset', 'edfx'))}"
    run_dir = os.path.join(getattr(args, "output_dir", None) or config.train.output_dir, name)
    os.makedirs(run_dir, exist_ok=True)
    return run_dir, os.path.exists(os.path.join(run_dir, "checkpoint.pth"))


def synthetic_windows(n, seed, length=3072, pad=36):
    """SURVEY 8d synthetic 30-s windows: sinusoid mix + noise in [0,1], exact zeros in the pads."""
    r = np.random.default_rng(seed)
    t = np.arange(length - 2 * pad, dtype=np.float64)
    x = np.zeros((n, 1, length), np.float32)
    for b in range(n):
        sig = sum(r.uniform(0.2, 1.0) * np.sin(2 * np.pi * f * t / 100.0 + r.uniform(0, 2 * np.pi)) for f in (1.5, 6.0, 10.0, 13.0))
        x[b, 0, pad:length - pad] = np.clip(0.5 + 0.1 * sig + 0.05 * r.standard_normal(t.shape), 0, 1)
    return x


WINDOW = 3000      # 30 s at 100 Hz (dataset.py:7-8)
BORDER = 36        # BorderPadD(spatial_border=[36]) (dataset.py:18)
EPOCH = 3000       # one scored sleep epoch: 30 s at 100 Hz
STAGES_SUFFIX = ".stages.npy"     # R.npy's hypnogram: R.stages.npy (never taken for a recording)


def stages_path(recording, path_stages=None):
    """Where the stage codes of `recording` (R.npy) live: R.stages.npy beside it, or under `path_stages` with the same stem."""
    stem = os.path.basename(recording)[:-4] if recording.endswith(".npy") else os.path.basename(recording)
    return os.path.join(path_stages or os.path.dirname(recording), stem + STAGES_SUFFIX)


def centre_label(stages, start):
    """Stage code of the window cropped at `start`: the code of the 30-s epoch holding its centre sample start + 1500 (the centre rule of
    get_center_label, run_sleep_decode.py:44-47); -1 (unscored) past the end of the hypnogram."""
    e = (start + WINDOW // 2) // EPOCH
    return int(stages[e]) if e < len(stages) else -1


def normalise_recording(a):
    """The deterministic head of get_trans (dataset.py:12-16): ScaleIntensityD(factor=1e6) = x * (1 + 1e6), then
    ScaleIntensityD(minv=0, maxv=1) = min-max over the WHOLE recording (a constant recording maps to zeros, as
    monai.transforms.utils.rescale_array does).  float32 in, float32 out, flattened to one channel."""
    a = np.asarray(a, dtype=np.float32).reshape(-1) * np.float32(1.0 + 1e6)
    lo, hi = a.min(), a.max()
    if hi == lo:
        return np.zeros_like(a)
    return (a - lo) / (hi - lo)


def crop_and_pad(rec, start):
    """RandSpatialCropD(roi_size=[3000], random_size=False) at offset `start`, then 36 zeros on each side -> (1, 3072)."""
    w = np.zeros((1, WINDOW + 2 * BORDER), np.float32)
    w[0, BORDER:BORDER + WINDOW] = rec[start:start + WINDOW]
    return w


def read_ids(path_ids, path_pre_processed, dataset="edfx"):
    """File list from an id CSV (column FILE_NAME_EEG), as get_datalist builds it (dataset.py:33-60): '.npy' suffix for edfx."""
    import csv
    with open(path_ids, newline="") as f:
        rows = list(csv.DictReader(f))
    if rows and "FILE_NAME_EEG" not in rows[0]:
        raise ValueError(f"{path_ids}: no FILE_NAME_EEG column (dataset.py:49)")
    final = ".npy" if dataset == "edfx" else ""
    return [os.path.join(path_pre_processed or "", r["FILE_NAME_EEG"] + final) for r in rows]


def shard_files(files, rank, world):
    """Rank `rank`'s slice of the file list, the SAME length on every rank: ceil(N / world) entries, taken round-robin and wrapped
    around the end of the list (what torch's DistributedSampler does with drop_last=False).  Equal lengths matter: every rank runs
    one gradient all-reduce per batch, so a rank with one more batch than the others would wait in a collective nobody else enters."""
    if world <= 1 or not files:
        return list(files)
    per = -(-len(files) // world)
    return [files[(rank + i * world) % len(files)] for i in range(per)]


class WindowLoader:
    """Iterable of {'eeg': float32 (B,1,3072)} batches -- the loader output contract of dataset.py:10-30,62-69.

    Source: the recordings named by an id CSV (`path_ids`, column FILE_NAME_EEG: the reference's train / valid / test split), or
    every *.npy under `path_pre_processed` when no CSV is given, or synthetic windows (`n_synthetic`).  Each item = normalise the
    whole recording (x * (1 + 1e6), min-max), random 3000-sample crop, 36-sample zero pad.  The reference re-reads and re-normalises
    a whole night (~23 MB) for every 12 KB window (PersistentDataset(cache_dir=None)); here a recording is read and normalised ONCE
    and kept in memory, and `windows_per_recording` crops are drawn from it per epoch (1 = the reference's epoch definition).
    `shard=(rank, world)` gives every data-parallel rank its own slice of the file list (an epoch is the data once, not world
    times; `shard_files`: equal length on every rank, so all ranks run the same number of steps per epoch).  A run that names real
    data (`path_ids` / `path_pre_processed`) and finds none raises instead of silently training on synthetic windows.  Crop offsets come from a numpy Generator seeded per loader (`crop_starts` can be injected for parity tests).

    `stages=True` (or a `path_stages` directory): class labels for conditional training.  Every recording R.npy has a hypnogram R.stages.npy
    beside it (or under `path_stages`): a 1-D integer array, one code per 30-s epoch from sample 0 of the stored recording, W 0, N1 1, N2 2,
    N3/N4 3, REM 4 (run_sleep_decode.py:112-118), negative = unscored.  A window's label is the code of the epoch holding its centre sample;
    a crop whose centre is unscored is drawn again (from the loader's Generator, also after an injected `crop_starts` value).  Batches then
    carry 'label', int64 (B,)."""

    def __init__(self, path_pre_processed, batch_size, n_synthetic=0, seed=0, drop_last=False, shuffle=True, path_ids=None,
                 dataset="edfx", shard=(0, 1), windows_per_recording=1, crop_starts=None, stages=False, path_stages=None):
        self.batch_size, self.drop_last, self.shuffle = batch_size, drop_last, shuffle
        self.rng = np.random.default_rng(seed)
        self.wpr = max(1, int(windows_per_recording))
        self.crop_starts = crop_starts
        self.recordings, self.windows, self.files = None, None, []
        if n_synthetic:
            files = []
        elif path_ids:
            files = read_ids(path_ids, path_pre_processed, dataset)
            missing = [f for f in files if not os.path.exists(f)]
            if missing:
                raise FileNotFoundError(f"{len(missing)} recordings listed in {path_ids} are missing, e.g. {missing[0]}")
        else:
            files = sorted(glob.glob(os.path.join(path_pre_processed or "", "**", "*.npy"), recursive=True)) if path_pre_processed else []
            files = [f for f in files if not f.endswith(STAGES_SUFFIX)]
        rank, world = shard
        if (path_ids or path_pre_processed) and not n_synthetic and not files:
            raise FileNotFoundError(f"no recordings found (path_ids={path_ids!r}, path_pre_processed={path_pre_processed!r}); "
                                    "refusing to fall back to synthetic windows for a run that named real data")
        files = shard_files(files, rank, world)
        self.stage_files = None
        if stages or path_stages:
            if not files:
                raise ValueError("stage labels need recordings (path_ids / path_pre_processed), not synthetic windows")
            self.stage_files = [stages_path(f, path_stages) for f in files]
            missing = [f for f in self.stage_files if not os.path.exists(f)]
            if missing:
                raise FileNotFoundError(f"{len(missing)} stage files are missing, e.g. {missing[0]}")
            self.stage_codes = [None] * len(files)
        if files:
            self.files = files
            self.recordings = [None] * len(files)          # read + normalised on first use, then cached
            self.n = len(files) * self.wpr
        else:
            self.windows = synthetic_windows(n_synthetic or 4 * batch_size, seed)
            self.n = len(self.windows)

    def __len__(self):
        return self.n // self.batch_size if self.drop_last else -(-self.n // self.batch_size)

    def _recording(self, r):
        if self.recordings[r] is None:
            rec = normalise_recording(np.load(self.files[r]))
            if rec.shape[0] < WINDOW:
                raise ValueError(f"{self.files[r]}: {rec.shape[0]} samples, need at least {WINDOW}")
            self.recordings[r] = rec
        return self.recordings[r]

    def _stages(self, r):
        if self.stage_codes[r] is None:
            st = np.load(self.stage_files[r])
            if st.ndim != 1 or not np.issubdtype(st.dtype, np.integer):
                raise ValueError(f"{self.stage_files[r]}: stage codes must be a 1-D integer array, got {st.dtype} {st.shape}")
            self.stage_codes[r] = st.astype(np.int64)
        return self.stage_codes[r]

    def _item(self, i):
        if self.windows is not None:
            return self.windows[i]
        rec = self._recording(i // self.wpr)
        draw = lambda: int(self.rng.integers(0, rec.shape[0] - WINDOW + 1))       # RandSpatialCrop: every valid start, last one included
        s = int(self.crop_starts[i]) if self.crop_starts is not None else draw()
        if self.stage_files is None:
            return crop_and_pad(rec, s)
        st = self._stages(i // self.wpr)
        for _ in range(10000):
            lab = centre_label(st, s)
            if lab >= 0:
                return crop_and_pad(rec, s), lab
            s = draw()
        raise ValueError(f"{self.files[i // self.wpr]}: no scored epoch under the centre of 10000 crops")

    def __iter__(self):
        order = self.rng.permutation(self.n) if self.shuffle else np.arange(self.n)
        for k in range(len(self)):
            idx = order[k * self.batch_size:(k + 1) * self.batch_size]
            items = [self._item(int(i)) for i in idx]
            if self.stage_files is None:
                yield {"eeg": torch.from_numpy(np.stack(items))}
            else:
                yield {"eeg": torch.from_numpy(np.stack([w for w, _ in items])), "label": torch.tensor([c for _, c in items], dtype=torch.int64)}


def add_device_loader_args(p):
    p.add_argument("--device_loader", action="store_true", help="keep the recordings in device memory (eegldm.data.WindowBank) and crop, pad and "
                   "label every batch there in one launch, instead of the per-item numpy loop and an upload per batch.  Same distribution of "
                   "windows as the host loader, another random stream (device Philox instead of numpy)")
    p.add_argument("--sampling", default="recording", choices=["recording", "uniform", "balanced"], help="with --device_loader, how training "
                   "windows are drawn: each recording once per epoch (the host loader's epoch), uniformly over every valid start of the bank, or "
                   "class first, then uniformly within the class (needs stages).  Validation always visits recordings")


def window_loader(args, path_pre_processed, batch_size, n_synthetic=0, sampling=None, **kw):
    """The loader of an entry script: WindowLoader(path_pre_processed, batch_size, n_synthetic, **kw), or with --device_loader a
    DeviceWindowLoader over a bank of exactly the files (and stage files) that loader resolved -- id CSV, directory scan and shard included.
    sampling: None = the command line's --sampling (training), or a fixed mode (validation passes "recording")."""
    host = WindowLoader(path_pre_processed, batch_size, n_synthetic, **kw)
    mode = sampling or getattr(args, "sampling", "recording")
    if not getattr(args, "device_loader", False):
        if getattr(args, "sampling", "recording") != "recording":
            raise ValueError("--sampling needs --device_loader")
        return host
    if not host.files:
        raise ValueError("--device_loader banks recordings (--path_train_ids / --path_pre_processed), not synthetic windows")
    if kw.get("crop_starts") is not None:
        raise ValueError("injected crop_starts belong to the host loader")
    from ..data import DeviceWindowLoader, WindowBank
    bank = WindowBank(host.files, host.stage_files)
    return DeviceWindowLoader(bank, batch_size, kw.get("seed", 0), sampling=mode, windows_per_recording=kw.get("windows_per_recording", 1),
                              drop_last=kw.get("drop_last", False), shuffle=kw.get("shuffle", True))


def add_ema_args(p):
    p.add_argument("--ema_decay", type=float, default=None, help="keep an exponential moving average of the UNet weights with this decay "
                   "(updated inside the Adam kernel); adds the 'ema' entry to checkpoint.pth and writes best_model_ema.pth / final_model_ema.pth")
    p.add_argument("--ema_no_warmup", action="store_true", help="constant decay instead of min(decay, (1 + n) / (10 + n))")


def add_loss_weighting_args(p):
    p.add_argument("--loss_weighting", default=None, choices=["none", "min_snr"], help="weight every sample's loss by its noise level "
                   "(schedulers.loss_weights; min_snr = Min-SNR-gamma, Hang et al. 2023) through the weighted native loss; adds the "
                   "'loss_weighting' entry to checkpoint.pth.  Without the flag the step is the plain MSE, as before")
    p.add_argument("--snr_gamma", type=float, default=5.0, help="the clamp of --loss_weighting min_snr")
    p.add_argument("--loss_by_noise_level", type=int, default=0, metavar="K", help="print the loss in K equal timestep ranges (training: the epoch's "
                   "steps; validation: against the prediction type's own target) and append them to {run_dir}/loss_by_noise_level.json")


def step_weighting(args):
    """Keywords of the train step for the parsed flags: {} without them (the plain exports), else loss_weighting / snr_gamma
    (--loss_by_noise_level alone: "none", the weighted loss with every weight 1 -- it is the one that returns per-sample losses)."""
    if args.loss_weighting is None and not args.loss_by_noise_level:
        return {}
    return dict(loss_weighting=args.loss_weighting or "none", snr_gamma=args.snr_gamma)


def loss_weighting_resume(args, ck):
    """checkpoint.pth against the command line: without --loss_weighting the checkpoint's setting is restored into `args`; a different
    one is refused (the two halves of the run would optimise different objectives)."""
    saved = ck.get("loss_weighting")
    if args.loss_weighting is None:
        if saved is not None:
            args.loss_weighting, args.snr_gamma = saved["weighting"], float(saved["snr_gamma"])
        return
    mine = {"weighting": args.loss_weighting, "snr_gamma": float(args.snr_gamma)}
    if saved is None or saved["weighting"] != mine["weighting"] or float(saved["snr_gamma"]) != mine["snr_gamma"]:
        raise ValueError(f"checkpoint.pth was trained with loss_weighting {saved}, the command line asks for {mine}: start a new run directory "
                         "or resume with the checkpoint's setting")


def add_context_args(p):
    p.add_argument("--context", action="store_true", help="train a context-conditioned UNet (learned repair / continuation): "
                   "UNetModel(in_channels=2 C + 1, context_channels=C + 1) sees the kept signal and the keep-mask as extra input channels, "
                   "with masks drawn at random on the device; adds the 'context' entry to checkpoint.pth")
    p.add_argument("--ctx_p_none", type=float, default=None, help="share of samples trained without any context (default 0.1)")
    p.add_argument("--ctx_p_prefix", type=float, default=None, help="share of samples trained as a continuation: keep a prefix (default 0.3)")
    p.add_argument("--ctx_span_min", type=int, default=None, help="shortest regenerated span, in positions of the sampler's resolution "
                   "(default L / 32: a convention, not measured on sleep data)")
    p.add_argument("--ctx_span_max", type=int, default=None, help="longest regenerated span (default L / 2: a convention, not measured on sleep data)")


_CONTEXT_FLAGS = (("p_none", "ctx_p_none"), ("p_prefix", "ctx_p_prefix"), ("span_min", "ctx_span_min"), ("span_max", "ctx_span_max"))


def context_entry(args, channels, L=None):
    """The 'context' entry of checkpoint.pth for the parsed flags -- {context_channels, p_none, p_prefix, span_min, span_max} with the
    defaults filled in for sequences of L positions and checked (ValueError) -- or None without --context.  L None (before the data is
    known): only what the flags themselves can get wrong is checked, and the spans of the result are placeholders."""
    from ..training import context_draw_args
    given = [flag for _k, flag in _CONTEXT_FLAGS if getattr(args, flag, None) is not None]
    if not getattr(args, "context", False):
        if given:
            raise ValueError(f"--{given[0]} needs --context")
        return None
    spec = {k: getattr(args, flag) for k, flag in _CONTEXT_FLAGS if getattr(args, flag, None) is not None}
    if L is None:
        spec.setdefault("span_min", 1); spec.setdefault("span_max", max(1, spec["span_min"]))
        L = max(1, spec["span_max"])
    p_none, p_prefix, span_min, span_max = context_draw_args(spec, L)
    return {"context_channels": int(channels) + 1, "p_none": p_none, "p_prefix": p_prefix, "span_min": span_min, "span_max": span_max}


def context_resume(args, ck):
    """checkpoint.pth against the command line, before the model is built: a checkpoint trained with --context restores the flag and every
    draw parameter that was not given; a contradicting flag -- another value, or --context against a checkpoint without the entry -- is
    refused (the first conv would not even have the checkpoint's shape)."""
    saved = ck.get("context")
    if saved is None:
        if getattr(args, "context", False):
            raise ValueError("checkpoint.pth was trained without --context: start a new run directory")
        return
    args.context = True
    for k, flag in _CONTEXT_FLAGS:
        mine = getattr(args, flag, None)
        if mine is None:
            setattr(args, flag, saved[k])
        elif type(saved[k])(mine) != saved[k]:
            raise ValueError(f"checkpoint.pth was trained with context {k} = {saved[k]}, the command line asks for {mine}: start a new run "
                             "directory or resume with the checkpoint's setting")


def context_of_checkpoint(ck, out_channels=None):
    """How the scripts recognise a context model -> context_channels, or 0.  ck: what torch.load gave -- a checkpoint.pth (its 'context'
    entry) or a bare state dict (input_blocks.0.0.weight has 2 * out + 1 input channels, out from out.2.weight unless given)."""
    if isinstance(ck.get("context"), dict):
        return int(ck["context"]["context_channels"])
    sd = ck.get("diffusion", ck)
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    w = sd.get("input_blocks.0.0.weight")
    if w is None or "out.2.weight" not in sd:
        return 0
    out = int(sd["out.2.weight"].shape[0]) if out_channels is None else int(out_channels)
    return out + 1 if int(w.shape[1]) == 2 * out + 1 else 0


def context_model_kwargs(up, weights, diffusion_path=None):
    """For the sampling scripts: recognise a context model -- by the 'context' entry of {diffusion_path}/checkpoint.pth when there is one,
    else by the first conv of the state dict `weights` -- and widen the UNet parameters `up` (in place) to in_channels = 2 C + 1.
    -> the extra UNetModel keywords ({} for a plain model)."""
    cc = 0
    ck_path = os.path.join(diffusion_path, "checkpoint.pth") if diffusion_path else None
    if ck_path and os.path.exists(ck_path):
        cc = context_of_checkpoint(torch.load(ck_path, map_location="cpu"), up["out_channels"])
    else:
        cc = context_of_checkpoint(weights, up["out_channels"])
    if not cc:
        return {}
    up["in_channels"] = int(up["out_channels"]) + cc
    return {"context_channels": cc}


def _positive_float(text):
    x = float(text)
    if not x > 0.0:
        raise argparse.ArgumentTypeError(f"must be > 0 (inf = measure only), got {text}")
    return x


def _positive_int(text):
    k = int(text)
    if k < 1:
        raise argparse.ArgumentTypeError(f"must be >= 1, got {text}")
    return k


def add_grad_clip_args(p, accum=True):
    p.add_argument("--max_grad_norm", type=_positive_float, default=None, help="clip the global L2 norm of the gradient to this value before every "
                   "optimizer step (on the device, inside the Adam launch; after the all-reduce in data-parallel runs); adds the grad-norm "
                   "figures to the epoch line and the 'grad_clip' entry to checkpoint.pth")
    if accum:
        p.add_argument("--grad_accum_steps", type=_positive_int, default=None, metavar="K", help="one optimizer step (and one all-reduce) per K "
                       "micro-batches, each counted 1 / K (default 1); --max_steps keeps counting micro-batches")


def accum_plan(i, n_batches, K, steps_left=None):
    """Micro-batch i (0-based) of an epoch of n_batches, groups of K, at most steps_left further micro-batches allowed (None: no limit)
    -> (zero, last, k): zero the gradient before it, all-reduce and step after it, and it is the group's k-th micro-batch.  Groups start
    at the epoch's first batch; the one cut short by the epoch's end or by the step limit is stepped with its k < K micro-batches, the
    gradient scaled by K / k (accum_factor) so that the update is the mean over what was seen."""
    K = int(K)
    end = n_batches if steps_left is None else min(n_batches, int(steps_left))
    j = i % K
    return j == 0, (j == K - 1 or i == end - 1), j + 1


def accum_factor(K, k):
    return float(K) / float(k)


def accum_schedule(n_batches, K, steps_left=None):
    """The whole epoch as a list of {"zero", "sync", "step", "factor"} (factor: the multiplier of grad_inv_scale at a step, else None)."""
    end = n_batches if steps_left is None else min(n_batches, int(steps_left))
    out = []
    for i in range(end):
        zero, last, k = accum_plan(i, n_batches, K, steps_left)
        out.append({"zero": zero, "sync": last, "step": last, "factor": accum_factor(K, k) if last else None})
    return out


def grad_clip_entry(args):
    """The 'grad_clip' entry of checkpoint.pth, or None when neither flag was given (nor restored)."""
    mg, ga = getattr(args, "max_grad_norm", None), getattr(args, "grad_accum_steps", None)
    if mg is None and ga is None:
        return None
    return {"max_grad_norm": None if mg is None else float(mg), "grad_accum_steps": int(ga or 1)}


def grad_clip_resume(args, ck, rank=0):
    """checkpoint.pth against the command line: a flag that was not given takes the checkpoint's value; one that was given wins, and a
    difference is reported in one line."""
    saved = ck.get("grad_clip")
    if saved is None:
        return
    changed = []
    for name in ("max_grad_norm", "grad_accum_steps"):
        if not hasattr(args, name):
            continue
        mine, theirs = getattr(args, name), saved.get(name)
        if mine is None:
            setattr(args, name, theirs)
        elif theirs is not None and mine != theirs:
            changed.append(f"{name} {theirs} -> {mine}")
    if changed and rank == 0:
        print("grad_clip: the command line overrides checkpoint.pth (" + ", ".join(changed) + ")")


def format_clip_stats(opt, name=""):
    """The epoch line's grad-norm part (one host read), then the counters start again."""
    st = opt.clip_stats()
    opt.reset_clip_stats()
    return f" | grad norm{name} {st['last_norm']:.4f}, max {st['max_norm_seen']:.4f}, clipped {st['clipped']}/{st['steps']}"


def append_noise_level_record(run_dir, record):
    """{run_dir}/loss_by_noise_level.json: a list with one record per evaluated epoch (kept across resumes)."""
    import json
    path = os.path.join(run_dir, "loss_by_noise_level.json")
    records = []
    if os.path.exists(path):
        with open(path) as f:
            records = json.load(f)
    records.append(record)
    with open(path, "w") as f:
        json.dump(records, f, indent=1)
    return path


def format_noise_level_table(name, rows):
    cells = " ".join(f"[{r['t_lo']}-{r['t_hi']}] " + (f"{r['mean']:.5f}" if r["mean"] is not None else "-") + f" ({r['count']})" for r in rows)
    return f"  loss by noise level, {name}: {cells}"


def cpu_state(sd):
    return {k: v.cpu() for k, v in sd.items()}


def ema_checkpoint_entry(ema, best_loss):
    """The 'ema' entry of checkpoint.pth."""
    return {"decay": ema.decay, "warmup": ema.warmup, "num_updates": ema.num_updates, "best_loss": best_loss, "shadow": cpu_state(ema.state_dict())}


def ema_resume(ema, ck, rank=0):
    """Restores shadow and update count from a loaded checkpoint.pth (call after the model's weights have been loaded); returns the EMA's
    best validation loss.  A checkpoint without an EMA starts the average from the loaded weights."""
    if "ema" in ck:
        ema.load_state_dict(ck["ema"]["shadow"], num_updates=ck["ema"]["num_updates"])
        return float(ck["ema"]["best_loss"])
    ema.reset()
    if rank == 0:
        print("checkpoint.pth has no EMA: the average starts from the loaded weights")
    return float("inf")


def rng_seed(base_seed, role, rank=0, world=1):
    """Distinct Philox key per (role, rank): base * 2^20 + role * 4096 + rank.  Roles: 1 timesteps, 2 posterior eps, 3 diffusion
    noise, 4 autoencoder eps, 5-7 validation draws, 8 training loader (crop / shuffle / synthetic windows), 9 validation loader,
    10 label dropout of classifier-free guidance training (p_uncond), 11 context masks of training (--context), 12 context masks of the
    validation.  (seed + role + rank collides across ranks: rank r's noise stream == rank r+1's eps stream.)"""
    assert 0 <= rank < 4096 and 0 <= role < 256
    return (int(base_seed) << 20) + (int(role) << 12) + int(rank)
