"""Raw recordings in, the loader's files out: python -m eegldm.entry.prepare_recordings

    --edf 'raw/*-PSG.edf' --hypnogram_suffix -Hypnogram.edf          Sleep-EDF: the hypnogram shares the first six characters (SC4ssN)
    --edf 'edfs/shhs1-*.edf' --profusion_dir annotations/            SHHS: {stem}-profusion.xml

Every channel of --channels becomes {stem}-{channel}.npy (float32 (1, N): low-passed at --h_freq, resampled to --sfreq_out on the device, cut
to the sleep period +- --wake_mins at epoch boundaries) and {stem}-{channel}.stages.npy (int32, one code per 30-s epoch: W 0, N1 1, N2 2,
N3/N4 3, REM 4, -1 unscored, -2 rejected by --reject_ptp / --reject_flat).  ids.csv lists them (FILE_NAME_EEG without '.npy', as
read_ids(dataset="edfx") expects; recording, channel, sfreq_in, n_epochs, and subject / night where the name is SC4ssN... or shhs1-<id>);
--split a,b,c writes ids_train.csv / ids_valid.csv / ids_test.csv by subject; prepare_report.json holds what was read and done per file.
A file that fails is reported and skipped; the exit status is then 1.  This takes the place of convert_edfx.py / convert_shhs.py and of
split_train_valid_test_*.py; `eegldm.recordings` states how it differs from them (the filter is not mne's)."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import xml.etree.ElementTree as ET

import numpy as np

from ..recordings import channel_file_name, prepare_recording

ID_COLUMNS = ("FILE_NAME_EEG", "recording", "channel", "sfreq_in", "n_epochs", "subject", "night")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--edf", nargs="+", required=True, help="polysomnogram files or glob patterns")
    p.add_argument("--hypnogram_suffix", default=None, help="Sleep-EDF: the hypnogram is the file beside the PSG whose name starts with the "
                   "PSG's first six characters and ends with this suffix")
    p.add_argument("--profusion_dir", default=None, help="SHHS: directory of {stem}-profusion.xml")
    p.add_argument("--channels", nargs="+", required=True, help="signal labels as in the EDF header, e.g. 'EEG Fpz-Cz'")
    p.add_argument("--h_freq", type=float, default=18.0)
    p.add_argument("--sfreq_out", type=int, default=100)
    p.add_argument("--wake_mins", type=int, default=30)
    p.add_argument("--units", default="V", choices=["V", "uV"])
    p.add_argument("--reject_ptp", type=float, default=None, help="mark epochs with max - min above this (stored unit) as -2")
    p.add_argument("--reject_flat", type=float, default=None, help="mark epochs with sd at or below this (stored unit) as -2")
    p.add_argument("--split", default=None, help="train,valid,test shares by subject, e.g. 0.8,0.1,0.1")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--output_dir", required=True)
    # `--hypnogram_suffix -Hypnogram.edf`: argparse would take the value for an option, so the pair is joined with '=' first
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):
        if argv[i] == "--hypnogram_suffix":
            argv[i:i + 2] = [f"--hypnogram_suffix={argv[i + 1]}"]
            break
    a = p.parse_args(argv)
    if (a.hypnogram_suffix is None) == (a.profusion_dir is None):
        p.error("give exactly one of --hypnogram_suffix and --profusion_dir")
    return a


def find_hypnogram(edf, args):
    stem = os.path.basename(edf)
    stem = stem[:-4] if stem.lower().endswith(".edf") else stem
    if args.profusion_dir is not None:
        path = os.path.join(args.profusion_dir, stem + "-profusion.xml")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found")
        return path
    found = sorted(glob.glob(os.path.join(glob.escape(os.path.dirname(edf)), glob.escape(stem[:6]) + "*" + glob.escape(args.hypnogram_suffix))))
    if len(found) != 1:
        raise FileNotFoundError(f"{len(found)} files match {stem[:6]}*{args.hypnogram_suffix} beside {edf}")
    return found[0]


def subject_night(stem):
    """('ss', 'N') of SC4ssN..., ('<id>', '1') of shhs1-<id>, else ('', '')."""
    m = re.match(r"^S[CT][47](\d\d)(\d)", stem)
    if m:
        return m.group(1), m.group(2)
    m = re.match(r"^shhs1-(\d+)", stem)
    return (m.group(1), "1") if m else ("", "")


def split_subjects(rows, shares, seed):
    """{'train' / 'valid' / 'test': rows}: subjects shuffled with the seed and cut at the cumulative shares; a row without a subject counts as
    a subject of its own (its recording).  No subject lands in two sets."""
    key = lambda r: r["subject"] or r["recording"]
    subjects = sorted({key(r) for r in rows})
    order = [subjects[i] for i in np.random.default_rng(seed).permutation(len(subjects))]
    total = float(sum(shares))
    n_train = int(round(len(order) * shares[0] / total))
    n_valid = int(round(len(order) * (shares[0] + shares[1]) / total)) - n_train
    sets = {"train": set(order[:n_train]), "valid": set(order[n_train:n_train + n_valid]), "test": set(order[n_train + n_valid:])}
    return {name: [r for r in rows if key(r) in members] for name, members in sets.items()}


def write_ids(path, rows):
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=ID_COLUMNS)
        w.writeheader()
        w.writerows(rows)


def main(argv=None):
    args = parse_args(argv)
    shares = None
    if args.split is not None:
        shares = [float(v) for v in args.split.split(",")]
        if len(shares) != 3 or min(shares) < 0 or sum(shares) <= 0:
            raise ValueError(f"--split takes three non-negative shares, got {args.split!r}")
    files = sorted({f for pat in args.edf for f in (glob.glob(pat) or [pat])})
    os.makedirs(args.output_dir, exist_ok=True)
    rows, reports, failed = [], [], []
    for edf in files:
        stem = os.path.basename(edf)
        stem = stem[:-4] if stem.lower().endswith(".edf") else stem
        try:
            done = prepare_recording(edf, find_hypnogram(edf, args), args.channels, sfreq_out=args.sfreq_out, h_freq=args.h_freq,
                                     wake_mins=args.wake_mins, units=args.units, reject_ptp=args.reject_ptp, reject_flat=args.reject_flat)
        except (ValueError, OSError, RuntimeError, ET.ParseError) as e:
            print(f"FAILED {edf}: {e}", file=sys.stderr)
            failed.append({"edf": edf, "error": str(e)})
            continue
        subject, night = subject_night(stem)
        for channel, (signal, stages, report) in done.items():
            name = f"{stem}-{channel_file_name(channel)}"
            np.save(os.path.join(args.output_dir, name + ".npy"), signal)
            np.save(os.path.join(args.output_dir, name + ".stages.npy"), stages)
            rows.append({"FILE_NAME_EEG": name, "recording": stem, "channel": channel, "sfreq_in": report["sfreq_in"],
                         "n_epochs": report["n_epochs"], "subject": subject, "night": night})
            reports.append(dict(report, file=name))
            print(f"{name}: {report['sfreq_in']} Hz -> {report['sfreq_out']} Hz (U {report['U']}, D {report['D']}, {report['n_taps']} taps), "
                  f"epochs [{report['e0']}, {report['e1']}), stages {report['stage_counts']}")
    write_ids(os.path.join(args.output_dir, "ids.csv"), rows)
    if shares is not None:
        for name, part in split_subjects(rows, shares, args.seed).items():
            write_ids(os.path.join(args.output_dir, f"ids_{name}.csv"), part)
    with open(os.path.join(args.output_dir, "prepare_report.json"), "w") as f:
        json.dump({"files": reports, "failed": failed}, f, indent=1)
    print(f"{len(rows)} files written to {args.output_dir}, {len(failed)} recordings failed")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
