"""Seams of a long recording beside the window interiors (numpy only): RMS of the signal and of its first difference inside each ramp
span of long_{seed}_layout.json against the same figures over the window interiors, per seam and pooled.  A ramp of length 0 (hard
switch) is looked at over --halfwidth samples on either side of the switch.  The report makes no claim about plausibility; it is what
--margin / --ramp of eegldm.entry.sample_long are tuned by.

    python tools/seam_report.py long_0.npy long_0_layout.json [--halfwidth 8] [--json]
"""
import argparse
import json

import numpy as np


def _rms(v):
    v = np.asarray(v, np.float64)
    return float(np.sqrt(np.mean(v * v))) if v.size else float("nan")


def seam_report(signal, layout, halfwidth=8):
    """signal: the recording, any shape whose last axis is time; layout: the dict of long_{seed}_layout.json.  -> dict(seams=[...],
    pooled=..., interior=...): rms / diff_rms per seam span, pooled over the seams, and over the interiors; ratio_* = seam / interior."""
    x = np.asarray(signal, np.float64)
    x = x.reshape(-1, x.shape[-1])
    n = x.shape[-1]
    spans = []
    for a, b in layout["seams"]:
        if b - a < 2:                                   # hard switch: the samples around it
            a, b = a - halfwidth, a + halfwidth
        spans.append((max(0, int(a)), min(n, int(b))))
    inside = np.zeros(n, bool)
    for a, b in spans:
        inside[a:b] = True
    # a difference belongs to a span when both of its samples do
    d = np.diff(x, axis=-1)
    d_in = inside[1:] & inside[:-1]
    d_out = ~inside[1:] & ~inside[:-1]
    interior = dict(rms=_rms(x[:, ~inside]), diff_rms=_rms(d[:, d_out]))
    seams = []
    for k, (a, b) in enumerate(spans):
        s = dict(seam=k + 1, span=[a, b], rms=_rms(x[:, a:b]), diff_rms=_rms(d[:, a:b - 1]))
        s["ratio_rms"], s["ratio_diff_rms"] = s["rms"] / interior["rms"], s["diff_rms"] / interior["diff_rms"]
        seams.append(s)
    pooled = dict(rms=_rms(x[:, inside]), diff_rms=_rms(d[:, d_in]))
    pooled["ratio_rms"], pooled["ratio_diff_rms"] = pooled["rms"] / interior["rms"], pooled["diff_rms"] / interior["diff_rms"]
    return dict(seams=seams, pooled=pooled, interior=interior)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("recording"); ap.add_argument("layout")
    ap.add_argument("--halfwidth", type=int, default=8)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args(argv)
    rep = seam_report(np.load(args.recording), json.load(open(args.layout)), args.halfwidth)
    if args.json:
        print(json.dumps(rep))
        return rep
    i = rep["interior"]
    print(f"interior: rms {i['rms']:.5g}, first-difference rms {i['diff_rms']:.5g}")
    for s in rep["seams"] + [dict(rep["pooled"], seam="pooled", span=["", ""])]:
        print(f"seam {s['seam']} {s['span']}: rms {s['rms']:.5g} (x{s['ratio_rms']:.3f} of interior), first-difference rms {s['diff_rms']:.5g} "
              f"(x{s['ratio_diff_rms']:.3f})")
    return rep


if __name__ == "__main__":
    main()
