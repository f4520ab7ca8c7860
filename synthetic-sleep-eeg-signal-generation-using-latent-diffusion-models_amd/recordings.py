"""Preparing raw recordings: EDF / EDF+ polysomnograms and their hypnograms in, the loader's files out (R.npy: one channel at 100 Hz,
low-passed at 18 Hz, float32 (1, N); R.stages.npy: int32, one code per 30-s epoch, W 0, N1 1, N2 2, N3/N4 3, REM 4, negative = unscored).

File parsing is numpy and the standard library.  The signal path is two device calls (csrc/resample.hip): `resample_fir`, a zero-phase
polyphase FIR that low-passes and changes the rate of a whole night in one pass, reading EDF's int16 samples directly, and `epoch_stats`,
(min, max, mean, sd) per epoch.  Everything that refuses an argument does so with ValueError before the device is touched.

THE FILTER IS NOT mne's: `lowpass_resample_design` follows this project's recollection of mne's firwin defaults (Hamming window, transition
min(max(0.25 h_freq, 2), Nyquist - h_freq), 3.3 / width taps) and is pinned to nothing; the resampler is a polyphase FIR, not mne's FFT
method, and ONE filter at the virtual rate sfreq_in U serves both raw.filter(h_freq=18) and raw.resample(100)."""
import os
import re
import xml.etree.ElementTree as ET
from fractions import Fraction

import numpy as np
import torch

from ._lib import check, default_context, lib, ptr
from .metrics import fir_length

RS_MAX_TAPS, RS_MAX_U, RS_MAX_D, RS_MAX_LEN, EPOCH_MAX = 16383, 64, 4096, 1 << 30, 12288
RS_EDGES = {"zero": 0, "reflect": 1}
ANNOTATION_LABEL = "EDF Annotations"
STAGE_UNSCORED, STAGE_REJECTED = -1, -2
UNIT_VOLTS = {"uV": 1e-6, "mV": 1e-3, "V": 1.0}


# ---------------------------------------------------------------------------------------------------- EDF
def _field(b):
    return b.decode("latin-1").strip()


def _read_header(path):
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(256)
        if len(head) < 256:
            raise ValueError(f"{path}: truncated: {len(head)} bytes, the fixed EDF header alone has 256")
        try:
            ns = int(_field(head[252:256]))
            header_bytes = int(_field(head[184:192]))
            n_records = int(_field(head[236:244]))
            duration_text = _field(head[244:252])
            duration = Fraction(duration_text)
        except ValueError as e:
            raise ValueError(f"{path}: not an EDF header ({e})") from None
        if ns < 1 or header_bytes != 256 * (ns + 1):
            raise ValueError(f"{path}: header of {header_bytes} bytes does not match {ns} signals")
        sig = f.read(256 * ns)
    if len(sig) < 256 * ns:
        raise ValueError(f"{path}: truncated inside the signal headers")
    reserved = _field(head[192:236])
    if reserved.startswith("EDF+D"):
        raise ValueError(f"{path}: EDF+D (discontinuous recording) is not supported")

    def col(off, width):
        return [_field(sig[off * ns + i * width:off * ns + (i + 1) * width]) for i in range(ns)]

    labels, dims = col(0, 16), col(96, 8)
    try:
        pmin, pmax = [float(v) for v in col(104, 8)], [float(v) for v in col(112, 8)]
        dmin, dmax = [int(v) for v in col(120, 8)], [int(v) for v in col(128, 8)]
        spr = [int(v) for v in col(216, 8)]
    except ValueError as e:
        raise ValueError(f"{path}: unreadable signal header ({e})") from None
    if min(spr) < 0 or sum(spr) < 1:
        raise ValueError(f"{path}: samples per record {spr}")
    record_bytes = 2 * sum(spr)
    body = size - header_bytes
    if n_records == -1:
        n_records = body // record_bytes
        if n_records * record_bytes != body:
            raise ValueError(f"{path}: truncated: {body} data bytes are no whole number of {record_bytes}-byte records")
    elif n_records < 0 or body < n_records * record_bytes:
        raise ValueError(f"{path}: truncated: {n_records} records of {record_bytes} bytes announced, {body} data bytes present")
    return {"path": path, "version": _field(head[0:8]), "patient": _field(head[8:88]), "recording": _field(head[88:168]),
            "startdate": _field(head[168:176]), "starttime": _field(head[176:184]), "header_bytes": header_bytes, "reserved": reserved,
            "n_records": n_records, "record_duration": duration, "record_duration_text": duration_text, "n_signals": ns, "labels": labels,
            "dimensions": dims, "physical_min": pmin, "physical_max": pmax, "digital_min": dmin, "digital_max": dmax,
            "samples_per_record": spr}


def _read_records(h):
    """(n_records, samples per record) int16 of the data part."""
    n = sum(h["samples_per_record"])
    with open(h["path"], "rb") as f:
        f.seek(h["header_bytes"])
        a = np.fromfile(f, dtype="<i2", count=h["n_records"] * n)
    if a.size != h["n_records"] * n:
        raise ValueError(f"{h['path']}: truncated: {a.size} of {h['n_records'] * n} samples read")
    return a.reshape(h["n_records"], n)


def read_edf(path, channels=None):
    """{'header': the fields of the fixed and the per-signal headers, 'signals': {label: {...}}} of an EDF / EDF+C file.  A signal is
    {'data': int16 (N,), 'sfreq': Fraction (samples per record over the record duration, the duration parsed from its decimal text),
    'gain', 'offset' (float64: physical = digital * gain + offset), 'dimension', 'physical_min/max', 'digital_min/max'}.  channels: labels to
    read (default: every signal but the annotations).  A record count of -1 is derived from the file size.  ValueError: EDF+D, a truncated
    file, digital_max == digital_min, an unknown channel (the message lists the labels present)."""
    h = _read_header(path)
    labels = h["labels"]
    if channels is None:
        channels = [n for n in labels if n != ANNOTATION_LABEL]
    missing = [c for c in channels if c not in labels]
    if missing:
        raise ValueError(f"{path}: no channel {missing}; the file has {labels}")
    if h["record_duration"] <= 0 and any(c != ANNOTATION_LABEL for c in channels):
        raise ValueError(f"{path}: record duration {h['record_duration_text']!r} gives no sampling rate")
    rec = _read_records(h)
    start = np.concatenate([[0], np.cumsum(h["samples_per_record"])])
    signals = {}
    for c in channels:
        i = labels.index(c)
        dmin, dmax = h["digital_min"][i], h["digital_max"][i]
        if dmax == dmin:
            raise ValueError(f"{path}: channel {c!r} has digital_max == digital_min == {dmax}: no gain")
        gain = (h["physical_max"][i] - h["physical_min"][i]) / (dmax - dmin)
        signals[c] = {"data": np.ascontiguousarray(rec[:, start[i]:start[i + 1]]).reshape(-1).astype(np.int16, copy=False),
                      "sfreq": Fraction(h["samples_per_record"][i]) / h["record_duration"], "gain": gain,
                      "offset": h["physical_min"][i] - dmin * gain, "dimension": h["dimensions"][i],
                      "physical_min": h["physical_min"][i], "physical_max": h["physical_max"][i], "digital_min": dmin, "digital_max": dmax}
    return {"header": h, "signals": signals}


def read_edf_annotations(path):
    """[(onset_s, duration_s, text), ...] from the time-stamped annotation lists of the 'EDF Annotations' signal of an EDF+ file
    (+onset\\x15duration\\x14text\\x14\\x00; the format of Sleep-EDF's *-Hypnogram.edf).  The empty time-keeping entries are left out."""
    h = _read_header(path)
    if ANNOTATION_LABEL not in h["labels"]:
        raise ValueError(f"{path}: no {ANNOTATION_LABEL!r} signal; the file has {h['labels']}")
    rec = _read_records(h)
    start = np.concatenate([[0], np.cumsum(h["samples_per_record"])])
    out = []
    for i, name in enumerate(h["labels"]):
        if name != ANNOTATION_LABEL:
            continue
        for row in rec[:, start[i]:start[i + 1]]:
            for tal in np.ascontiguousarray(row).tobytes().split(b"\x00"):
                if not tal:
                    continue
                parts = tal.split(b"\x14")
                stamp = parts[0].split(b"\x15")
                try:
                    onset = float(stamp[0])
                    duration = float(stamp[1]) if len(stamp) > 1 and stamp[1] else 0.0
                except ValueError:
                    raise ValueError(f"{path}: unreadable annotation time stamp {parts[0]!r}") from None
                out += [(onset, duration, t.decode("utf-8", "replace")) for t in parts[1:] if t]
    return sorted(out, key=lambda a: a[0])


def read_profusion_stages(path):
    """int32 codes of the SleepStages / SleepStage elements of an SHHS profusion XML, found by tag (0 W, 1..4 N1..N4, 5 REM, above: unscored)."""
    root = ET.parse(path).getroot()
    node = root if root.tag == "SleepStages" else root.find(".//SleepStages")
    if node is None:
        raise ValueError(f"{path}: no SleepStages element")
    try:
        codes = [int(e.text) for e in node.iter("SleepStage")]
    except (TypeError, ValueError):
        raise ValueError(f"{path}: a SleepStage element holds no integer") from None
    return np.asarray(codes, np.int32)


# ---------------------------------------------------------------------------------------------------- stages
_STAGE_OF_LAST_CHAR = {"W": 0, "1": 1, "2": 2, "3": 3, "4": 3, "R": 4}      # run_sleep_decode.py:112-118


def stages_from_annotations(annots, n_epochs, epoch_s=30):
    """int32 (n_epochs,) in the loader's codes from 'Sleep stage X' annotations: W 0, 1 1, 2 2, 3 and 4 3, R 4; 'Sleep stage ?', 'Movement
    time' and epochs no annotation covers are -1.  An annotation that spans k epochs fills k epochs; an onset that is no multiple of the
    epoch is refused; a duration that is none fills the whole epochs it covers (the ragged rest stays uncovered: -1); other annotations are
    ignored."""
    out = np.full(int(n_epochs), STAGE_UNSCORED, np.int32)
    for onset, duration, text in annots:
        text = text.strip()
        if text.startswith("Sleep stage "):
            code = _STAGE_OF_LAST_CHAR.get(text[-1], STAGE_UNSCORED)
        elif text == "Movement time":
            code = STAGE_UNSCORED
        else:
            continue
        e0, k = onset / epoch_s, duration / epoch_s
        if e0 != int(e0) or e0 < 0:
            raise ValueError(f"annotation {text!r} starts at {onset} s, no multiple of the {epoch_s}-s epoch")
        out[int(e0):int(e0) + int(k)] = code
    return out


def stages_from_profusion(codes):
    """Profusion codes to the loader's: 4 -> 3, 5 -> 4 (convert_shhs.py:85-92), codes above 5 (and negative ones) -> -1."""
    c = np.asarray(codes).astype(np.int64).reshape(-1)
    out = np.where(c == 4, 3, np.where(c == 5, 4, c))
    return np.where((c > 5) | (c < 0), STAGE_UNSCORED, out).astype(np.int32)


def sleep_span(stages, wake_mins=30):
    """(e0, e1): the epochs [e0, e1) from wake_mins before the first epoch scored 1..4 to wake_mins behind the last one, clamped to the night
    (convert_shhs.py:103-111; two epochs per minute)."""
    s = np.asarray(stages).reshape(-1)
    idx = np.nonzero((s >= 1) & (s <= 4))[0]
    if idx.size == 0:
        raise ValueError("no epoch is scored as sleep (1..4): nothing to cut the night around")
    w = 2 * int(wake_mins)
    return max(0, int(idx[0]) - w), min(int(s.size), int(idx[-1]) + 1 + w)


# ---------------------------------------------------------------------------------------------------- filter design
def _fraction(v):
    if isinstance(v, Fraction):
        return v
    f = Fraction(v) if isinstance(v, (int, np.integer)) else Fraction(repr(float(v)))
    return f


def resample_ratio(sfreq_in, sfreq_out):
    """(U, D) reduced, sfreq_out / sfreq_in = U / D."""
    a, b = _fraction(sfreq_in), _fraction(sfreq_out)
    if not (a > 0 and b > 0):
        raise ValueError(f"sampling rates must be positive, got {sfreq_in} and {sfreq_out}")
    r = b / a
    return r.numerator, r.denominator


def lowpass_resample_design(sfreq_in, sfreq_out, h_freq=18.0):
    """(U, D, taps float64): ONE Hamming-windowed-sinc low-pass at the virtual rate sfreq_in U that is both the h_freq low-pass and the
    anti-aliasing / anti-imaging filter of the rate change.  Transition width min(max(0.25 h_freq, 2), min(sfreq_in, sfreq_out) / 2 - h_freq),
    half-amplitude point h_freq + width / 2, length the smallest odd integer >= 3.3 rate / width (`fir_length`), DC gain U (so that the
    zero-stuffed signal keeps its level).  Refused: U > 64, more than 16383 taps, h_freq at or above either Nyquist rate."""
    u, d = resample_ratio(sfreq_in, sfreq_out)
    fin, fout, h = float(_fraction(sfreq_in)), float(_fraction(sfreq_out)), float(h_freq)
    if not h > 0:
        raise ValueError(f"h_freq must be positive, got {h_freq}")
    nyq = 0.5 * min(fin, fout)
    if h >= nyq:
        raise ValueError(f"h_freq = {h_freq} Hz is not below the Nyquist rates of {fin} and {fout} Hz ({0.5 * fin}, {0.5 * fout})")
    if u > RS_MAX_U:
        raise ValueError(f"{fin} -> {fout} Hz needs U = {u} (D = {d}); eegldm_resample_fir takes U <= {RS_MAX_U}")
    if d > RS_MAX_D:
        raise ValueError(f"{fin} -> {fout} Hz needs D = {d} (U = {u}); eegldm_resample_fir takes D <= {RS_MAX_D}")
    width = min(max(0.25 * h, 2.0), nyq - h)
    rate = fin * u
    m = fir_length(rate, width)
    if m > RS_MAX_TAPS:
        raise ValueError(f"{fin} -> {fout} Hz with a {width} Hz transition needs {m} taps at {rate} Hz; eegldm_resample_fir takes {RS_MAX_TAPS}")
    right = (h + 0.5 * width) / (0.5 * rate)
    k = np.arange(m, dtype=np.float64) - 0.5 * (m - 1)
    taps = right * np.sinc(right * k) * np.hamming(m)
    return u, d, taps * (u / np.sum(taps))


# ---------------------------------------------------------------------------------------------------- device calls
def _as_rows(x, name):
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    if x.dim() == 1:
        x = x[None]
    if x.dim() == 3 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 2:
        raise ValueError(f"{name}: rows (B, L) expected, got shape {tuple(x.shape)}")
    return x


def _rows_on(x, dev, dtype):
    x = x.to(dev, dtype)
    if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def _ld(t):
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


def _per_row(v, rows, name):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, rows)
    if a.size != rows:
        raise ValueError(f"{name}: one value per row ({rows}) expected, got {a.size}")
    with np.errstate(over="ignore"):
        if not np.all(np.isfinite(a.astype(np.float32))):
            raise ValueError(f"{name}: non-finite values (as fp32)")
    return a.astype(np.float32)


def resample_fir(x, taps, U, D, edge="reflect", gain=None, offset=None, ctx=None):
    """eegldm_resample_fir over the rows of x: (B, ceil(L U / D)) fp32 on the device.  y[m] = sum_k taps[k] v[m D + k - c], v the row
    zero-stuffed by U and extended by zeros ("zero") or whole-sample reflection ("reflect").  x is floating point (taken as fp32) or int16
    with per-row gain and offset (the sample is fmaf(d, gain, offset) in fp32); rows (B, L), (B, 1, L) or one row (L,)."""
    x = _as_rows(x, "x")
    t = np.asarray(taps, np.float64).reshape(-1)
    if edge not in RS_EDGES:
        raise ValueError(f"edge must be one of {tuple(RS_EDGES)}, got {edge!r}")
    if not 1 <= t.size <= RS_MAX_TAPS or t.size % 2 == 0:
        raise ValueError(f"an odd number of taps in 1..{RS_MAX_TAPS} is needed, got {t.size}")
    with np.errstate(over="ignore"):
        if not np.all(np.isfinite(t.astype(np.float32))):
            raise ValueError("non-finite taps (as fp32)")
    if int(U) != U or not 1 <= int(U) <= RS_MAX_U:
        raise ValueError(f"U must be an integer in 1..{RS_MAX_U}, got {U}")
    if int(D) != D or not 1 <= int(D) <= RS_MAX_D:
        raise ValueError(f"D must be an integer in 1..{RS_MAX_D}, got {D}")
    U, D = int(U), int(D)
    B, L = int(x.shape[0]), int(x.shape[1])
    if not 1 <= L <= RS_MAX_LEN:
        raise ValueError(f"rows of 1..2^30 samples are taken, got {L}")
    c = (t.size - 1) // 2
    if edge == "reflect" and -(-c // U) > L - 1:
        raise ValueError(f"reflect needs ceil(c / U) <= L - 1, got {t.size} taps, U = {U}, rows of {L} samples")
    is_i16 = x.dtype == torch.int16
    if not is_i16 and not x.dtype.is_floating_point:
        raise ValueError(f"x must be floating point or int16, got {x.dtype}")
    if is_i16:
        if gain is None or offset is None:
            raise ValueError("int16 rows need gain and offset (physical = digital * gain + offset)")
        g, o = _per_row(gain, B, "gain"), _per_row(offset, B, "offset")
    elif gain is not None or offset is not None:
        raise ValueError("gain / offset belong to int16 rows; floating-point rows are taken as they are")
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    xd = _rows_on(x, dev, torch.int16 if is_i16 else torch.float32)
    lout = -(-L * U // D)
    out = torch.empty(B, lout, device=dev)
    if B:
        td = torch.from_numpy(t.astype(np.float32)).to(dev)
        gd = torch.from_numpy(g).to(dev) if is_i16 else None
        od = torch.from_numpy(o).to(dev) if is_i16 else None
        check(lib.eegldm_resample_fir(ctx.h, ptr(xd), _ld(xd), 1 if is_i16 else 0, ptr(gd), ptr(od), ptr(td), int(t.size), U, D, ptr(out), lout, B, L,
                                      RS_EDGES[edge]))
    return out


def epoch_stats(x, epoch_len, ctx=None):
    """eegldm_epoch_stats: (B, L // epoch_len, 4) fp32 on the device, (min, max, mean, sd) of every whole epoch; mean and sd from float64 sums,
    the sd about the mean; a NaN in an epoch makes its four values NaN."""
    x = _as_rows(x, "x")
    if int(epoch_len) != epoch_len or not 1 <= int(epoch_len) <= EPOCH_MAX:
        raise ValueError(f"epoch_len must be an integer in 1..{EPOCH_MAX}, got {epoch_len}")
    if not x.dtype.is_floating_point:
        raise ValueError(f"x must be floating point, got {x.dtype}")
    if x.shape[1] > RS_MAX_LEN:
        raise ValueError(f"rows of at most 2^30 samples are taken, got {x.shape[1]}")
    E = int(epoch_len)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    xd = _rows_on(x, dev, torch.float32)
    B, L = int(xd.shape[0]), int(xd.shape[1])
    out = torch.empty(B, L // E, 4, device=dev)
    if B and L // E:
        check(lib.eegldm_epoch_stats(ctx.h, ptr(xd), _ld(xd), B, L, E, ptr(out)))
    return out


# ---------------------------------------------------------------------------------------------------- one recording
def channel_file_name(label):
    """The channel's part of an output file name: 'EEG Fpz-Cz' -> 'Fpz-Cz' (the reference renames its channels so), then every character outside
    [A-Za-z0-9._-] becomes '_'."""
    name = label[4:] if label.startswith("EEG ") else label
    return re.sub(r"[^A-Za-z0-9._-]", "_", name.strip())


def _quartiles(a):
    a = a[np.isfinite(a)]
    return [float(v) for v in np.percentile(a, [0, 25, 50, 75, 100])] if a.size else None


def prepare_recording(edf, hypnogram, channels, sfreq_out=100, h_freq=18.0, wake_mins=30, units="V", reject_ptp=None, reject_flat=None,
                      epoch_s=30, ctx=None):
    """{channel: (signal float32 (1, N), stages int32 (N / epoch,), report)} for one polysomnogram and its hypnogram (an EDF+ annotation file,
    or a profusion XML when the name ends in .xml).  The whole recording is low-passed at h_freq and resampled to sfreq_out on the device
    (edges by reflection), then trimmed to the whole epochs both files cover and cut to `sleep_span`.  units "V" stores volts (physical
    dimensions uV / mV / V are converted through the gain), "uV" microvolts.  reject_ptp / reject_flat mark epochs with max - min > X or
    sd <= Y as -2 (in the stored unit; off by default)."""
    if units not in ("V", "uV"):
        raise ValueError(f"units must be 'V' or 'uV', got {units!r}")
    rec = read_edf(edf, channels)
    head = rec["header"]
    epoch = _fraction(sfreq_out) * epoch_s
    if epoch.denominator != 1 or not 1 <= epoch.numerator <= EPOCH_MAX:
        raise ValueError(f"an epoch of {epoch_s} s at {sfreq_out} Hz is {epoch} samples: a whole number in 1..{EPOCH_MAX} is needed")
    epoch = int(epoch)
    if str(hypnogram).lower().endswith(".xml"):
        all_stages, source = stages_from_profusion(read_profusion_stages(hypnogram)), "profusion"
    else:
        hh = _read_header(hypnogram)
        if (hh["startdate"], hh["starttime"]) != (head["startdate"], head["starttime"]):
            raise ValueError(f"{hypnogram} starts at {hh['startdate']} {hh['starttime']}, {edf} at {head['startdate']} {head['starttime']}: "
                             "not the same recording")
        annots = read_edf_annotations(hypnogram)
        scored = [a for a in annots if a[2].startswith("Sleep stage ") or a[2] == "Movement time"]
        n_h = int(max((a[0] + a[1]) // epoch_s for a in scored)) if scored else 0
        all_stages, source = stages_from_annotations(annots, n_h, epoch_s), "annotations"
    ctx = ctx or default_context(0)
    out = {}
    for name in channels:
        s = rec["signals"][name]
        if s["dimension"] not in UNIT_VOLTS:
            raise ValueError(f"{edf}: channel {name!r} has physical dimension {s['dimension']!r}; one of {tuple(UNIT_VOLTS)} is needed")
        scale = UNIT_VOLTS[s["dimension"]] * (1.0 if units == "V" else 1e6)
        u, d, taps = lowpass_resample_design(s["sfreq"], sfreq_out, h_freq)
        y = resample_fir(torch.from_numpy(s["data"])[None], taps, u, d, "reflect", gain=s["gain"] * scale, offset=s["offset"] * scale, ctx=ctx)
        n = min(int(y.shape[1]) // epoch, int(all_stages.size))
        e0, e1 = sleep_span(all_stages[:n], wake_mins)
        cut = y[:, e0 * epoch:e1 * epoch]
        stats = epoch_stats(cut, epoch, ctx=ctx)[0].cpu().numpy().astype(np.float64)
        stages = all_stages[e0:e1].copy()
        ptp, sd = stats[:, 1] - stats[:, 0], stats[:, 3]
        rej_ptp = (ptp > reject_ptp) if reject_ptp is not None else np.zeros(len(stages), bool)
        rej_flat = (sd <= reject_flat) if reject_flat is not None else np.zeros(len(stages), bool)
        stages[rej_ptp | rej_flat] = STAGE_REJECTED
        report = {"edf": os.path.basename(str(edf)), "hypnogram": os.path.basename(str(hypnogram)), "stage_source": source, "channel": name,
                  "startdate": head["startdate"], "starttime": head["starttime"], "n_records": head["n_records"],
                  "record_duration": head["record_duration_text"], "sfreq_in": str(s["sfreq"]), "sfreq_out": str(_fraction(sfreq_out)),
                  "dimension": s["dimension"], "units": units, "gain": s["gain"], "offset": s["offset"], "U": u, "D": d, "n_taps": int(taps.size),
                  "h_freq": float(h_freq), "n_samples_in": int(s["data"].size), "n_samples_resampled": int(y.shape[1]),
                  "n_epochs_recording": int(y.shape[1]) // epoch, "n_epochs_hypnogram": int(all_stages.size), "e0": e0, "e1": e1,
                  "n_epochs": e1 - e0, "stage_counts": {str(int(k)): int(v) for k, v in zip(*np.unique(stages, return_counts=True))},
                  "rejected_ptp": int(rej_ptp.sum()), "rejected_flat": int(rej_flat.sum()),
                  "epoch_quartiles": {"ptp": _quartiles(ptp), "mean": _quartiles(stats[:, 2]), "sd": _quartiles(sd)}}
        out[name] = (cut.cpu().numpy().astype(np.float32, copy=False).reshape(1, -1), stages.astype(np.int32), report)
    return out
