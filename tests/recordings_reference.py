"""float64 numpy references of the two primitives of csrc/resample.hip, the bounds they are held to, and test-only writers of the files
eegldm.recordings reads.  Shared by tests/test_recordings_cpu.py and tests/test_gpu_resample_fir.py.

eegldm_resample_fir.  `resample64` evaluates the definition in float64 FROM THE fp32 INPUTS (x, taps, gain, offset are the values handed to
the call; an int16 sample enters as the exact float64 d * gain + offset):

    c = (M - 1) / 2,  v[i] = xe[i / U] where U divides i, else 0,  y[m] = sum_k taps[k] v[m D + k - c],  m in [0, ceil(L U / D))
    edge 0: xe is zero outside [0, L);   edge 1: xe[-i] = x[i], xe[L-1+i] = x[L-1-i]

It is computed phase by phase: the outputs m = p, p + U, ... share the taps k0, k0 + U, ... with k0 = (c - p D) mod U, and their first
samples advance by D, so they are the product of a strided window view of the extended row with those taps.  `resample64_stuffed` is the independent
restatement (zero-stuff, np.convolve, stride) the CPU tests hold it to.

Error bound (`resample_error_bound`), u = 2^-24, g(n) = n u / (1 - n u), n = ceil(M / U) the most terms an output has:
* fp32 rows: one fmaf chain of at most n steps from +0:                          e = g(n) A + n 2^-126,   A = sum_k |taps[k]| |v|
* int16 rows: the device converts with ONE fp32 rounding, fmaf((float)d, gain, offset), which the float64 reference does not make; it is part
  of the error as the square is in the RMS bound of events_reference:           e = (u + g(n) (1 + u)) A + n 2^-126,  A on d * gain + offset

eegldm_epoch_stats.  `epoch_stats64`: (min, max, mean, sd) per whole epoch in float64, sd = sqrt(mean((x - mean)^2)).  Bounds (the final
roundings of float64 accumulations, whose own error is ~E 2^-53 and vanishes beside u): |mean - ref| <= 2 u |mean| + u max|x|,
|sd - ref| <= 4 u (sd + |mean|).
"""
import numpy as np

from events_reference import TINY, U as EPS, extend, g

PASS_TOL, STOP_TOL = 5e-3, 4e-3          # |H / U - 1| up to h_freq, |H / U| from h_freq + width: the design evaluated in float64 gives 4.1e-3 / 2.9e-3


# ---------------------------------------------------------------------------------------------------- resampler
def out_len(L, U, D):
    return -(-int(L) * int(U) // int(D))


def staged64(x, gain=None, offset=None):
    """(B, L) float64 of what enters the chain, without the int16 path's fp32 rounding."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        gn = np.asarray(gain, np.float32).astype(np.float64).reshape(-1, 1)
        of = np.asarray(offset, np.float32).astype(np.float64).reshape(-1, 1)
        return x.astype(np.float64) * gn + of
    return x.astype(np.float32).astype(np.float64)


_BLOCK = 16384        # outputs per matrix-vector product: bounds the copy numpy makes of the strided window view


def _poly(xs, h, U, D, edge):
    """sum_k h[k] v[m D + k - c] on float64 rows xs (B, L) with float64 taps h."""
    B, L = xs.shape
    M = len(h)
    c = (M - 1) // 2
    lout = out_len(L, U, D)
    pad = -(-c // U)
    xe = extend(xs, pad, edge)
    y = np.zeros((B, lout))
    for p in range(min(U, lout)):
        q = p * D - c
        k0 = (-q) % U
        hp = h[k0::U]
        if len(hp) == 0:
            continue
        j0 = (q + k0) // U
        n = len(range(p, lout, U))
        with np.errstate(all="ignore"):
            for b in range(B):
                w = np.lib.stride_tricks.sliding_window_view(xe[b], len(hp))[j0 + pad::D][:n]      # row i: xe[j0 + i D .. + nt), a view
                y[b, p::U] = np.concatenate([w[i:i + _BLOCK] @ hp for i in range(0, n, _BLOCK)])
    return y


def resample64(x, taps, U, D, edge=0, gain=None, offset=None):
    """The definition in float64 from the fp32 (or int16 + fp32 gain / offset) inputs: (B, ceil(L U / D)) float64."""
    return _poly(staged64(x, gain, offset), np.asarray(taps, np.float32).astype(np.float64), U, D, edge)


def resample64_stuffed(x, taps, U, D, edge=0, gain=None, offset=None):
    """The same by the textbook route: extend, zero-stuff by U, np.convolve with the taps, take every D-th value from the centre tap on."""
    xs = staged64(x, gain, offset)
    h = np.asarray(taps, np.float32).astype(np.float64)
    B, L = xs.shape
    c = (len(h) - 1) // 2
    pad = -(-c // U)
    xe = extend(xs, pad, edge)
    v = np.zeros((B, xe.shape[1] * U))
    v[:, ::U] = xe
    lout = out_len(L, U, D)
    # sample j sits at v[(j + pad) U], so y[m] = sum_k h[k] v[m D + k - c + pad U]: the convolution with the reversed taps at i = m D - c + pad U + M - 1
    out = np.zeros((B, lout))
    for b in range(B):
        full = np.convolve(v[b], h[::-1])                # full[i] = sum_k h[k] v[i - (M - 1) + k]
        out[b] = full[pad * U - c + len(h) - 1::D][:lout]
    return out


def resample_error_bound(x, taps, U, D, edge=0, gain=None, offset=None):
    """E (B, Lout): |y_device - resample64| <= E elementwise for finite inputs."""
    h = np.abs(np.asarray(taps, np.float32).astype(np.float64))
    n = -(-len(h) // U)
    A = _poly(np.abs(staged64(x, gain, offset)), h, U, D, edge)
    if np.asarray(x).dtype == np.int16:
        return (EPS + g(n) * (1.0 + EPS)) * A + n * TINY
    return g(n) * A + n * TINY


def resample_support_mask(L, M, U, D, idx, edge=0):
    """True at the outputs m one of whose terms holds sample idx (under edge 1 its reflected copies count too)."""
    hit = np.zeros((1, L))
    hit[0, idx] = 1.0
    return _poly(hit, np.ones(M), U, D, edge)[0] > 0


# ---------------------------------------------------------------------------------------------------- epoch statistics
def epoch_stats64(x, E):
    """(B, L // E, 4) float64: (min, max, mean, sd) of the whole epochs of fp32 rows; a NaN in an epoch makes its four values NaN."""
    x = np.asarray(x, np.float32).astype(np.float64)
    B, L = x.shape
    n = L // E
    e = x[:, :n * E].reshape(B, n, E)
    with np.errstate(all="ignore"):
        mean = e.sum(-1) / E
        sd = np.sqrt(((e - mean[..., None]) ** 2).sum(-1) / E)
        out = np.stack([e.min(-1), e.max(-1), mean, sd], -1)
    out[np.isnan(e).any(-1)] = np.nan
    return out


def epoch_stats_bounds(x, E):
    """(mean bound, sd bound), each (B, L // E)."""
    ref = epoch_stats64(x, E)
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.shape[1] // E
    amax = np.abs(x[:, :n * E].reshape(x.shape[0], n, E)).max(-1)
    return 2 * EPS * np.abs(ref[..., 2]) + EPS * amax, 4 * EPS * (ref[..., 3] + np.abs(ref[..., 2]))


# ---------------------------------------------------------------------------------------------------- frequency response
def response(taps, rate, n_fft=1 << 20):
    """(freqs, |H|) of the taps at sampling rate `rate` on an n_fft-point transform."""
    H = np.abs(np.fft.rfft(np.asarray(taps, np.float64), n_fft))
    return np.arange(len(H)) * (rate / n_fft), H


# ---------------------------------------------------------------------------------------------------- file writers (tests only)
def _pad(s, n):
    b = str(s).encode("latin-1")
    assert len(b) <= n, (s, n)
    return b + b" " * (n - len(b))


def write_edf(path, signals, record_duration="1", n_records=None, startdate="01.01.89", starttime="22.00.00", reserved="", announce=None):
    """signals: list of dicts {label, data int16 (n_records * spr,), spr, pmin, pmax, dmin, dmax, dim}.  announce: the record count written into
    the header (default the true one; -1 = unknown)."""
    ns = len(signals)
    nrec = n_records if n_records is not None else len(signals[0]["data"]) // signals[0]["spr"]
    head = (_pad("0", 8) + _pad("X X X X", 80) + _pad("Startdate X X X X", 80) + _pad(startdate, 8) + _pad(starttime, 8) + _pad(256 * (ns + 1), 8)
            + _pad(reserved, 44) + _pad(nrec if announce is None else announce, 8) + _pad(record_duration, 8) + _pad(ns, 4))
    cols = [(16, "label"), (80, None), (8, "dim"), (8, "pmin"), (8, "pmax"), (8, "dmin"), (8, "dmax"), (80, None), (8, "spr"), (32, None)]
    for width, key in cols:
        for s in signals:
            head += _pad("" if key is None else s.get(key, ""), width)
    body = bytearray()
    for r in range(nrec):
        for s in signals:
            body += np.asarray(s["data"][r * s["spr"]:(r + 1) * s["spr"]], "<i2").tobytes()
    with open(path, "wb") as f:
        f.write(head + bytes(body))
    return path


def eeg_signal(label, data, spr, pmin=-200.0, pmax=200.0, dmin=-2048, dmax=2047, dim="uV"):
    return {"label": label, "data": np.asarray(data, np.int16), "spr": spr, "pmin": pmin, "pmax": pmax, "dmin": dmin, "dmax": dmax, "dim": dim}


def write_edf_annotations(path, annots, startdate="01.01.89", starttime="22.00.00", record_bytes=None):
    """One-record EDF+C file whose only signal is 'EDF Annotations': the time-keeping entry, then one entry per (onset, duration, text)."""
    def num(v):
        return ("%+d" % v) if float(v) == int(v) else ("%+g" % v)
    tal = b"+0\x14\x14\x00"
    for onset, duration, text in annots:
        tal += num(onset).encode() + (b"\x15" + num(duration).encode()[1:] if duration is not None else b"") + b"\x14" + text.encode() + b"\x14\x00"
    n = record_bytes or (len(tal) + 1) // 2 * 2
    tal += b"\x00" * (n - len(tal))
    sig = {"label": "EDF Annotations", "data": np.frombuffer(tal, "<i2"), "spr": n // 2, "pmin": -1, "pmax": 1, "dmin": -32768, "dmax": 32767, "dim": ""}
    return write_edf(path, [sig], record_duration="0", n_records=1, startdate=startdate, starttime=starttime, reserved="EDF+C")


def write_profusion(path, codes, epoch_length=30):
    """An SHHS-style profusion XML; ScoredEvents comes first so that SleepStages is NOT the fifth child the reference indexes."""
    stages = "".join(f"<SleepStage>{int(c)}</SleepStage>" for c in codes)
    with open(path, "w") as f:
        f.write(f"<?xml version=\"1.0\"?><CMPStudyConfig><EpochLength>{epoch_length}</EpochLength><ScoredEvents></ScoredEvents>"
                f"<SleepStages>{stages}</SleepStages></CMPStudyConfig>")
    return path
