"""float64 numpy references of the two primitives of csrc/events.hip, the operation-count bound the filter is held to, and the sequential
definition of the run extraction.  Shared by tests/test_events_cpu.py and tests/test_gpu_events.py.

eegldm_fir_same.  The reference evaluates the definition in float64 FROM THE fp32 INPUTS (x and taps are the fp32 values handed to the call):

    c = (M - 1) / 2,   y[b][n] = sum_{k=0..M-1} taps[k] xe[b][n + k - c]
    edge 0: xe is zero outside [0, L);   edge 1: xe[-i] = x[i], xe[L-1+i] = x[L-1-i]
    mode 1: every sample enters as fl32(x * x), the stored value is sqrt(max(sum, 0)); a non-finite sum stays non-finite

Error bound (`fir_error_bound`), u = 2^-24, g(n) = n u / (1 - n u) (Higham, lemma 3.1), every term in float64 on the reference's values:

* plain: one fmaf chain of M steps from +0, one rounding per step:                   e = g(M) A,   A = sum_k |taps[k]| |xe|
  and a partial sum below 2^-126 may be flushed or rounded as a subnormal:           + M 2^-126
* rms: the reference squares in fp32 as the kernel does (x * x is one correctly rounded fp32 multiplication on both sides, so the staged
  values are THE SAME numbers: the square's rounding is part of the definition, not of the error); the issue's "one more rounding per
  square" is kept all the same, so that a kernel that fused the square into the chain would still pass:
                                                                                      e_S = (u + g(M) (1 + u)) A2 + M 2^-126,  A2 = sum_k |taps[k]| fl32(x^2)
  through the clamp (a contraction) and the square root, |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt(|a - b|)):
                                                                                      e_r = min(e_S / sqrt(S), sqrt(e_S))      (sqrt(e_S) where S <= 0)
  plus sqrtf's own error, SQRTF_ULPS = 1 ulp of the computed root (HIP documents 1 ulp for sqrtf; IEEE-correct rounding would be 0.5;
  tests/test_gpu_events.py measures it through the export with M = 1, taps = [1], mode = 1, which stores sqrtf(fl32(x * x)), and holds it to
  this figure); an ulp is at most 2 u of the value:                                  + 2 SQRTF_ULPS u (sqrt(max(S, 0)) + e_r) + 2^-126

eegldm_threshold_events.  `threshold_events` below is the definition itself, one sample at a time: integer logic on exact fp32 comparisons
plus a np.float32 running sum.  It is exact: the device result must equal it in every integer and every float bit.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
SQRTF_ULPS = 1.0
MAX_M, MAX_L, MAX_E = 2049, 4096, 64


def g(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------- FIR
def extend(x, c, edge):
    """(B, L) -> (B, L + 2 c): the rows extended by c samples on both sides."""
    x = np.asarray(x)
    B, L = x.shape
    if c == 0:
        return x.copy()
    if edge == 0:
        z = np.zeros((B, c), x.dtype)
        return np.concatenate([z, x, z], 1)
    assert c <= L - 1
    return np.concatenate([x[:, 1:c + 1][:, ::-1], x, x[:, L - 1 - c:L - 1][:, ::-1]], 1)


def _staged(x, mode):
    x32 = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return (x32 * x32 if mode else x32).astype(np.float64)       # x32 * x32: one fp32 rounding, as in the kernel


def _corr(xe, t, L):
    """sum_k t[k] xe[:, n + k] for n in [0, L), float64, row by row (np.correlate: the direct sum)."""
    with np.errstate(all="ignore"):
        return np.stack([np.correlate(r, t, "valid")[:L] for r in xe]) if len(xe) else np.zeros((0, L))


def _sum64(x, taps, edge, mode):
    t = np.asarray(taps, np.float32).astype(np.float64)
    return _corr(extend(_staged(x, mode), (len(t) - 1) // 2, edge), t, np.asarray(x).shape[1])


def fir64(x, taps, edge=0, mode=0):
    """The definition in float64 from the fp32 inputs: (B, L) float64."""
    y = _sum64(x, taps, edge, mode)
    if mode:
        with np.errstate(all="ignore"):
            y = np.where(y == -np.inf, np.nan, np.sqrt(np.maximum(y, 0.0)))          # np.maximum keeps a NaN; -inf (negative taps on an inf) stays non-finite
    return y


def fir_error_bound(x, taps, edge=0, mode=0):
    """E (B, L): |y_device - fir64| <= E elementwise for finite inputs."""
    t = np.abs(np.asarray(taps, np.float32).astype(np.float64))
    M = len(t)
    L = np.asarray(x).shape[1]
    A = _corr(extend(np.abs(_staged(x, mode)), (M - 1) // 2, edge), t, L)
    if not mode:
        return g(M) * A + M * TINY
    S = np.maximum(_sum64(x, taps, edge, 1), 0.0)
    e_s = (U + g(M) * (1.0 + U)) * A + M * TINY
    e_r = np.where(S > 0.0, np.minimum(e_s / np.sqrt(np.where(S > 0, S, 1.0)), np.sqrt(e_s)), np.sqrt(e_s))
    return e_r + 2.0 * SQRTF_ULPS * U * (np.sqrt(S) + e_r) + TINY


def support_mask(L, M, idx):
    """True at the outputs n whose support [n - c, n + c] holds sample idx (edge 0; with edge 1 the reflected copies count too: see
    `support_mask_reflect`)."""
    c = (M - 1) // 2
    n = np.arange(L)
    return np.abs(n - idx) <= c


def support_mask_reflect(L, M, idx):
    c = (M - 1) // 2
    pos = np.arange(-c, L + c)
    src = np.where(pos < 0, -pos, np.where(pos > L - 1, 2 * (L - 1) - pos, pos))
    hit = (src == idx).astype(np.int64)
    return np.convolve(hit, np.ones(M, np.int64), "valid") > 0


# ---------------------------------------------------------------------------------------------------- events
def close_mask(active, merge_gap):
    """Step 2 of the definition: inactive stretches strictly between two active samples, at most merge_gap long, become active."""
    a = np.asarray(active, bool).copy()
    idx = np.nonzero(a)[0]
    gap = np.diff(idx) - 1
    for k in np.nonzero((gap > 0) & (gap <= merge_gap))[0]:
        a[idx[k] + 1:idx[k + 1]] = True
    return a


def sequential_merge(active, merge_gap):
    """The same set by the left-to-right transitive merge of raw runs whose gaps are <= merge_gap: list of [start, stop, n_raw]."""
    a = np.asarray(active, bool)
    runs = []
    n, L = 0, len(a)
    while n < L:
        if a[n]:
            s = n
            while n < L and a[n]:
                n += 1
            if runs and s - runs[-1][1] <= merge_gap:
                runs[-1][1] = n; runs[-1][2] += 1
            else:
                runs.append([s, n, 1])
        else:
            n += 1
    return runs


def runs_of(mask):
    """[start, stop) of the maximal True runs of a boolean vector, from the differences (equal to sequential_merge(mask, -1))."""
    m = np.concatenate([[False], np.asarray(mask, bool), [False]])
    d = np.diff(m.astype(np.int8))
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


def run_features_loop(s, aux, start, stop):
    """(peak, argmax, sum, aux_max, aux_min) of the run [start, stop) of one row, one sample at a time: THE definition.  peak / aux_max / aux_min
    move only under a strict fp32 comparison from the value at `start`, so a NaN (possible inside a closed gap) never replaces them, the first of
    equal maxima wins, and a NaN at aux[start] stays; the sum is the np.float32 running sum from +0, so a NaN in the run makes it NaN."""
    peak, arg, tot = s[start], start, np.float32(0.0)
    amax = amin = np.float32(0.0) if aux is None else aux[start]
    with np.errstate(all="ignore"):
        for k in range(start, stop):
            v = s[k]
            tot = np.float32(tot + v)
            if v > peak:
                peak, arg = v, k
            if aux is not None:
                q = aux[k]
                if q > amax:
                    amax = q
                if q < amin:
                    amin = q
    return peak, arg, tot, amax, amin


def run_features(s, aux, start, stop):
    """`run_features_loop` in array form (tests/test_events_cpu.py holds the two equal bit for bit): np.argmax / np.argmin return the FIRST extreme
    and compare as the loop does once the NaNs are masked; np.cumsum in float32 is the sequential sum."""
    r = s[start:stop]
    with np.errstate(all="ignore"):
        arg = int(np.argmax(np.where(np.isnan(r), -np.inf, r)))
        tot = np.cumsum(np.concatenate([np.zeros(1, np.float32), r]), dtype=np.float32)[-1]
        amax = amin = np.float32(0.0)
        if aux is not None:
            q = aux[start:stop]
            if np.isnan(q[0]):
                amax = amin = q[0]
            else:
                amax = q[int(np.argmax(np.where(np.isnan(q), -np.inf, q)))]
                amin = q[int(np.argmin(np.where(np.isnan(q), np.inf, q)))]
    return r[arg], start + arg, tot, amax, amin


def threshold_events(s, thr, aux=None, min_len=1, max_len=MAX_L, merge_gap=0, drop_edge=False, max_events=32, counts=None, ev_i=None, ev_f=None):
    """The definition, row by row.  s (B, L) fp32, thr (B,) fp32, aux (B, L) fp32 or None.  Returns (counts (B, 2) int32, ev_i (B, E, 6) int32,
    ev_f (B, E, 4) fp32); the tables passed in are filled in place, so that untouched slots keep what they held."""
    s = np.asarray(s, np.float32); thr = np.asarray(thr, np.float32)
    B, L = s.shape
    E = int(max_events)
    counts = np.zeros((B, 2), np.int32) if counts is None else counts
    ev_i = np.zeros((B, E, 6), np.int32) if ev_i is None else ev_i
    ev_f = np.zeros((B, E, 4), np.float32) if ev_f is None else ev_f
    if aux is not None:
        aux = np.asarray(aux, np.float32)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            active = s[b] > thr[b]
        raw = runs_of(active)
        closed = close_mask(active, merge_gap)
        rawstart = np.zeros(L, bool)
        for r in raw:
            rawstart[r[0]] = True
        up = np.zeros(L, bool)
        if aux is not None:
            with np.errstate(invalid="ignore"):
                up[1:] = (aux[b, :-1] < 0) & (aux[b, 1:] >= 0)
        e = 0
        for start, stop in runs_of(closed):
            n = stop - start
            if not (min_len <= n <= max_len) or (drop_edge and (start == 0 or stop == L)):
                continue
            if e < E:
                peak, arg, tot, amax, amin = run_features(s[b], None if aux is None else aux[b], start, stop)
                ev_i[b, e] = (start, n, arg, int(up[start + 1:stop].sum()), int(rawstart[start:stop].sum()), (1 if start == 0 else 0) | (2 if stop == L else 0))
                ev_f[b, e] = (peak, tot, amax, amin)
            e += 1
        counts[b] = (e, len(raw))
    return counts, ev_i, ev_f


# ---------------------------------------------------------------------------------------------------- planted events (pipeline tests)
PLANT_B, PLANT_L, PLANT_SFREQ, PLANT_SEEDS = 16, 3000, 100.0, (0, 1, 2, 3, 4)
SPINDLE_FACTOR = 3.0              # envelope_threshold factor of the planted-spindle test: 1.5 leaves 1 to 5 noise events per seed
SW_AMP, SW_NEG_S, SW_POS_S = 5.0, 0.6, 0.5


def lowpass_noise(seed, taps):
    """(PLANT_B, PLANT_L) float32: white Gaussian noise of unit variance passed through `taps` (float64, no edge: the valid part of a longer draw)."""
    r = np.random.default_rng(seed)
    white = r.standard_normal((PLANT_B, PLANT_L + len(taps) - 1))
    return np.stack([np.correlate(row, taps, "valid") for row in white]).astype(np.float32), r


def planted_spindles(seed, taps):
    """(noise, planted, bursts): `planted` = noise + three bursts 3 cos^2(pi (t - c0) / d) sin(2 pi f t) on |t - c0| < d / 2 per window, c0 = 5 + 8 k +- 1 s,
    d in [0.8, 1.6] s, f in [12, 15] Hz; bursts[b][k] = (c0, d, f)."""
    noise, r = lowpass_noise(seed, taps)
    t = np.arange(PLANT_L) / PLANT_SFREQ
    x = noise.astype(np.float64)
    bursts = np.zeros((PLANT_B, 3, 3))
    for b in range(PLANT_B):
        for k in range(3):
            c0, d, f = 5.0 + 8.0 * k + r.uniform(-1.0, 1.0), r.uniform(0.8, 1.6), r.uniform(12.0, 15.0)
            on = np.abs(t - c0) < 0.5 * d
            x[b, on] += 3.0 * np.cos(np.pi * (t[on] - c0) / d) ** 2 * np.sin(2.0 * np.pi * f * t[on])
            bursts[b, k] = (c0, d, f)
    return noise, x.astype(np.float32), bursts


def planted_slow_waves(seed, taps):
    """(noise, planted, t0): one negative half-sine of SW_NEG_S followed by a positive one of SW_POS_S, amplitude SW_AMP, three per window starting at
    t0[b][k] = 4 + 8 k +- 1 s."""
    noise, r = lowpass_noise(seed, taps)
    t = np.arange(PLANT_L) / PLANT_SFREQ
    x = noise.astype(np.float64)
    t0 = np.zeros((PLANT_B, 3))
    for b in range(PLANT_B):
        for k in range(3):
            a = 4.0 + 8.0 * k + r.uniform(-1.0, 1.0)
            neg = (t >= a) & (t < a + SW_NEG_S); pos = (t >= a + SW_NEG_S) & (t < a + SW_NEG_S + SW_POS_S)
            x[b, neg] -= SW_AMP * np.sin(np.pi * (t[neg] - a) / SW_NEG_S)
            x[b, pos] += SW_AMP * np.sin(np.pi * (t[pos] - a - SW_NEG_S) / SW_POS_S)
            t0[b, k] = a
    return noise, x.astype(np.float32), t0


def spindles64(x, thr, band_taps, box, min_len, max_len, merge_gap, drop_edge, max_events=32):
    """The spindle detector restated on the references: float64 filters from fp32 inputs (rounded to fp32 between the stages), the exact run logic."""
    band = fir64(x, band_taps, 1, 0).astype(np.float32)
    env = fir64(band, box, 1, 1).astype(np.float32)
    return band, env, threshold_events(env, np.full(len(x), thr, np.float32), aux=band, min_len=min_len, max_len=max_len, merge_gap=merge_gap,
                                       drop_edge=drop_edge, max_events=max_events)


def match_planted(mid_s, window, centres, tol_s):
    """(found, extra): planted events (b, k) with a detected midpoint within tol_s of centres[b][k], and detected events that match none."""
    found = np.zeros(centres.shape, bool)
    used = np.zeros(len(mid_s), bool)
    for i, (w, m) in enumerate(zip(window, mid_s)):
        hit = np.abs(centres[int(w)] - m) <= tol_s
        found[int(w)] |= hit
        used[i] = hit.any()
    return found, int((~used).sum())
