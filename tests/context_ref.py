"""numpy restatement of the context-mask draw (include/eegldm.h: eegldm_context_mask), bit for bit: Philox4x32-10 keyed by `seed` at counter
offset + b, word 0 as a float32 against the probabilities, the ranges from 64-bit products of 32-bit words.  Shared by tests/test_context_cpu.py
and tests/test_gpu_context.py."""
import numpy as np

_M0, _M1, _W0, _W1, _LO = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
_S32 = np.uint64(32)
NONE, PREFIX, SPAN = 0, 1, 2


def philox4x32(seed, ctr):
    """ctr: uint64 array -> four uint64 arrays holding the 32-bit words of Philox4x32-10(key = seed, counter = (ctr, 0))."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    c0, c1 = ctr & _LO, ctr >> _S32
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = seed & _LO, seed >> _S32
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def check_draw(L, p_none, p_prefix, span_min, span_max):
    """The refusals of the library, as ValueError."""
    if not (0.0 <= p_none <= 1.0 and 0.0 <= p_prefix <= 1.0):
        raise ValueError("a probability outside [0, 1]")
    if np.float32(p_none) + np.float32(p_prefix) > np.float32(1.0):
        raise ValueError("p_none + p_prefix > 1")
    if span_min < 1 or span_max < span_min or span_max > L:
        raise ValueError("span range")


def draw_intervals(B, L, p_none, p_prefix, span_min, span_max, seed, offset):
    """-> (kind (B,), r0 (B,), r1 (B,)): sample b regenerates [r0, r1) and keeps the rest."""
    check_draw(L, p_none, p_prefix, span_min, span_max)
    with np.errstate(over="ignore"):
        ctr = np.uint64(int(offset) & 0xFFFFFFFFFFFFFFFF) + np.arange(B, dtype=np.uint64)
    w0, w1, w2, _w3 = philox4x32(seed, ctr)
    u0 = w0.astype(np.float32) * np.float32(2.3283064365386963e-10)
    pn = np.float32(p_none); ps = np.float32(p_none) + np.float32(p_prefix)
    kind = np.where(u0 < pn, NONE, np.where(u0 < ps, PREFIX, SPAN))
    s = (np.uint64(1) + ((w1 * np.uint64(L - 1)) >> _S32)).astype(np.int64) if L > 1 else np.zeros(B, np.int64)
    ln = np.int64(span_min) + ((w1 * np.uint64(span_max - span_min + 1)) >> _S32).astype(np.int64)
    start = ((w2 * (np.uint64(L + 1) - ln.astype(np.uint64))) >> _S32).astype(np.int64)
    r0 = np.where(kind == NONE, 0, np.where(kind == PREFIX, s, start))
    r1 = np.where(kind == SPAN, start + ln, L)
    return kind, r0, r1


def draw_mask(B, L, p_none, p_prefix, span_min, span_max, seed, offset):
    """-> float32 (B, L): 1 = keep, 0 = regenerate."""
    _kind, r0, r1 = draw_intervals(B, L, p_none, p_prefix, span_min, span_max, seed, offset)
    pos = np.arange(L)[None, :]
    return np.where((pos >= r0[:, None]) & (pos < r1[:, None]), 0.0, 1.0).astype(np.float32)
