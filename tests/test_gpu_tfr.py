"""-m gpu: the two primitives of csrc/tfr.hip and the layer built on them.  eegldm_stft_power against a float64 evaluation of its definition
within the operation-by-operation bound of tests/tfr_reference.py and against numpy's single-precision rfft (at most 8 times its error), its
bit-exact anchors (zeros, repeat runs, row, batch, frame-position and launch independence, bands-only equal to the fold of a full call, bin
sub-ranges, no-ops, non-finite samples, refusals); eegldm_pac_intervals within its float64 bound, its skipped samples, out-of-range intervals
and interval independence; the planted spindle / slow-oscillation coupling; the spectrogram helpers and the entry script."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest
import torch

import tfr_reference as R

pytestmark = pytest.mark.gpu
FILL = 7.0e30


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t = time.time()
    yield
    print(f"\n[numerics] tfr: wall time of tests/test_gpu_tfr.py {time.time() - t:.1f} s")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _carve(a, ld, off, fill=FILL):
    """Rows of `a` on the device with row stride ld (>= L), starting `off` floats into an allocation filled with `fill`."""
    n, d = a.shape
    buf = torch.full((off + n * ld + 4,), fill, device="cuda")
    view = buf[off:off + n * ld].view(n, ld)[:, :d]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    return buf, view


def _out(n, off):
    buf = torch.full((off + n + 4,), FILL, device="cuda")
    return buf, buf[off:off + n]


def _at(buf, off):
    """The address `off` elements into buf (an empty view has no data_ptr of its own)."""
    return None if buf is None else C.c_void_p(buf.data_ptr() + off * buf.element_size())


def _gutters_intact(buf, off, n):
    g = buf.cpu().numpy()
    return bool(np.all(g[:off] == np.float32(FILL)) and np.all(g[off + n:] == np.float32(FILL)))


def _stft(x, tp, w2=None, n_fft=256, hop=50, centre=1, edge=1, detrend=1, onesided=1, scale=1.0, bins="all", bands=None, ld=None, offs=(0, 0, 0, 0),
          expect_rc=0):
    """(power (B, F, k1 - k0) or None, bands (B, F, NB) or None) as fp32 numpy, through carved buffers; bins None: no spectrogram."""
    import gpu_util as G
    x = np.asarray(x, np.float32)
    tp = np.atleast_2d(np.asarray(tp, np.float32))
    B, L = x.shape
    K, n_win = tp.shape
    w2 = np.ones(K, np.float32) if w2 is None else np.asarray(w2, np.float32)
    ld = L if ld is None else ld
    _xb, xv = _carve(x, ld, offs[0])
    _tb, tv = _out(K * n_win, offs[1])
    tv.copy_(torch.from_numpy(tp.reshape(-1)))
    F = max(R.num_frames(L, n_win, hop, centre), 0)
    nbin = n_fft // 2 + 1
    k0, k1 = (0, nbin) if isinstance(bins, str) else (bins if bins is not None else (0, 0))
    pbuf = pv = bbuf = bv = None
    if bins is not None:
        pbuf, pv = _out(B * F * (k1 - k0), offs[2])
    nb = 0 if bands is None else len(bands)
    if nb:
        bbuf, bv = _out(B * F * nb, offs[3])
    bh = (C.c_int * max(2 * nb, 1))(*([int(v) for r in bands for v in r] if nb else [0]))
    rc = G.lib.eegldm_stft_power(G.ctx().h, G.ptr(xv), ld, B, L, G.ptr(tv), (C.c_float * K)(*w2.tolist()), K, n_win, n_fft, hop, centre, edge, detrend,
                                 onesided, float(scale), k0, k1, _at(pbuf, offs[2]), bh if nb else None, nb, _at(bbuf, offs[3]))
    torch.cuda.synchronize()
    assert (rc == 0) == (expect_rc == 0), (rc, G.lib.eegldm_last_error())
    if pbuf is not None:
        assert _gutters_intact(pbuf, offs[2], B * F * (k1 - k0)), "a write outside power"
    if bbuf is not None:
        assert _gutters_intact(bbuf, offs[3], B * F * nb), "a write outside bands"
    power = None if pv is None else pv.cpu().numpy().reshape(B, F, k1 - k0).copy()
    bsum = None if bv is None else bv.cpu().numpy().reshape(B, F, nb).copy()
    return power, bsum


def _tapers(rng, K, n_win):
    """K taper look-alikes with both signs, fp32, of roughly unit energy."""
    n = np.arange(n_win)
    t = np.stack([np.sin(np.pi * (k + 1) * (n + 0.5) / n_win) for k in range(K)]) * (1.0 + 0.1 * rng.standard_normal((K, n_win)))
    return (t / np.sqrt(np.sum(t * t, axis=1, keepdims=True))).astype(np.float32)


def _band_sets(nbin, which):
    if which == 1:
        return [(nbin // 3, 2 * nbin // 3)]
    edges = np.linspace(0, nbin, 9).astype(int)
    touching = [(int(edges[i]), int(edges[i + 1])) for i in range(8)]
    return touching + [(0, nbin), (1, nbin - 1), (3, 17), (10, 12), (0, 1), (nbin - 1, nbin), (5, 6), (nbin // 2, nbin // 2 + 1)]     # 16: overlapping, one-bin


# ------------------------------------------------------------------------------------------------ 1. STFT against float64 and the yardstick
HOPS = lambda n_win: (1, 7, n_win, n_win + 3)
NWINS = lambda n_fft: (1, 2, min(200, n_fft - 2), n_fft - 1, n_fft)         # 200 where the transform holds it
LS = lambda n_win: (1, max(n_win - 1, 1), n_win, n_win + 1, 3000, 3072, 10007)
KS, BS, MAGS, NBS = (1, 2, 3, 8), (1, 5, 130), (1e-3, 1.0, 1e3), (1, 16)
REF_BUDGET = 2.5e6          # B F K n_fft of one float64 reference: the batch, then L, then the centring give way where a case is large


@pytest.mark.parametrize("n_fft", R.NFFT)
def test_stft_against_float64(n_fft):
    """|P - P64| <= E_P and |bands - bands64| <= E_band elementwise over n_win, hop, L, centre, edge, detrend (row means of 0 and 30 sd), K, bin
    ranges, band sets, B, magnitudes, row strides above L and every pointer 0..3 floats off an allocation filled with 7e30."""
    rng = np.random.default_rng(n_fft)
    nbin = n_fft // 2 + 1
    n = 0
    worst_p = worst_b = 0.0
    seen = set()
    for n_win in NWINS(n_fft):
        for hop in HOPS(n_win):
            for rep in range(2):
                n += 1
                K, B, mag = KS[n % 4], BS[n % 3], MAGS[(n // 3) % 3]
                centre, edge, detrend = (n >> 1) & 1, n & 1, (n >> 2) & 1
                ls = LS(n_win)
                L = ls[(n + rep * 3) % 7]
                work = lambda B_, L_, c_: B_ * max(R.num_frames(L_, n_win, hop, c_), 0) * K * n_fft
                if work(B, L, centre) > REF_BUDGET:
                    B = 1
                for cand in (L,) + tuple(sorted(ls, reverse=True)):
                    if work(B, cand, centre) <= REF_BUDGET:
                        L = cand
                        break
                else:
                    centre, L = 0, n_win + 1
                if centre and edge and n_win // 2 > L - 1:
                    edge = 0
                bins = ("all", (n % nbin, n % nbin + 1), (0, 1), (nbin - 1, nbin), None)[n % 5]
                nb = NBS[n % 2] if bins is not None or n % 2 else 16
                bands = _band_sets(nbin, nb) if (n % 3 or bins is None) else None
                if bins is None and bands is None:
                    bins = "all"
                mean = 30.0 * mag if (n >> 3) & 1 else 0.0
                x = (rng.standard_normal((B, L)) * mag + mean).astype(np.float32)
                tp = _tapers(rng, K, n_win)
                w2 = rng.uniform(0.5, 1.0, K).astype(np.float32)
                scale = np.float32((0.01, 1.0, 3.0)[n % 3])
                onesided = (n >> 4) & 1
                got_p, got_b = _stft(x, tp, w2, n_fft, hop, centre, edge, detrend, onesided, scale, bins, bands, ld=L + n % 3,
                                     offs=(n % 4, (n // 4) % 4, (n // 2) % 4, (n // 8) % 4))
                P, E = R.stft_error_bound(x, tp, w2, n_fft, hop, centre, edge, detrend, scale, onesided)
                tag = f"n_fft={n_fft} n_win={n_win} hop={hop} L={L} B={B} K={K} centre={centre} edge={edge} detrend={detrend} mag={mag} mean={mean} bins={bins}"
                if got_p is not None:
                    k0, k1 = (0, nbin) if bins == "all" else bins
                    assert got_p.shape == P[:, :, k0:k1].shape and np.all(np.isfinite(got_p)), tag
                    err = np.abs(got_p.astype(np.float64) - P[:, :, k0:k1])
                    assert np.all(err <= E[:, :, k0:k1]), f"{tag}: power off by {err.max():.3e}"
                    if err.size:
                        worst_p = max(worst_p, float((err / E[:, :, k0:k1]).max()))
                if got_b is not None:
                    want, Eb = R.bands64(P, bands), R.bands_error_bound(P, E, bands)
                    assert got_b.shape == want.shape and np.all(np.isfinite(got_b)), tag
                    err = np.abs(got_b.astype(np.float64) - want)
                    assert np.all(err <= Eb), f"{tag}: bands off by {err.max():.3e}"
                    if err.size:
                        worst_b = max(worst_b, float((err / Eb).max()))
                seen.update({("K", K), ("B", B), ("mag", mag), ("centre", centre), ("edge", edge), ("detrend", detrend), ("L", ls.index(L)), ("nb", nb if bands else 0),
                             ("bins", n % 5), ("mean", mean > 0), ("F>0", P.shape[1] > 0)})
    for key, vals in (("K", KS), ("mag", MAGS), ("centre", (0, 1)), ("edge", (0, 1)), ("detrend", (0, 1)), ("nb", NBS), ("bins", range(5)), ("mean", (False, True))):
        assert all((key, v) in seen for v in vals), (key, sorted(s for s in seen if s[0] == key))
    assert ("B", 1) in seen and ("B", 5) in seen and (n_fft > 256 or ("B", 130) in seen) and len({s for s in seen if s[0] == "L"}) >= 4
    print(f"[numerics] tfr n_fft={n_fft}: {n} calls, worst error / bound: power {worst_p:.4f}, bands {worst_b:.4f} (C = {R.fft_constant(n_fft):.0f})")


def test_stft_long_row():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, 300000)).astype(np.float32)
    tp = _tapers(rng, 3, 200)
    bands = _band_sets(129, 16)
    got_p, got_b = _stft(x, tp, None, 256, 100, 1, 1, 1, 1, 0.01, "all", bands, ld=300001, offs=(1, 2, 3, 1))
    P, E = R.stft_error_bound(x, tp, np.ones(3), 256, 100, 1, 1, 1, 0.01, 1)
    assert got_p.shape == (1, 3000, 129) and np.all(np.abs(got_p - P) <= E) and np.all(np.abs(got_b - R.bands64(P, bands)) <= R.bands_error_bound(P, E, bands))
    only_b = _stft(x, tp, None, 256, 100, 1, 1, 1, 1, 0.01, None, bands)[1]
    assert np.array_equal(_bits(only_b), _bits(got_b)) and np.array_equal(_bits(got_b), _bits(R.fold_bands32(got_p, bands)))


@pytest.mark.parametrize("n_fft", R.NFFT)
def test_stft_against_single_precision_rfft(n_fft):
    """Per frame, the RMS over the bins of |P_device - P_64| is at most 8 times that of numpy's complex64 rfft of the same float32 frame
    (K = 1, scale = 1, two-sided, no detrend: the device's v is fl32(taper xe), the yardstick's input)."""
    rng = np.random.default_rng(1000 + n_fft)
    ratios = []
    for i, n_win in enumerate(NWINS(n_fft)):
        hop = max(n_win // 2, n_fft // 8) + 3
        L = max(3000, 3 * n_fft)
        x = (rng.standard_normal((2, L)) * MAGS[i % 3]).astype(np.float32)
        tp = _tapers(rng, 1, n_win)
        centre, edge = i & 1, (i >> 1) & 1
        got = _stft(x, tp, None, n_fft, hop, centre, edge, 0, 0, 1.0)[0]
        dev, yard = R.yardstick_errors(got, x, tp, n_fft, hop, centre, edge)
        assert dev.size >= 4
        bad = dev > R.YARDSTICK_FACTOR * yard
        both = yard > 0
        ratios.append((n_win, float(np.max(dev[both] / yard[both])) if both.any() else 0.0, float(np.median(dev[both] / yard[both])) if both.any() else 0.0))
        print(f"[numerics] tfr n_fft={n_fft} n_win={n_win}: device / complex64 rfft error per frame: max {ratios[-1][1]:.3f}, median {ratios[-1][2]:.3f} ({dev.size} frames)")
        assert not bad.any(), f"n_fft={n_fft} n_win={n_win}: {int(bad.sum())} of {bad.size} frames above {R.YARDSTICK_FACTOR} x the complex64 rfft, worst {ratios[-1][1]:.3f}"


# ------------------------------------------------------------------------------------------------ 2. bit-exact anchors
def test_stft_zeros_repeats_rows_and_positions():
    rng = np.random.default_rng(11)
    tp = _tapers(rng, 3, 200)
    bands = _band_sets(129, 16)
    z_p, z_b = _stft(np.zeros((3, 1000), np.float32), tp, None, 256, 50, bands=bands)
    assert np.all(z_p == 0.0) and np.all(z_b == 0.0)
    x = rng.standard_normal((130, 1000)).astype(np.float32) + 3.0
    a_p, a_b = _stft(x, tp, [1.0, 0.5, 0.25], 256, 50, scale=0.37, bands=bands)
    b_p, b_b = _stft(x, tp, [1.0, 0.5, 0.25], 256, 50, scale=0.37, bands=bands, ld=1003, offs=(1, 2, 3, 1))
    assert np.array_equal(_bits(a_p), _bits(b_p)) and np.array_equal(_bits(a_b), _bits(b_b)), "run != run"
    r_p, r_b = _stft(x[77:78], tp, [1.0, 0.5, 0.25], 256, 50, scale=0.37, bands=bands)
    assert np.array_equal(_bits(r_p[0]), _bits(a_p[77])) and np.array_equal(_bits(r_b[0]), _bits(a_b[77])), "a row alone != the row in a batch of 130"
    # bands-only == the ascending fp32 fold of the full call == the bands of the call that writes both; bin sub-ranges are slices
    only_b = _stft(x, tp, [1.0, 0.5, 0.25], 256, 50, scale=0.37, bins=None, bands=bands)[1]
    assert np.array_equal(_bits(only_b), _bits(a_b)) and np.array_equal(_bits(a_b), _bits(R.fold_bands32(a_p, bands)))
    for k0, k1 in ((0, 1), (128, 129), (17, 18), (5, 77), (1, 129)):
        sub = _stft(x[:5], tp, [1.0, 0.5, 0.25], 256, 50, scale=0.37, bins=(k0, k1))[0]
        assert np.array_equal(_bits(sub), _bits(a_p[:5, :, k0:k1])), (k0, k1)
    # the same n_win samples: frame 0 of a short row, an interior frame of a long row, another row, other hops (other frames per workgroup)
    seg = rng.standard_normal(200).astype(np.float32) * 2.0 + 1.0
    s_p, s_b = _stft(seg[None], tp, None, 256, 50, centre=0, bands=bands)
    assert s_p.shape == (1, 1, 129)
    for hop, L, at in ((50, 3000, 1000), (1, 700, 333), (7, 5000, 7 * 300), (203, 10007, 203 * 31)):
        long = rng.standard_normal((5, L)).astype(np.float32)
        long[3, at:at + 200] = seg
        l_p, l_b = _stft(long, tp, None, 256, hop, centre=0, bands=bands)
        assert np.array_equal(_bits(l_p[3, at // hop]), _bits(s_p[0, 0])) and np.array_equal(_bits(l_b[3, at // hop]), _bits(s_b[0, 0])), (hop, L)
    c_p = _stft(np.concatenate([np.zeros(100, np.float32), seg, np.zeros(100, np.float32)])[None], tp, None, 256, 100, centre=1, edge=0)[0]
    assert np.array_equal(_bits(c_p[0, 2]), _bits(s_p[0, 0])), "centred frame 2 covers [100, 300)"


def test_stft_noops_and_refusals_leave_outputs_untouched():
    rng = np.random.default_rng(12)
    tp = _tapers(rng, 2, 200)
    x = rng.standard_normal((2, 199)).astype(np.float32)
    p, b = _stft(x, tp, None, 256, 50, centre=0, bands=[(0, 5)])                       # F == 0: _stft checks that the whole allocation kept its fill
    assert p.shape == (2, 0, 129) and b.shape == (2, 0, 1)
    import gpu_util as G
    xd = torch.from_numpy(rng.standard_normal((2, 1000)).astype(np.float32)).cuda()
    td = torch.from_numpy(tp).cuda()
    pw = torch.full((2 * 20 * 129,), FILL, device="cuda"); bd = torch.full((2 * 20 * 2,), FILL, device="cuda")
    w2 = (C.c_float * 2)(1.0, 1.0)
    bh = (C.c_int * 4)(0, 5, 5, 9)

    def call(x=xd, ldx=1000, B=2, L=1000, K=2, n_win=200, n_fft=256, hop=50, centre=1, edge=1, k0=0, k1=129, power=pw, bh=bh, NB=2, bands=bd, w2=w2):
        return G.lib.eegldm_stft_power(G.ctx().h, G.ptr(x), ldx, B, L, G.ptr(td), w2, K, n_win, n_fft, hop, centre, edge, 1, 1, 1.0, k0, k1, G.ptr(power), bh, NB,
                                       G.ptr(bands))

    for kw in (dict(n_fft=200), dict(n_win=257), dict(hop=0), dict(K=9), dict(NB=17), dict(k1=130), dict(bh=(C.c_int * 4)(0, 5, 9, 5)), dict(ldx=999),
               dict(L=100, ldx=1000), dict(power=None, bands=None), dict(w2=(C.c_float * 2)(1.0, -1.0)), dict(B=0), dict(L=0)):
        rc = call(**kw)
        torch.cuda.synchronize()
        assert (rc == 0) == (kw.keys() <= {"B"} or kw == dict(L=0)), kw
        assert bool((pw == FILL).all()) and bool((bd == FILL).all()), kw
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((pw != FILL).all()) and bool((bd != FILL).all())


@pytest.mark.parametrize("centre,edge,detrend,zero_tap", [(1, 1, 1, False), (1, 0, 0, False), (0, 0, 0, True), (1, 1, 0, True)])
def test_stft_non_finite_samples_poison_exactly_their_frames(centre, edge, detrend, zero_tap):
    rng = np.random.default_rng(13)
    L, n_win, hop, n_fft = 700, 200, 50, 256
    tp = _tapers(rng, 3, n_win)
    if zero_tap:
        tp[:, 57] = 0.0                   # a sample under a stored zero taper value still poisons its frame (0 * inf)
    x = rng.standard_normal((2, L)).astype(np.float32)
    bands = [(0, 129), (7, 8)]
    base_p, base_b = _stft(x, tp, None, n_fft, hop, centre, edge, detrend, bands=bands)
    for val in (np.inf, -np.inf, np.nan):
        for idx in (0, 57 + 3 * hop, 333, L - 1):
            y = x.copy(); y[0, idx] = val
            p, b = _stft(y, tp, None, n_fft, hop, centre, edge, detrend, bands=bands)
            hit = R.poisoned_frames(L, n_win, hop, centre, edge, idx)
            assert hit.any() or (centre == 0 and idx == L - 1 and (L - n_win) % hop), (idx,)
            assert not np.isfinite(p[0, hit]).any() and not np.isfinite(b[0, hit]).any(), (val, idx)
            assert np.array_equal(_bits(p[0, ~hit]), _bits(base_p[0, ~hit])) and np.array_equal(_bits(b[0, ~hit]), _bits(base_b[0, ~hit])), (val, idx)
            assert np.array_equal(_bits(p[1]), _bits(base_p[1])) and np.array_equal(_bits(b[1]), _bits(base_b[1])), (val, idx)


# ------------------------------------------------------------------------------------------------ 3. phase-amplitude sums
def _pac(pr, pi, am, iv=None, ld=None, offs=(0, 0, 0, 0), out_off=0, NI=None):
    import gpu_util as G
    B, L = pr.shape
    ld = L if ld is None else ld
    views = [_carve(np.asarray(t, np.float32), ld + i, offs[i])[1] for i, t in enumerate((pr, pi, am))]
    ivd = None
    if iv is not None:
        ivb = torch.zeros(offs[3] + 3 * len(iv) + 1, dtype=torch.int32, device="cuda")
        ivd = ivb[offs[3]:offs[3] + 3 * len(iv)]
        ivd.copy_(torch.from_numpy(np.asarray(iv, np.int32).reshape(-1)))
    ni = (B if iv is None else len(iv)) if NI is None else NI
    obuf = torch.full((out_off + 4 * ni + 2,), FILL, dtype=torch.float64, device="cuda")
    ov = obuf[out_off:out_off + 4 * ni]
    G.check(G.lib.eegldm_pac_intervals(G.ctx().h, G.ptr(views[0]), ld, G.ptr(views[1]), ld + 1, G.ptr(views[2]), ld + 2, B, L, G.ptr(ivd), ni, G.ptr(ov)))
    torch.cuda.synchronize()
    g = obuf.cpu().numpy()
    assert np.all(g[:out_off] == FILL) and np.all(g[out_off + 4 * ni:] == FILL), "a write outside out"
    return ov.cpu().numpy().reshape(ni, 4).copy()


def test_pac_against_float64():
    rng = np.random.default_rng(21)
    n, worst = 0, 0.0
    for L in (1, 63, 64, 65, 3000):
        for B in (1, 5, 130):
            n += 1
            pr, pi = (rng.standard_normal((B, L)).astype(np.float32) * (1e-3, 1.0, 1e3)[n % 3] for _ in range(2))
            am = np.abs(rng.standard_normal((B, L))).astype(np.float32) * (1e3, 1.0, 1e-3)[n % 3]
            if L >= 63:                       # skipped samples: a NaN or inf in each input, and h == 0
                for r in range(B):
                    pr[r, (3 + r) % L] = np.nan; pi[r, (9 + r) % L] = np.inf; am[r, (17 + r) % L] = -np.inf; am[r, (23 + r) % L] = np.nan
                    pr[r, (31 + r) % L] = 0.0; pi[r, (31 + r) % L] = 0.0
            lens = sorted({1, min(64, L), min(65, L), L})
            iv = [(r % B, (s * 7) % (L - ln + 1), ln) for r in range(B) for s, ln in enumerate(lens)]
            iv += [(B, 0, 1), (-1, 0, 1), (0, -1, 2), (0, 0, 0), (0, 0, -5), (0, L - 1, 2), (0, 0, L + 1), (0, L, 1)]
            for ivs, off in ((iv, n % 4), (None, 0)):
                got = _pac(pr, pi, am, ivs, ld=L + n % 3, offs=(n % 4, (n + 1) % 4, (n + 2) % 4, off), out_off=n % 2)
                want, E = R.pac64(pr, pi, am, ivs), R.pac_error_bound(pr, pi, am, ivs)
                assert np.array_equal(got[:, 0], want[:, 0]), (L, B, "n must be exact")
                assert np.all(np.abs(got - want) <= E), (L, B, float(np.max(np.abs(got - want) - E)))
                worst = max(worst, float(np.max(np.abs(got - want)[:, 1:] / np.where(E[:, 1:] > 0, E[:, 1:], 1.0))))
                if ivs is not None:
                    assert np.array_equal(got[-8:], np.tile([-1.0, 0.0, 0.0, 0.0], (8, 1))), "out-of-range intervals"
                    if L >= 63:
                        whole = [q for q, v in enumerate(ivs[:-8]) if v[2] == L]
                        assert np.all(got[whole, 0] == L - 5)
    print(f"[numerics] tfr pac: {n} shapes, worst error / bound {worst:.4f}")


def test_pac_interval_independence_and_constant_phase():
    rng = np.random.default_rng(22)
    B, L = 7, 3000
    pr, pi = (rng.standard_normal((B, L)).astype(np.float32) for _ in range(2))
    am = np.abs(rng.standard_normal((B, L))).astype(np.float32)
    iv = [(int(rng.integers(B)), int(s), int(ln)) for s, ln in zip(rng.integers(0, 2000, 500), rng.integers(1, 1000, 500))]
    many = _pac(pr, pi, am, iv)
    for q in (0, 123, 499):
        assert np.array_equal(_pac(pr, pi, am, [iv[q]]).view(np.int64), many[q:q + 1].view(np.int64)), "an interval alone != the same interval among 500"
    assert np.array_equal(_pac(pr, pi, am, iv).view(np.int64), many.view(np.int64)), "run != run"
    from eegldm import metrics as M
    # a constant phase: mvl == 1.  On an axis every term is exact (a * 1 / 1), so sum a pr / h repeats sum a bit for bit: 4 x 2^-53 as the
    # issue sets it.  Off the axes the terms round (3/5 is no float64) and the two sums drift apart by their chains: the derived
    # (ceil(len / 64) + 6 + 6) 2^-53 of tfr_reference.pac_error_bound, twice (numerator and denominator).
    for (re, im), tol in (((1.0, 0.0), 4), ((0.0, -2.0), 4), ((-0.5, 0.0), 4), ((3.0, 4.0), 2 * (47 + 12)), ((-1.0, 1.0), 2 * (47 + 12))):
        r = M.pac_from_out(_pac(np.full((B, L), re, np.float32), np.full((B, L), im, np.float32), am))
        assert np.all(np.abs(r["mvl"] - 1.0) <= tol * R.V), ((re, im), float(np.max(np.abs(r["mvl"] - 1.0))) / R.V)
        assert np.all(np.abs(np.angle(np.exp(1j * (r["phase"] - np.arctan2(im, re))))) <= 1e-13) and np.all(r["n"] == L)
    short = M.pac_from_out(_pac(np.full((B, L), 3.0, np.float32), np.full((B, L), 4.0, np.float32), am, [(2, 100, 64), (3, 7, 1)]))
    assert np.all(np.abs(short["mvl"] - 1.0) <= 2 * 13 * R.V)
    # the Python layer: same numbers, intervals and whole rows
    py = M.phase_amplitude_coupling(torch.from_numpy(pr), torch.from_numpy(pi), torch.from_numpy(am), np.asarray(iv[:20]))
    want = M.pac_from_out(many[:20])
    assert np.array_equal(py["n"], want["n"]) and np.array_equal(py["mvl"], want["mvl"]) and np.array_equal(py["phase"], want["phase"])
    rows = M.phase_amplitude_coupling(torch.from_numpy(pr)[:, None], torch.from_numpy(pi), torch.from_numpy(am))
    assert np.array_equal(rows["sum_a"], _pac(pr, pi, am)[:, 1])


# ------------------------------------------------------------------------------------------------ 4. planted coupling
def _planted_device(seed, theta):
    from eegldm import metrics as M
    x, centres = R.planted_windows(seed, theta)
    table = {"window": np.repeat(np.arange(x.shape[0]), 3), "argmax": centres.reshape(-1)}
    return x, M.spindle_so_coupling(torch.from_numpy(x), table, so_band=(0.4, 1.25), so_trans_hz=0.6, sigma_band=(11.0, 16.0), sigma_trans_hz=2.0, half_s=0.5)


@pytest.mark.parametrize("seed", range(5))
def test_planted_coupling(seed):
    for theta in (0.0, 2.0):
        _x, res = _planted_device(seed, theta)
        assert res["n_events"] == 48 and res["n_dropped"] == 0
        for key in ("peak_phase_stats", "preferred_phase_stats"):
            s = res[key]
            print(f"[numerics] tfr planted seed={seed} theta={theta} {key}: mean {s['mean']:.4f} R {s['R']:.4f}")
            assert s["n"] == 48 and R.circ_dist(s["mean"], theta) <= 0.1 and s["R"] >= 0.95 and s["p"] < 1e-6, (seed, theta, key, s)
        assert np.all((res["mvl"] > 0.0) & (res["mvl"] <= 1.0))
    _x, res = _planted_device(seed, None)
    for key in ("peak_phase_stats", "preferred_phase_stats"):
        assert res[key]["R"] <= 0.5, (seed, key, res[key])


def test_planted_coupling_through_the_detector():
    """The full path: detect_spindles on the planted windows (threshold from the windows themselves), then spindle_so_coupling."""
    from eegldm import metrics as M
    x, centres = R.planted_windows(0, 0.0)
    w = torch.from_numpy(x)
    thr = M.envelope_threshold(w, factor=1.5)
    table = M.detect_spindles(w, thr)
    near = [np.min(np.abs(centres[wi] - a)) for wi, a in zip(table["window"], table["argmax"])]
    print(f"[numerics] tfr planted detector: {len(near)} spindles detected for 48 planted, {int(np.sum(np.asarray(near) <= 15))} within 0.15 s of a planted centre")
    assert len(near) >= 40 and np.sum(np.asarray(near) <= 15) >= 40
    res = M.spindle_so_coupling(w, table, so_band=(0.4, 1.25), so_trans_hz=0.6)
    for key in ("peak_phase_stats", "preferred_phase_stats"):
        s = res[key]
        print(f"[numerics] tfr planted detector {key}: n {s['n']} mean {s['mean']:.4f} R {s['R']:.4f}")
        assert R.circ_dist(s["mean"], 0.0) <= 0.1 and s["R"] >= 0.95, (key, s)
    both = M.compare_coupling(res, _planted_device(1, 2.0)[1])
    assert abs(both["preferred_phase_distance"] - 2.0) <= 0.2 and 0.0 <= both["mvl"]["ks"] <= 1.0 and both["synthetic"]["n_events"] == 48


# ------------------------------------------------------------------------------------------------ 5. helpers and the entry script
def test_spectrogram_and_band_courses_agree_with_the_reference():
    from eegldm import metrics as M
    rng = np.random.default_rng(31)
    sfreq = 100.0
    x = rng.standard_normal((4, 3000)).astype(np.float32)
    x[1, 1000:1100] += 3.0 * np.sin(2 * np.pi * 13.0 * np.arange(100) / sfreq)           # a one-second sigma burst
    for window, K in (("dpss", 3), ("hann", 1)):
        sp = M.spectrogram(torch.from_numpy(x)[:, None], sfreq=sfreq, window=window, fmax=30.0)
        tp, w = M.spectrogram_tapers(200, window)
        assert tp.shape[0] == K and sp["n_fft"] == 256 and sp["n_frames"] == 60 and sp["times"][1] == 0.5 and sp["band_names"] == list(M.BANDS)
        scale = 1.0 / (sfreq * K)
        P, E = R.stft_error_bound(x, tp.astype(np.float32), np.ones(K), 256, 50, 1, 1, 1, scale, 1)
        k1 = int(np.searchsorted(np.arange(129) * sp["df"], 30.0, side="right"))
        assert sp["power"].shape == (4, 60, k1) and np.array_equal(sp["freqs"], np.arange(k1) * 100.0 / 256)
        assert np.all(np.abs(sp["power"].cpu().numpy() - P[:, :, :k1]) <= E[:, :, :k1])
        _names, ranges = M.band_bin_ranges(M.BANDS, sfreq, 256)
        bp = sp["band_power"].cpu().numpy()
        assert bp.dtype == np.float64 and np.all(np.abs(bp - R.bands64(P, ranges) * sp["df"]) <= R.bands_error_bound(P, E, ranges) * sp["df"])
        lean = M.spectrogram(torch.from_numpy(x), sfreq=sfreq, window=window, keep_power=False)
        assert lean["power"] is None and np.array_equal(lean["band_power"].cpu().numpy(), bp)
        st = M.band_course_stats(sp["band_power"])
        ref = M.band_course_stats(R.bands64(P, ranges) * sp["df"])
        for f in M.COURSE_FEATURES:
            assert np.all(np.abs(st[f] - ref[f]) <= 1e-4 * np.maximum(np.abs(ref[f]), 1e-3)), f
        sigma = sp["band_names"].index("sigma")
        assert st["cv"][1, sigma] > 2.0 * max(st["cv"][0, sigma], st["cv"][2, sigma], st["cv"][3, sigma])
    raw = M.stft_power(torch.from_numpy(x), tp, n_fft=256, hop=50, bins=(3, 9), bands=[(0, 4)])
    assert raw["n_frames"] == 60 and raw["power"].shape == (4, 60, 6) and raw["bands"].shape == (4, 60, 1)
    assert M.stft_power(torch.zeros(0, 3000), tp, bins=False, bands=[(0, 4)])["bands"].shape == (0, 30, 1)


def test_time_frequency_script_round_trip(tmp_path):
    from eegldm.entry import time_frequency as T
    real = np.concatenate([R.planted_windows(0, 0.0)[0], R.planted_windows(1, 0.0)[0][:8]])[:, None, :]          # (24, 1, 3000)
    syn = R.planted_windows(2, 2.0)[0][:10][:, None, :]
    os.makedirs(tmp_path / "syn")
    np.save(tmp_path / "syn" / "sample_0.npy", syn[:4]); np.save(tmp_path / "syn" / "sample_1.npy", syn[4:])
    np.save(tmp_path / "syn" / "sample_0_label.npy", np.array([2, 2, 2, 2])); np.save(tmp_path / "syn" / "sample_1_label.npy", np.array([2, 2, 3, 3, 3, 3]))
    np.save(tmp_path / "hold.npy", real)
    out = str(tmp_path / "time_frequency.json")
    res = T.main(T.parse_args(["--samples", str(tmp_path / "syn" / "sample_*.npy"), "--holdout_npy", str(tmp_path / "hold.npy"), "--labels_from_samples",
                               "--so_lo", "0.4", "--so_trans_hz", "0.6", "--chunk", "7", "--seed", "1", "--output", out]))
    with open(out) as f:
        back = json.load(f)
    assert back == json.loads(json.dumps(res))
    assert back["n_real"] == 24 and back["n_synthetic"] == 10 and back["window_s"] == 30.0 and back["band_names"] == ["delta", "theta", "alpha", "sigma", "beta"]
    for side, n in (("real", 24), ("synthetic", 10)):
        bc = back[side]["band_courses"]
        assert bc["n_windows"] == n and sorted(bc["bands"]) == sorted(back["band_names"])
        for band in back["band_names"]:
            assert sorted(bc["bands"][band]) == ["cv", "lag1", "mean"] and bc["bands"][band]["mean"]["n"] == n and bc["bands"][band]["mean"]["mean"] > 0
    assert "per_stage" not in back["real"]["band_courses"]
    st = back["synthetic"]["band_courses"]["per_stage"]
    assert sorted(st) == ["2", "3"] and st["2"]["n_windows"] == 6 and st["3"]["n_windows"] == 4
    for block in ("real_vs_synthetic", "real_vs_real"):
        for band in back["band_names"]:
            for feat in ("mean", "cv", "lag1"):
                v = back[block]["band_courses"][band][feat]
                assert 0.0 <= v["ks"] <= 1.0 and v["wasserstein"] >= 0.0
        cp = back[block]["coupling"]
        assert cp["real"]["n_events"] >= 20 and cp["synthetic"]["n_events"] >= 10 and 0.0 <= cp["mvl"]["ks"] <= 1.0
    assert back["real_vs_real"]["n"] == [12, 12]
    assert abs(back["real_vs_synthetic"]["coupling"]["preferred_phase_distance"] - 2.0) <= 0.3 and back["real_vs_real"]["coupling"]["preferred_phase_distance"] <= 0.2
    assert "not been validated" in back["caveat"] and "not evidence of realism" in back["caveat"]
    # one long recording: band courses, and the spectrogram on request
    rec = np.concatenate(list(real[:4, 0]))[None, None, :]                                  # (1, 1, 12000)
    np.save(tmp_path / "long_0.npy", rec)
    r = T.main(T.parse_args(["--recording", str(tmp_path / "long_0.npy"), "--save_spectrogram", "--output_dir", str(tmp_path / "rec")]))
    bp, times = np.load(r["stem"] + "_band_power.npy"), np.load(r["stem"] + "_times.npy")
    sg, freqs = np.load(r["stem"] + "_spectrogram.npy"), np.load(r["stem"] + "_freqs.npy")
    assert bp.shape == (1, 240, 5) and times.shape == (240,) and sg.shape == (1, 240, 129) and freqs.shape == (129,) and r["n_frames"] == 240
    assert np.all(bp > 0) and np.all(np.isfinite(sg)) and json.load(open(r["stem"] + "_bands.json"))["band_names"] == back["band_names"]
    T.main(T.parse_args(["--recording", str(tmp_path / "long_0.npy"), "--output_dir", str(tmp_path / "rec2")]))
    assert not os.path.exists(tmp_path / "rec2" / "long_0_spectrogram.npy") and np.array_equal(np.load(tmp_path / "rec2" / "long_0_band_power.npy"), bp)
