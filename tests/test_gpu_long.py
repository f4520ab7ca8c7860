"""-m gpu: long recordings (overlapped windows on one canvas) -- eegldm_canvas_step against the float64 recursion and against
eegldm_multistep_step bit for bit wherever one window owns a position, the gather and compose kernels, the native loop
(eegldm_sample_long) against eegldm_sample_multistep and against the torch host loop, seamlessness with a zero network, and the entry
script."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from make_golden_cases import UNET_CASES  # noqa: E402
from param_gen import normal  # noqa: E402
from test_gpu_dpm_solver import U24, _ae, _carve, _step_reference, _tiny  # noqa: E402

# (L, C, R, W, m, r): L = 16 / 64, C = 1 / 3, R = 1 / 2, W = 1 / 2 / 3 / 5; (m, r) = (0, 0), (4, 0), (4, 8), (3, 5) -- the last has an odd
# stride (53), so canvas and window offsets fall on every residue mod 4 against each other; L = 16 admits only the first two (L >= 3 m + 2 r)
SHAPES = [(16, 1, 1, 1, 0, 0), (16, 3, 2, 2, 0, 0), (16, 1, 2, 3, 4, 0), (16, 3, 1, 5, 4, 0), (64, 1, 1, 2, 4, 8), (64, 3, 2, 3, 4, 8),
          (64, 1, 2, 5, 3, 5), (64, 3, 1, 3, 3, 5), (64, 1, 1, 1, 4, 8), (64, 1, 2, 5, 0, 0)]
OFFSETS = {"aligned": [0] * 8, "all+4B": [1] * 8, "all+8B": [2] * 8, "all+12B": [3] * 8, "mixed": [0, 1, 2, 3, 1, 3, 2, 0]}
COEF = [(0.0123, 0.93, 0.41, 0.0), (0.31, 0.78, 0.9, -0.37)]          # (a_t, cx, c0, c1): c1 = 0 and c1 != 0


def _f32(v):
    return float(np.float32(v))


def _lay(W, L, m, r):
    from eegldm.sampling import long_layout
    return long_layout(W, L, m, r)


def _slices(cv, lay):
    """(R, C, Lc) -> (R * W, C, L) by torch slicing"""
    R, Cc, _ = cv.shape
    S, L = lay.stride, lay.window_len
    return torch.stack([cv[:, :, k * S:k * S + L] for k in range(lay.n_windows)], 1).reshape(R * lay.n_windows, Cc, L)


def _inputs(shape, guided, pred, seed):
    L, Cc, R, W, m, r = shape
    lay = _lay(W, L, m, r)
    nw, n = R * W * Cc * L, R * Cc * lay.canvas_len
    mo = torch.from_numpy(normal((2 * nw if guided else nw,), seed=seed)) * (0.6 if pred == "sample" else 1.0)
    canvas = torch.from_numpy(normal((n,), seed=seed + 1)).reshape(R, Cc, lay.canvas_len)
    hist = (torch.from_numpy(normal((n,), seed=seed + 2)) * 0.8).reshape(R, Cc, lay.canvas_len)
    return lay, mo, canvas, hist


def _canvas_step(G, shape, mo, w, guided, canvas, hist, a_t, pred, clip, cx, c0, c1, out, win, win2, x0):
    from eegldm.schedulers import PRED
    L, Cc, R, W, m, r = shape
    G.check(G.lib.eegldm_canvas_step(G.ctx().h, G.ptr(mo), w, int(guided), G.ptr(canvas), G.ptr(hist), a_t, PRED[pred], int(clip), cx, c0, c1,
                                     R, Cc, W, L, m, r, G.ptr(out), G.ptr(win), G.ptr(win2), G.ptr(x0)))


def _canvas_reference(shape, lay, mo_h, w, guided, canvas_h, hist_h, a_t, pred, clip, cx, c0, c1):
    """float64 restatement -> (prev, x0, prev bound).  Per window the data prediction and its bound are _step_reference's (called with
    cx = 0, c0 = 1, c1 = 0 on the window rows: its x0 and x0_tol); the fused prediction is sum_k w_k x0_k with layout.weights (float32
    weights, float64 arithmetic); the update and its bound are _step_reference's on the canvas."""
    L, Cc, R, W, m, r = shape
    S, Lc = lay.stride, lay.canvas_len
    rows = _slices(canvas_h, lay).reshape(-1)
    _p, x0_k, tol_k, _t = _step_reference(mo_h, w, guided, rows, torch.zeros_like(rows), a_t, pred, clip, 0.0, 1.0, 0.0)
    x0_k, tol_k = x0_k.reshape(R, W, Cc, L), tol_k.reshape(R, W, Cc, L)
    x0, tol0, mag, cnt = (torch.zeros(R, Cc, Lc, dtype=torch.float64) for _ in range(4))
    for k in range(W):
        wk = torch.from_numpy(lay.weights(k)).double()
        sl = slice(k * S, k * S + L)
        x0[:, :, sl] += wk * x0_k[:, k]
        tol0[:, :, sl] += wk * tol_k[:, k]
        mag[:, :, sl] += (wk * x0_k[:, k]).abs()
        cnt[:, :, sl] += (wk != 0).double()
    assert ((cnt == 1) | (cnt == 2)).all()
    tol0 = tol0 + 2.0 * U24 * mag * (cnt == 2)                   # the fuse: (1 - u) * a and the fma, two roundings of values <= mag
    x, h = canvas_h.double(), hist_h.double()
    prev = cx * x + c0 * x0 + c1 * h
    tolp = 4.0 * U24 * ((cx * x).abs() + (c0 * x0).abs() + (c1 * h).abs()) + abs(c0) * tol0
    return prev, x0, tol0, tolp, cnt


# ------------------------------------------------------------------ 1. the step kernel
@pytest.mark.parametrize("layout", list(OFFSETS))
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
def test_canvas_step_vs_float64_recursion_and_multistep_step(pred, clip, guided, layout):
    """eegldm_canvas_step on random model outputs, canvas and history, every shape of SHAPES, c1 = 0 and c1 != 0, every buffer carved at the
    layout's offset from a 16-byte line.

    Bound, from the operation count (u = 2^-24), the one of test_single_step_vs_float64_recursion (tests/test_gpu_dpm_solver.py) plus the
    fuse: per window x0_k carries that file's x0_tol (rtol 2e-5, atol 2e-5, and the guided mix's 3 u (|w| |o_c - o_u| + |o|) times
    |d x0 / d o|); the fused x0 = fma(u, x0_b, (1 - u) * x0_a) adds two roundings (the product and the fma; 1 - u is the float32 weight
    layout.weights holds, so the reference uses the same number) of values no larger than M = |u x0_b| + |(1 - u) x0_a|: 2 u M, and
    passes the windows' own errors on weighted, u tol_b + (1 - u) tol_a; the update is three roundings of values no larger than
    S = |cx x| + |c0 x0| + |c1 hist|: 4 u S allowed, and x0's error enters times |c0|.

    Bit for bit: wherever ONE window carries the weight (every position when W = 1, m = r = 0 or r = 0) canvas_out, hist and pred_x0
    equal what eegldm_multistep_step returns for that window's row (run on the gathered rows, prev2 and pred_x0 included); win / win2
    equal eegldm_canvas_gather of canvas_out; hist == pred_x0; inputs unwritten; in place == out of place; a second launch repeats the
    bytes; hist = NULL with c1 = 0 == the call with a history buffer."""
    import gpu_util as G
    from eegldm.schedulers import PRED
    lib, ctx = G.lib, G.ctx()
    offs = OFFSETS[layout]
    w = 3.0
    worst = 0.0
    for si, shape in enumerate(SHAPES):
        L, Cc, R, W, m, r = shape
        for case, (a_t, cx, c0, c1) in enumerate(COEF):
            a_t, cx, c0, c1 = (_f32(v) for v in (a_t, cx, c0, c1))
            lay, mo_h, cv_h, h_h = _inputs(shape, guided, pred, 1000 + 10 * si + case)
            n, nw = cv_h.numel(), R * W * Cc * L
            mo, cv, hist = _carve(mo_h, mo_h.numel(), offs[0]), _carve(cv_h.reshape(-1), n, offs[1]), _carve(h_h.reshape(-1), n, offs[2])
            out, x0 = _carve(None, n, offs[3]), _carve(None, n, offs[4])
            win, win2 = _carve(None, nw, offs[5]), _carve(None, nw, offs[6])
            _canvas_step(G, shape, mo, w, guided, cv, hist, a_t, pred, clip, cx, c0, c1, out, win, win2, x0)
            rp, r0, tol0, tolp, cnt = _canvas_reference(shape, lay, mo_h, w, guided, cv_h, h_h, a_t, pred, clip, cx, c0, c1)
            e0 = (x0.cpu().double().reshape(rp.shape) - r0).abs()
            ep = (out.cpu().double().reshape(rp.shape) - rp).abs()
            worst = max(worst, float((e0 / tol0).max()), float((ep / tolp).max()))
            assert (e0 <= tol0).all(), (shape, case, float((e0 / tol0).max()))
            assert (ep <= tolp).all(), (shape, case, float((ep / tolp).max()))
            assert torch.equal(hist, x0)
            assert torch.equal(cv, cv_h.reshape(-1).to(G.DEV)) and torch.equal(mo, mo_h.to(G.DEV)), "an input was written"
            # the scattered rows are the gather of the new canvas
            gw, gw2 = _carve(None, nw, offs[7]), _carve(None, nw, offs[5])
            G.check(lib.eegldm_canvas_gather(ctx.h, G.ptr(out), R, Cc, W, L, lay.stride, G.ptr(gw), G.ptr(gw2)))
            assert torch.equal(win, gw) and torch.equal(win2, gw) and torch.equal(gw2, gw)
            assert torch.equal(gw.cpu(), _slices(out.cpu().reshape(R, Cc, -1), lay).reshape(-1))
            # one owner: eegldm_multistep_step on the gathered rows, bit for bit
            xr, hr = _carve(None, nw, offs[1]), _carve(None, nw, offs[2])
            G.check(lib.eegldm_canvas_gather(ctx.h, G.ptr(cv), R, Cc, W, L, lay.stride, G.ptr(xr), None))
            G.check(lib.eegldm_canvas_gather(ctx.h, G.ptr(_carve(h_h.reshape(-1), n, offs[2])), R, Cc, W, L, lay.stride, G.ptr(hr), None))
            pr, pr2, zr = _carve(None, nw, offs[3]), _carve(None, nw, offs[6]), _carve(None, nw, offs[4])
            G.check(lib.eegldm_multistep_step(ctx.h, G.ptr(mo), w, int(guided), G.ptr(xr), G.ptr(hr), a_t, PRED[pred], int(clip), cx, c0, c1, G.ptr(pr),
                                              G.ptr(pr2), G.ptr(zr), nw))
            k1, j = (torch.from_numpy(v) for v in lay.owner())
            own = lambda rows: rows.cpu().reshape(R, W, Cc, L)[:, k1, :, j].permute(1, 2, 0)          # (R, C, Lc): the owner window's value
            one = (cnt == 1)
            assert one.all() == (W == 1 or r == 0)
            assert torch.equal(out.cpu().reshape(R, Cc, -1)[one], own(pr)[one]), (shape, case, "canvas_out differs from eegldm_multistep_step")
            assert torch.equal(x0.cpu().reshape(R, Cc, -1)[one], own(zr)[one])
            if W == 1:
                assert torch.equal(out, pr) and torch.equal(win2, pr2) and torch.equal(x0, zr) and torch.equal(hist, hr)
            if m == 0 and r == 0:
                assert torch.equal(win, pr) and torch.equal(win2, pr2)
            # in place, nullable outputs left out; a repeat; no history buffer when c1 = 0
            cv2, hist2 = _carve(cv_h.reshape(-1), n, offs[1]), _carve(h_h.reshape(-1), n, offs[2])
            _canvas_step(G, shape, mo, w, guided, cv2, hist2, a_t, pred, clip, cx, c0, c1, cv2, None, None, None)
            assert torch.equal(cv2, out) and torch.equal(hist2, x0)
            out3, win3 = _carve(None, n, offs[3]), _carve(None, nw, offs[5])
            _canvas_step(G, shape, mo, w, guided, cv, _carve(h_h.reshape(-1), n, offs[2]), a_t, pred, clip, cx, c0, c1, out3, win3, None, None)
            assert out3.cpu().numpy().tobytes() == out.cpu().numpy().tobytes() and torch.equal(win3, win)
            if c1 == 0.0:
                out4 = _carve(None, n, offs[3])
                _canvas_step(G, shape, mo, w, guided, cv, None, a_t, pred, clip, cx, c0, c1, out4, None, None, None)
                assert torch.equal(out4, out)
    print(f"{pred} clip={clip} guided={guided} {layout}: worst err / tol {worst:.3f}")


def test_canvas_argument_checks():
    import gpu_util as G
    lib, ctx = G.lib, G.ctx()
    p = G.ptr
    R, Cc, W, L, m, r = 1, 1, 2, 64, 4, 8
    lay = _lay(W, L, m, r)
    mo, win, win2 = (torch.zeros(W * L, device=G.DEV) for _ in range(3))
    cv, hist, out = (torch.zeros(lay.canvas_len, device=G.DEV) for _ in range(3))
    ok = lambda *a: lib.eegldm_canvas_step(ctx.h, *a)
    assert ok(p(mo), 0.0, 0, p(cv), p(hist), 0.5, 0, 0, 1.0, 1.0, 0.5, R, Cc, W, L, m, r, p(out), p(win), p(win2), None) == 0
    assert ok(p(mo), 0.0, 0, p(cv), None, 0.5, 0, 0, 1.0, 1.0, 0.5, R, Cc, W, L, m, r, p(out), p(win), None, None) != 0          # c1 without history
    assert ok(p(mo), 0.0, 0, p(cv), p(hist), 0.5, 0, 0, 1.0, 1.0, 0.5, R, Cc, W, 27, m, r, p(out), p(win), None, None) != 0      # L < 3 m + 2 r
    assert ok(p(mo), 0.0, 0, p(cv), p(hist), 0.5, 0, 0, 1.0, 1.0, 0.5, R, Cc, W, L, -1, r, p(out), p(win), None, None) != 0
    assert ok(p(mo), 0.0, 0, p(cv), p(hist), 1.0, 0, 0, 1.0, 1.0, 0.5, R, Cc, W, L, m, r, p(out), p(win), None, None) != 0       # a_t = 1
    assert ok(p(mo), 0.0, 0, p(cv), p(hist), 0.5, 3, 0, 1.0, 1.0, 0.5, R, Cc, W, L, m, r, p(out), p(win), None, None) != 0
    assert ok(p(mo), 0.0, 0, p(cv), p(hist), 0.5, 0, 0, 1.0, 1.0, 0.5, R, Cc, W, L, m, r, p(out), p(mo), None, None) != 0        # win over model_out
    assert ok(p(mo), 0.0, 0, p(cv), p(cv), 0.5, 0, 0, 1.0, 1.0, 0.5, R, Cc, W, L, m, r, p(out), p(win), None, None) != 0         # history over the canvas
    assert ok(p(mo), 0.0, 0, p(cv), p(hist), 0.5, 0, 0, 1.0, 1.0, 0.5, R, Cc, W, L, m, r, p(out), None, p(win2), None) != 0      # win2 without win
    assert lib.eegldm_canvas_gather(ctx.h, p(cv), R, Cc, W, L, L + 1, p(win), None) != 0
    assert lib.eegldm_canvas_compose(ctx.h, p(win), R, Cc, W, L, lay.stride + 1, m, r, p(out)) != 0                              # S != L - (2 m + r)


# ------------------------------------------------------------------ 2. gather and compose
@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 3), (2, 0, 1)])
def test_gather_is_torch_slicing(offs):
    """every shape of SHAPES plus strides that belong to no layout (S = 1, 7, L), every 4-byte alignment of canvas / win / win2"""
    import gpu_util as G
    lib, ctx = G.lib, G.ctx()
    cases = [(L, Cc, R, W, L - 2 * m - r) for L, Cc, R, W, m, r in SHAPES] + [(16, 2, 2, 5, 1), (16, 1, 1, 4, 7), (19, 3, 2, 3, 19)]
    for L, Cc, R, W, S in cases:
        Lc = (W - 1) * S + L
        cv_h = torch.from_numpy(normal((R * Cc * Lc,), seed=31 + L + S)).reshape(R, Cc, Lc)
        cv = _carve(cv_h.reshape(-1), cv_h.numel(), offs[0])
        nw = R * W * Cc * L
        win, win2 = _carve(None, nw, offs[1]), _carve(None, nw, offs[2])
        G.check(lib.eegldm_canvas_gather(ctx.h, G.ptr(cv), R, Cc, W, L, S, G.ptr(win), G.ptr(win2)))
        want = torch.stack([cv_h[:, :, k * S:k * S + L] for k in range(W)], 1).reshape(-1)
        assert torch.equal(win.cpu(), want) and torch.equal(win2, win), (L, Cc, R, W, S)
        assert torch.equal(cv.cpu(), cv_h.reshape(-1))
        only = _carve(None, nw, offs[1])
        G.check(lib.eegldm_canvas_gather(ctx.h, G.ptr(cv), R, Cc, W, L, S, G.ptr(only), None))
        assert torch.equal(only, win)


@pytest.mark.parametrize("offs", [(0, 0), (1, 1), (3, 2), (2, 3), (0, 1)])
@pytest.mark.parametrize("down", [1, 4])
def test_compose_crossfades_decoded_windows(down, offs):
    """Outside the ramps the recording holds the owning window's bytes; inside, fma(u, b, (1 - u) * a) -- evaluated in float64 from the
    float32 weights of the scaled layout and rounded to float32 -- to within 1 ulp of that value."""
    import gpu_util as G
    lib, ctx = G.lib, G.ctx()
    for si, (L, Cc, R, W, m, r) in enumerate(SHAPES):
        big = _lay(W, L, m, r).scaled(down)
        Lw, Sw, Lcw = big.window_len, big.stride, big.canvas_len
        dec_h = torch.from_numpy(normal((R * W * Cc * Lw,), seed=51 + si)).reshape(R, W, Cc, Lw)
        dec, out = _carve(dec_h.reshape(-1), dec_h.numel(), offs[0]), _carve(None, R * Cc * Lcw, offs[1])
        G.check(lib.eegldm_canvas_compose(ctx.h, G.ptr(dec), R, Cc, W, Lw, Sw, big.margin, big.ramp, G.ptr(out)))
        got = out.cpu().reshape(R, Cc, Lcw)
        k1, j = (torch.from_numpy(v) for v in big.owner())
        own = dec_h[:, k1, :, j].permute(1, 2, 0)
        ramp = torch.zeros(Lcw, dtype=torch.bool)
        for a, b in big.seams():
            ramp[a:b] = True
        assert torch.equal(got[:, :, ~ramp], own[:, :, ~ramp]), (L, Cc, R, W, m, r)
        for k in range(1, W):
            a0 = k * Sw + big.margin
            u = torch.from_numpy(big.weights(k)[big.margin:big.margin + big.ramp])
            assert torch.equal(torch.from_numpy(big.weights(k - 1)[Sw + big.margin:Sw + big.margin + big.ramp]), 1.0 - u)
            later, earlier = dec_h[:, k, :, big.margin:big.margin + big.ramp], dec_h[:, k - 1, :, Sw + big.margin:Sw + big.margin + big.ramp]
            ref = (u.double() * later.double() + ((1.0 - u) * earlier).double()).float()
            g = got[:, :, a0:a0 + big.ramp]
            ulp = torch.from_numpy(np.spacing(np.abs(ref.numpy())))
            assert ((g.double() - ref.double()).abs() <= ulp.double()).all(), (L, Cc, R, W, m, r, k)
        assert torch.equal(dec.cpu(), dec_h.reshape(-1))
        again = _carve(None, R * Cc * Lcw, offs[1])
        G.check(lib.eegldm_canvas_compose(ctx.h, G.ptr(dec), R, Cc, W, Lw, Sw, big.margin, big.ramp, G.ptr(again)))
        assert again.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()


# ------------------------------------------------------------------ 3. the native loop
def _tables(sched):
    from eegldm.sampling import _multistep_tables
    ts, a_t, cx, c0, c1 = _multistep_tables(sched)
    i64, f32 = (lambda v: (C.c_int64 * len(v))(*v)), (lambda v: (C.c_float * len(v))(*v))
    return (i64(ts), f32(a_t), f32(cx), f32(c0), f32(c1), len(ts))


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("order", [1, 2])
def test_native_loop_is_the_multistep_loop_without_overlap(order, graph):
    """W = 1 (with a margin and a ramp that then touch nothing): eegldm_sample_long returns eegldm_sample_multistep's bytes, canvas and
    windows; m = r = 0, W = 3: the bytes of a 3-row eegldm_sample_multistep call, the recording being the windows side by side."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample, sample_long
    _cfg, _sd, net = _tiny(601)
    ae = _ae(602)
    L = 64
    sched = make_sampling_scheduler(5, sampler="dpmpp_2m", solver_order=order)
    noise = torch.from_numpy(normal((1, 1, L), seed=603)).to(G.DEV)
    win, z = sample(net, ae, sched, noise, scale_factor=0.7, crop=0, use_graph=graph)
    info = {}
    rec, cv = sample_long(net, ae, sched, noise, 1, margin=4, ramp=8, scale_factor=0.7, crop=0, use_graph=graph, info=info)
    assert info["graph"] == graph and info["layout"].canvas_len == L
    assert torch.equal(cv, z) and torch.equal(rec, win)
    noise3 = torch.from_numpy(normal((3, 1, L), seed=604)).to(G.DEV)
    win3, z3 = sample(net, ae, sched, noise3, scale_factor=0.7, crop=0, use_graph=graph)
    canvas_noise = noise3.permute(1, 0, 2).reshape(1, 1, 3 * L).contiguous()
    rec3, cv3 = sample_long(net, ae, sched, canvas_noise, 3, margin=0, ramp=0, scale_factor=0.7, crop=0, use_graph=graph)
    assert torch.equal(cv3.reshape(3, 1, L), z3) and torch.equal(rec3.reshape(3, 1, 4 * L), win3)
    # the export itself, without the autoencoder and with only one of the outputs
    lat = torch.empty(1, 1, 3 * L, device=G.DEV)
    G.check(G.lib.eegldm_sample_long(net.h, None, G.ptr(canvas_noise), *_tables(sched)[:5], 5, 0, 0, 1.0, G.ptr(lat), None, 1, 3, L, 0, 0, int(graph),
                                     None, None, 1.0, 0))
    assert torch.equal(lat, cv3)
    assert G.lib.eegldm_sample_long(net.h, None, G.ptr(canvas_noise), *_tables(sched)[:5], 5, 0, 0, 1.0, None, None, 1, 3, L, 0, 0, 0, None, None, 1.0, 0) != 0
    assert G.lib.eegldm_sample_long(net.h, None, G.ptr(canvas_noise), *_tables(sched)[:5], 5, 0, 0, 1.0, G.ptr(lat), None, 1, 3, L, 30, 0, 0, None, None, 1.0, 0) != 0


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("dtype,case,R,W", [("float32", "tiny_l64", 1, 1), ("float32", "tiny_l64", 1, 5), ("bfloat16", "tiny_l64", 1, 5),
                                            ("bfloat16", "small_l256", 32, 4)])
def test_native_loop_matches_hostloop_ldm(dtype, case, R, W, graph, order):
    """sample_long (eegldm_sample_long) against sample_long_hostloop -- slicing, model, x0, taper, update, decode per window and cross-fade in
    torch -- with the comparison and the 5e-5 relative-L2 bound of the loop test in tests/test_gpu_edit.py: LDM with z / scale_factor and
    the decode, (m, r) = (4, 8), 5 steps, R * W = 1, 5 and 128 (bfloat16, L = 256: the 128-channel layers on the big-tile GEMM).  Two native
    runs are bit-identical; the recording has length down * Lc - 2 * crop."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample_long, sample_long_hostloop
    _cfg, _sd, net = _tiny(611, dtype, case)
    ae = _ae(612, dtype)
    L = UNET_CASES[case][2]
    lay = _lay(W, L, 4, 8)
    noise = torch.from_numpy(normal((R, 1, lay.canvas_len), seed=613))
    sched = make_sampling_scheduler(5, sampler="dpmpp_2m", solver_order=order)
    assert order == 1 or any(sched.c1)
    info = {}
    rec, cv = sample_long(net, ae, sched, noise, W, margin=4, ramp=8, scale_factor=0.7, crop=8, use_graph=graph, info=info)
    assert info["graph"] == graph
    assert rec.shape == (R, 1, 4 * lay.canvas_len - 16) and cv.shape == (R, 1, lay.canvas_len) and torch.isfinite(rec).all()
    rec2, cv2 = sample_long(net, ae, sched, noise, W, margin=4, ramp=8, scale_factor=0.7, crop=8, use_graph=graph)
    assert torch.equal(cv2, cv) and torch.equal(rec2, rec)
    rech, cvh = sample_long_hostloop(net, ae, sched, noise, W, margin=4, ramp=8, scale_factor=0.7, crop=8)
    print(f"{dtype} {case} R={R} W={W} graph={graph} order={order}: canvas rel-L2 {G.rel_l2(cv, cvh):.3e}, recording {G.rel_l2(rec, rech):.3e}")
    assert G.rel_l2(cv, cvh) < 5e-5 and G.rel_l2(rec, rech) < 5e-5


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("R,W", [(1, 5), (2, 3)])
def test_native_loop_matches_hostloop_conditional_and_guided(R, W, graph, order):
    """Class-conditional fp32 UNet, pixel-space call (autoencoder=None, the canvas is the recording), (m, r) = (3, 5) (odd stride): plain
    conditional with labels that differ from window to window, and guided with w = 3, against the host loop (5e-5 as above); W labels are
    broadcast over the recordings; guidance changes the result; repeats are bit-identical."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample_long, sample_long_hostloop
    _cfg, _sd, net = _tiny(621, num_classes=3)
    L = 64
    lay = _lay(W, L, 3, 5)
    noise = torch.from_numpy(normal((R, 1, lay.canvas_len), seed=622))
    lab = [2, 0, 1, 2, 0, 1][:R * W]
    sched = make_sampling_scheduler(5, sampler="dpmpp_2m", solver_order=order)
    kw = dict(margin=3, ramp=5, crop=4)
    rec, cv = sample_long(net, None, sched, noise, W, use_graph=graph, labels=lab, **kw)
    assert rec.shape == (R, 1, lay.canvas_len - 8) and torch.equal(rec, cv[:, :, 4:-4])
    _r, cvh = sample_long_hostloop(net, None, sched, noise, W, labels=lab, **kw)
    g = dict(labels=lab, guidance_scale=3.0, null_class=1)
    _r, cvg = sample_long(net, None, sched, noise, W, use_graph=graph, **g, **kw)
    _r, cvgh = sample_long_hostloop(net, None, sched, noise, W, **g, **kw)
    print(f"R={R} W={W} graph={graph} order={order}: conditional rel-L2 {G.rel_l2(cv, cvh):.3e}, guided {G.rel_l2(cvg, cvgh):.3e}")
    assert G.rel_l2(cv, cvh) < 5e-5 and G.rel_l2(cvg, cvgh) < 5e-5
    assert G.rel_l2(cvg, cv) > 1e-3
    assert torch.equal(sample_long(net, None, sched, noise, W, use_graph=graph, **g, **kw)[1], cvg)
    assert torch.equal(sample_long(net, None, sched, noise, W, use_graph=graph, labels=lab, guidance_scale=1.0, null_class=1, **kw)[1], cv)
    # W labels stand for every recording; other labels give another canvas
    assert torch.equal(sample_long(net, None, sched, noise, W, use_graph=graph, labels=(lab[:W] * R), **kw)[1],
                       sample_long(net, None, sched, noise, W, use_graph=graph, labels=lab[:W], **kw)[1])
    assert not torch.equal(sample_long(net, None, sched, noise, W, use_graph=graph, labels=[0] * W, **kw)[1], cv) or lab[:W] == [0] * W


def test_zero_network_gives_the_elementwise_recursion():
    """All weights zero: the model output is 0, x0 depends on xc alone, so both windows of a ramp predict the same value and the canvas has
    to follow the plain multistep recursion element by element -- whatever the network would have done at a window edge.  Outside the
    ramps: eegldm_multistep_step applied to the canvas-shaped buffer, bit for bit.  Inside: fusing two equal values b as fma(u, b, (1 - u)
    * b) is two roundings, <= 2 u |x0|; with E the error of x so far, x0 = x / sqrt(a) differs by E / sqrt(a) plus the two divisions'
    own rounding (3 u |x0| allowed); the update passes |cx| E + |c0| d0_i + |c1| d0_{i-1} on and adds its three roundings on either side
    (6 u S, S = |cx x| + |c0 x0| + |c1 hist|).  The bound is that recursion, evaluated in float64 along the run."""
    import gpu_util as G
    from eegldm.sampling import _multistep_tables, make_sampling_scheduler, sample_long
    _cfg, sd, net = _tiny(631)
    net.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()})
    R, W, L = 2, 3, 64
    lay = _lay(W, L, 4, 8)
    noise = torch.from_numpy(normal((R, 1, lay.canvas_len), seed=632)).to(G.DEV)
    sched = make_sampling_scheduler(5, sampler="dpmpp_2m")
    _rec, cv = sample_long(net, None, sched, noise, W, margin=4, ramp=8, crop=0)
    ts, a_t, cx, c0, c1 = _multistep_tables(sched)
    x, hist, zero = noise.clone().reshape(-1), torch.zeros(noise.numel(), device=G.DEV), torch.zeros(noise.numel(), device=G.DEV)
    E, d_prev = torch.zeros(noise.numel(), dtype=torch.float64), torch.zeros(noise.numel(), dtype=torch.float64)
    for i in range(len(ts)):
        xd, hd = x.double().cpu(), hist.double().cpu()
        x0 = torch.empty_like(x)
        G.check(G.lib.eegldm_multistep_step(G.ctx().h, G.ptr(zero), 0.0, 0, G.ptr(x), G.ptr(hist), a_t[i], 0, 0, cx[i], c0[i], c1[i], G.ptr(x), None,
                                            G.ptr(x0), x.numel()))
        x0d = x0.double().cpu()
        d0 = E / a_t[i] ** 0.5 + 5.0 * U24 * x0d.abs()
        S = (cx[i] * xd).abs() + (c0[i] * x0d).abs() + (c1[i] * hd).abs()
        E = abs(cx[i]) * E + abs(c0[i]) * d0 + abs(c1[i]) * d_prev + 6.0 * U24 * S
        d_prev = d0
    ramp = torch.zeros(lay.canvas_len, dtype=torch.bool)
    for a, b in lay.seams():
        ramp[a:b] = True
    got, want = cv.cpu().reshape(R, lay.canvas_len), x.cpu().reshape(R, lay.canvas_len)
    assert torch.equal(got[:, ~ramp], want[:, ~ramp])
    err = (got.double() - want.double()).abs()
    print(f"zero network: max |canvas - recursion| inside the ramps {float(err[:, ramp].max()):.3e}, bound {float(E.reshape(R, -1)[:, ramp].max()):.3e}")
    assert (err <= E.reshape(R, -1)).all()
    assert float(want.abs().max()) > 0.1


# ------------------------------------------------------------------ 4. entry script
def test_entry_script_writes_a_recording(tmp_path):
    """sample_long.py --n_windows 3 on tiny seeded checkpoints (class-conditional UNet): the three files, the layout json against
    long_layout, the labels against a 2-epoch hypnogram (margin 100 and ramp 150 latents: stride 418 latents = 16.72 s, window centres at
    15.36, 32.08 and 48.8 s -> epochs 0, 1, 1); the pixel-space twin; a rerun repeats the bytes and another seed does not."""
    import entry_pin_case as E
    from eegldm.entry import sample_long as SL
    from eegldm.models import UNetModel
    out = str(tmp_path)
    a_yaml, l_yaml, run_a, run_l, run_d = E.write_checkpoints(out)
    up = dict(E.LDM_YAML["model"]["params"]["unet_config"]["params"], in_channels=1, out_channels=1, num_classes=4)
    sd = E._seeded(UNetModel(**up), 303)
    torch.save(sd, os.path.join(run_l, "best_model.pth")); torch.save(sd, os.path.join(run_d, "best_model.pth"))
    hyp = os.path.join(out, "stages.npy")
    np.save(hyp, np.asarray([3, 1]))
    common = ["--output_dir", out, "--num_inference_steps", "4", "--n_windows", "3", "--num_classes", "4", "--hypnogram", hyp]
    ldm = common + ["--best_model_path", run_a, "--diffusion_path", run_l, "--autoencoderkl_config_file_path", a_yaml, "--ldm_config_file_path",
                    l_yaml, "--latent_channels", "1", "--margin", "100", "--ramp", "150"]
    dm = common + ["--pixel", "--config_file", l_yaml, "--diffusion_path", run_d, "--margin", "400", "--ramp", "600"]

    def run(base, *extra, seed=0):
        d = SL.main(SL.parse_args(base + list(extra) + ["--seed", str(seed)]))
        return (np.load(os.path.join(d, f"long_{seed}.npy")), np.load(os.path.join(d, f"long_{seed}_labels.npy")),
                json.load(open(os.path.join(d, f"long_{seed}_layout.json"))))

    for base, down, m, r in ((ldm, 4, 100, 150), (dm, 1, 400, 600)):
        rec, lab, lj = run(base)
        lay = _lay(3, 3072 // down, m, r).scaled(down)
        assert rec.shape == (1, 1, lay.canvas_len - 72) and rec.dtype == np.float32 and np.isfinite(rec).all()
        assert lj["samples"] == rec.shape[-1] and lj["S"] == lay.stride and lj["m"] == lay.margin and lj["r"] == lay.ramp
        assert lj["starts"] == [s - 36 for s in lay.starts] and lj["seams"] == [[a - 36, b - 36] for a, b in lay.seams()] and lj["n_windows"] == 3
        assert list(lab) == [3, 1, 1] and lab.dtype == np.int64
        again, _l, _j = run(base)
        assert again.tobytes() == rec.tobytes()
        other, _l, _j = run(base, seed=5)
        assert not np.array_equal(other, rec)
        guided, _l, _j = run(base, "--null_class", "0", "--guidance_scale", "2.0")
        assert np.isfinite(guided).all() and not np.array_equal(guided, rec)
