"""-m gpu: repairing and extending real recordings on the canvas -- eegldm_canvas_edit_step against the float64 recursion and, bit for
bit, against eegldm_canvas_step / eegldm_edit_start / eegldm_edit_step wherever they say the same thing; encode_long; the native loop
(eegldm_sample_long_edit) against eegldm_sample_long, eegldm_sample_edit and the torch host loop; the exact properties of masks; the
entry script."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from make_golden_cases import UNET_CASES  # noqa: E402
from param_gen import normal  # noqa: E402
from test_gpu_dpm_solver import U24, _ae, _carve, _tiny  # noqa: E402
from test_gpu_long import COEF, OFFSETS, SHAPES, _canvas_reference, _canvas_step, _f32, _inputs, _lay, _slices  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_NEXT = [0.05, 0.52, 1.0]
MASKS = ["zeros", "ones", "binary", "fractional"]


def _canvas_mask(kind, lay, R, Cc, seed):
    """(R, Cc, Lc) keep-mask.  binary: the value toggles at edges on every residue mod 4 (positions 1, 6, 11, 12), at one edge inside the
    second window's leading margin and one inside its ramp (where the layout has them), and at one row-dependent position."""
    Lc = lay.canvas_len
    if kind == "zeros":
        return torch.zeros(R, Cc, Lc)
    if kind == "ones":
        return torch.ones(R, Cc, Lc)
    if kind == "fractional":
        return torch.from_numpy(np.random.default_rng(seed).random((R, Cc, Lc)).astype(np.float32))
    edges = [1, 6, 11, 12]
    if lay.n_windows > 1 and lay.margin:
        edges.append(lay.stride + lay.margin // 2)
    if lay.n_windows > 1 and lay.ramp:
        edges.append(lay.stride + lay.margin + lay.ramp // 2)
    m = torch.ones(R, Cc, Lc)
    for row in range(R * Cc):
        v, at = 1.0, sorted(set(e for e in edges + [(17 + 5 * row) % Lc] if 0 < e < Lc))
        line = torch.ones(Lc)
        for a, b in zip(at, at[1:] + [Lc]):
            v = 1.0 - v
            line[a:b] = v
        m[row // Cc, row % Cc] = line
    return m


def _edit_step(G, shape, mo, w, guided, canvas, hist, a_t, a_next, pred, clip, cx, c0, c1, known, noise, mask, out, win, win2, x0):
    from eegldm.schedulers import PRED
    L, Cc, R, W, m, r = shape
    G.check(G.lib.eegldm_canvas_edit_step(G.ctx().h, G.ptr(mo), w, int(guided), G.ptr(canvas), G.ptr(hist), a_t, a_next, PRED[pred], int(clip), cx, c0,
                                          c1, R, Cc, W, L, m, r, G.ptr(known), G.ptr(noise), G.ptr(mask), G.ptr(out), G.ptr(win), G.ptr(win2),
                                          G.ptr(x0)))


# ------------------------------------------------------------------ 1. the step kernel
@pytest.mark.parametrize("layout", list(OFFSETS))
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
def test_canvas_edit_step_vs_float64_recursion_and_its_neighbours(pred, clip, guided, layout):
    """eegldm_canvas_edit_step on every shape of SHAPES (tests/test_gpu_long.py), c1 = 0 and c1 != 0, a_next < 1 and == 1, the four mask
    kinds, every buffer (known, noise and mask included) carved at the layout's offset from a 16-byte line.

    Bound, from the operation count (u = 2^-24), against  out = m k + (1 - m) x',  x' the float64 canvas step:
      * x' carries _canvas_reference's bound (tests/test_gpu_long.py: the per-window x0 tolerance, 2 u M for the fuse, 4 u S for the
        update, x0's error times |c0|).
      * k = fma(ka, z0, kb * noise) is two roundings of values no larger than K = |ka z0| + |kb noise|, and ka, kb are each a rounded
        sqrtf (one u on each term): |d k| <= 3 u K; 4 u K allowed, as tests/test_gpu_edit.py counts it.  a_next == 1: k = z0 exactly.
      * the blend fma(m, k, (1 - m) * x'): 1 - m, the product and the fma are roundings of values no larger than |m k| + |(1 - m) x'|
        (two of the blend's own magnitudes plus the rounded 1 - m: 3 u of that, 4 u allowed, as that file allows), and the operands'
        errors enter as m |d k| + (1 - m) |d x'|.
    Bit for bit: mask = NULL and mask == 0 are eegldm_canvas_step (canvas_out, win, win2, hist, pred_x0); mask == 1 is eegldm_edit_start's
    x_start at a_next; a binary mask picks between the two; wherever ONE window owns a position the result is eegldm_edit_step's
    (multistep form) for that window's gathered row -- all of it when W = 1 or m = r = 0; win / win2 are eegldm_canvas_gather of
    canvas_out; hist == pred_x0 == eegldm_canvas_step's unblended prediction; inputs unwritten; in place == out of place; a repeat
    gives the same bytes."""
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
            a_next = _f32(A_NEXT[(si + case) % 3])
            lay, mo_h, cv_h, h_h = _inputs(shape, guided, pred, 2000 + 10 * si + case)
            n, nw = cv_h.numel(), R * W * Cc * L
            z_h = torch.from_numpy(normal((n,), seed=2400 + 10 * si + case)) * 0.7
            nz_h = torch.from_numpy(normal((n,), seed=2700 + 10 * si + case))
            mo, cv, hist = _carve(mo_h, mo_h.numel(), offs[0]), _carve(cv_h.reshape(-1), n, offs[1]), _carve(h_h.reshape(-1), n, offs[2])
            known, noise = _carve(z_h, n, offs[5]), _carve(nz_h, n, offs[6])
            fresh_hist = lambda: _carve(h_h.reshape(-1), n, offs[2])
            # the unblended step, by eegldm_canvas_step and by mask = NULL
            plain, plain0, pwin, pwin2 = _carve(None, n, offs[3]), _carve(None, n, offs[4]), _carve(None, nw, offs[5]), _carve(None, nw, offs[6])
            _canvas_step(G, shape, mo, w, guided, cv, hist, a_t, pred, clip, cx, c0, c1, plain, pwin, pwin2, plain0)
            hn, outn, x0n, winn, win2n = fresh_hist(), _carve(None, n, offs[3]), _carve(None, n, offs[4]), _carve(None, nw, offs[5]), _carve(None, nw, offs[6])
            _edit_step(G, shape, mo, w, guided, cv, hn, a_t, a_next, pred, clip, cx, c0, c1, None, None, None, outn, winn, win2n, x0n)
            assert torch.equal(outn, plain) and torch.equal(x0n, plain0) and torch.equal(hn, hist) and torch.equal(winn, pwin) and torch.equal(win2n, pwin2)
            # k by the start kernel
            kdev = _carve(None, n, offs[3])
            G.check(lib.eegldm_edit_start(ctx.h, G.ptr(known), 1.0, G.ptr(noise), a_next, None, G.ptr(kdev), n))
            if a_next == 1.0:
                assert torch.equal(kdev, known)
            rp, _r0, _tol0, tolp, cnt = _canvas_reference(shape, lay, mo_h, w, guided, cv_h, h_h, a_t, pred, clip, cx, c0, c1)
            ka, kb = a_next ** 0.5, (1.0 - a_next) ** 0.5
            zd, nd = z_h.double().reshape(rp.shape), nz_h.double().reshape(rp.shape)
            rk = ka * zd + kb * nd
            tolk = 4.0 * U24 * ((ka * zd).abs() + (kb * nd).abs()) if a_next < 1.0 else torch.zeros_like(rk)
            # the gathered rows of the inputs, for eegldm_edit_step
            rows = {}
            for name, host in (("x", cv_h.reshape(-1)), ("h", h_h.reshape(-1)), ("z", z_h), ("nz", nz_h)):
                rows[name] = _slices(host.reshape(R, Cc, -1), lay).reshape(-1)
            k1, j = (torch.from_numpy(v) for v in lay.owner())
            own = lambda v: v.cpu().reshape(R, W, Cc, L)[:, k1, :, j].permute(1, 2, 0)          # (R, C, Lc): the owner window's value
            one = (cnt == 1)
            coef = (C.c_float * 3)(cx, c0, c1)
            for mi, mname in enumerate(MASKS):
                m_h = _canvas_mask(mname, lay, R, Cc, 3000 + 10 * si + case)
                mask = _carve(m_h.reshape(-1), n, offs[7])
                h2, out, x0, win, win2 = fresh_hist(), _carve(None, n, offs[3]), _carve(None, n, offs[4]), _carve(None, nw, offs[5]), _carve(None, nw, offs[6])
                _edit_step(G, shape, mo, w, guided, cv, h2, a_t, a_next, pred, clip, cx, c0, c1, known, noise, mask, out, win, win2, x0)
                md = m_h.double()
                ref = md * rk + (1.0 - md) * rp
                tol = 4.0 * U24 * ((md * rk).abs() + ((1.0 - md) * rp).abs()) + md * tolk + (1.0 - md) * tolp
                err = (out.cpu().double().reshape(rp.shape) - ref).abs()
                worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
                assert (err <= tol).all(), (shape, case, mname, float((err / tol.clamp_min(1e-300)).max()))
                assert torch.equal(h2, x0) and torch.equal(x0, plain0), "hist / pred_x0 must hold the model's own fused x0"
                for buf, host in ((cv, cv_h), (mo, mo_h), (known, z_h), (noise, nz_h), (mask, m_h)):
                    assert torch.equal(buf, host.reshape(-1).to(G.DEV)), "an input was written"
                if mname == "zeros":
                    assert torch.equal(out, plain) and torch.equal(win, pwin) and torch.equal(win2, pwin2)
                if mname == "ones":
                    assert torch.equal(out, kdev)
                if mname == "binary":
                    assert torch.equal(out, torch.where(mask == 1.0, kdev, plain))
                    assert bool((mask == 1.0).any()) and bool((mask == 0.0).any())
                # the scattered rows are the gather of the new canvas
                gw = _carve(None, nw, offs[7])
                G.check(lib.eegldm_canvas_gather(ctx.h, G.ptr(out), R, Cc, W, L, lay.stride, G.ptr(gw), None))
                assert torch.equal(win, gw) and torch.equal(win2, gw)
                # one owner: eegldm_edit_step (multistep form) on the gathered rows, bit for bit
                xr, hr, zr, nr = (_carve(rows[k], nw, offs[i]) for k, i in (("x", 1), ("h", 2), ("z", 5), ("nz", 6)))
                mr = _carve(_slices(m_h, lay).reshape(-1), nw, offs[7])
                pr, pr2, x0r = _carve(None, nw, offs[3]), _carve(None, nw, offs[6]), _carve(None, nw, offs[4])
                G.check(lib.eegldm_edit_step(ctx.h, G.ptr(mo), w, int(guided), G.ptr(xr), G.ptr(hr), a_t, a_next, PRED[pred], int(clip), coef, G.ptr(zr),
                                             G.ptr(nr), G.ptr(mr), G.ptr(pr), G.ptr(pr2), G.ptr(x0r), nw))
                assert one.all() == (W == 1 or r == 0)
                assert torch.equal(out.cpu().reshape(R, Cc, -1)[one], own(pr)[one]), (shape, case, mname, "differs from eegldm_edit_step")
                if W == 1:
                    assert torch.equal(out, pr) and torch.equal(win2, pr2) and torch.equal(x0, x0r) and torch.equal(h2, hr)
                if m == 0 and r == 0:
                    assert torch.equal(win, pr) and torch.equal(win2, pr2)
                # in place with the nullable outputs left out; a repeat
                cv2, h3 = _carve(cv_h.reshape(-1), n, offs[1]), fresh_hist()
                _edit_step(G, shape, mo, w, guided, cv2, h3, a_t, a_next, pred, clip, cx, c0, c1, known, noise, mask, cv2, None, None, None)
                assert torch.equal(cv2, out) and torch.equal(h3, x0)
                if mi >= 2:
                    out3, win3 = _carve(None, n, offs[3]), _carve(None, nw, offs[5])
                    _edit_step(G, shape, mo, w, guided, cv, fresh_hist(), a_t, a_next, pred, clip, cx, c0, c1, known, noise, mask, out3, win3, None, None)
                    assert out3.cpu().numpy().tobytes() == out.cpu().numpy().tobytes() and torch.equal(win3, win)
    print(f"{pred} clip={clip} guided={guided} {layout}: worst err / tol {worst:.3f}")


def test_canvas_edit_step_argument_checks():
    import gpu_util as G
    lib, ctx = G.lib, G.ctx()
    p = G.ptr
    R, Cc, W, L, m, r = 1, 1, 2, 64, 4, 8
    lay = _lay(W, L, m, r)
    mo, win = (torch.zeros(W * L, device=G.DEV) for _ in range(2))
    cv, hist, out, kn, nz, mk = (torch.zeros(lay.canvas_len, device=G.DEV) for _ in range(6))
    ok = lambda a_next, known, noise, mask, o=out: lib.eegldm_canvas_edit_step(ctx.h, p(mo), 0.0, 0, p(cv), p(hist), 0.5, a_next, 0, 0, 1.0, 1.0, 0.5, R, Cc,
                                                                               W, L, m, r, p(known), p(noise), p(mask), p(o), p(win), None, None)
    assert ok(0.6, kn, nz, mk) == 0 and ok(1.0, kn, nz, mk) == 0 and ok(0.6, None, None, None) == 0
    assert ok(0.6, None, nz, mk) != 0 and ok(0.6, kn, None, mk) != 0            # a mask needs known and noise
    assert ok(0.0, kn, nz, mk) != 0 and ok(1.5, kn, nz, mk) != 0                # a_next outside (0, 1]
    assert ok(0.6, out, nz, mk) != 0 and ok(0.6, kn, nz, hist) != 0 and ok(0.6, kn, cv, mk, o=cv) != 0      # an edit input over an output
    assert ok(0.6, cv, nz, mk) == 0                                             # ... but it may be the (read-only) canvas when not in place


# ------------------------------------------------------------------ 2. encode_long
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_encode_long(dtype):
    """W = 1: scale_factor * z_mu's bytes (eegldm_edit_start on the encoder's posterior mean); m = r = 0: the per-window encodes side by
    side; otherwise the owner window's latent outside the ramps, bit for bit, and within 1 ulp of _long_crossfade inside -- the standard
    of test_compose_crossfades_decoded_windows (tests/test_gpu_long.py)."""
    import gpu_util as G
    from eegldm.sampling import _long_crossfade, encode_long
    ae = _ae(702, dtype)
    sf, L, R = 0.7, 64, 2
    for W, m, r in ((1, 4, 8), (3, 0, 0), (3, 4, 8), (5, 3, 5)):
        lay = _lay(W, L, m, r)
        big = lay.scaled(4)
        rec = torch.from_numpy(normal((R, 1, big.canvas_len), seed=703 + W + m)).to(G.DEV) * 0.5
        z0 = encode_long(ae, rec, lay, sf)
        assert z0.shape == (R, 1, lay.canvas_len)
        z_mu, _s = ae.encode(_slices(rec, big).contiguous())
        rows = torch.empty_like(z_mu)
        G.check(G.lib.eegldm_edit_start(G.ctx().h, G.ptr(z_mu.contiguous()), sf, None, 1.0, G.ptr(rows), None, rows.numel()))
        rows = rows.reshape(R, W, 1, L)
        if W == 1:
            assert torch.equal(z0, rows[:, 0])
        if m == 0 and r == 0:
            assert torch.equal(z0, rows.permute(0, 2, 1, 3).reshape(R, 1, W * L))
        ref = _long_crossfade(rows, lay)
        ramp = torch.zeros(lay.canvas_len, dtype=torch.bool)
        for a, b in lay.seams():
            ramp[a:b] = True
        assert torch.equal(z0[:, :, ~ramp], ref[:, :, ~ramp])
        ulp = torch.from_numpy(np.spacing(np.abs(ref.cpu().numpy()))).double()
        assert ((z0.cpu().double() - ref.cpu().double()).abs() <= ulp).all()
        assert torch.equal(encode_long(ae, rec, lay, sf), z0)
        assert torch.equal(encode_long(ae, rec, lay, sf, native=False)[:, :, ~ramp], z0[:, :, ~ramp])
    with pytest.raises(ValueError, match="expected"):
        encode_long(ae, rec[:, :, :-4], lay, sf)


# ------------------------------------------------------------------ 3. the native loop
def _rec_mask(R, n, seed=0):
    """keep-mask (R, 1, n): a regenerated span that crosses a window boundary, plus scattered regenerated samples (the min-pool matters)"""
    m = torch.ones(R, 1, n)
    m[:, :, n // 3: n // 3 + n // 4 + 1] = 0.0
    for b in range(R):
        for t in (3 + b, n // 2 + 1 + 2 * b + seed, n - 6 - b):
            m[b, 0, t] = 0.0
    return m


def _tables(tab):
    i64, f32 = (lambda v: (C.c_int64 * len(v))(*v)), (lambda v: (C.c_float * len(v))(*v))
    return i64(tab["timesteps"]), f32(tab["a_t"]), f32(tab["cx"]), f32(tab["c0"]), f32(tab["c1"]), f32(tab["a_next"])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("order", [1, 2])
def test_native_loop_is_the_plain_long_loop_and_the_one_window_edit_loop(order, graph):
    """known = NULL: eegldm_sample_long_edit returns eegldm_sample_long's bytes (canvas and recording).  W = 1 (with a margin and a ramp
    that then touch nothing): sample_long(init=, mask=) returns the latents and window bytes of sample(init=, mask=) (eegldm_sample_edit,
    multistep form), composite included, at strength 0.5 and 1."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample, sample_long
    from eegldm.schedulers import scheduler_edit_tables
    _cfg, _sd, net = _tiny(711)
    ae = _ae(712)
    L, W = 64, 3
    sched = make_sampling_scheduler(5, sampler="dpmpp_2m", solver_order=order)
    lay = _lay(W, L, 4, 8)
    noise = torch.from_numpy(normal((2, 1, lay.canvas_len), seed=713)).to(G.DEV)
    rec, cv = sample_long(net, ae, sched, noise, W, margin=4, ramp=8, scale_factor=0.7, crop=0, use_graph=graph)
    ts, a_t, cx, c0, c1, a_next = _tables(scheduler_edit_tables(sched, 1.0))
    cv2, rec2, used = torch.empty_like(cv), torch.empty_like(rec), C.c_int(0)
    G.check(G.lib.eegldm_sample_long_edit(net.h, ae.h, G.ptr(noise), None, None, ts, a_t, cx, c0, c1, a_next, 5, 0, 0, 1.0 / 0.7, G.ptr(cv2), G.ptr(rec2),
                                          2, W, L, 4, 8, int(graph), C.byref(used), None, 1.0, 0))
    assert torch.equal(cv2, cv) and torch.equal(rec2, rec) and bool(used.value) == graph
    # a mask without the known signal is refused
    assert G.lib.eegldm_sample_long_edit(net.h, ae.h, G.ptr(noise), None, G.ptr(noise), ts, a_t, cx, c0, c1, a_next, 5, 0, 0, 1.0, G.ptr(cv2), None, 2, W, L,
                                         4, 8, 0, None, None, 1.0, 0) != 0
    B = 1
    noise1 = torch.from_numpy(normal((B, 1, L), seed=714)).to(G.DEV)
    init = torch.from_numpy(normal((B, 1, 4 * L), seed=715)) * 0.5
    for kw in (dict(strength=0.5), dict(strength=0.5, mask=_rec_mask(B, 4 * L)), dict(strength=1.0, mask=_rec_mask(B, 4 * L))):
        win, z = sample(net, ae, sched, noise1, scale_factor=0.7, crop=8, use_graph=graph, init=init, **kw)
        info = {}
        rec1, cv1 = sample_long(net, ae, sched, noise1, 1, margin=4, ramp=8, scale_factor=0.7, crop=8, use_graph=graph, init=init, info=info, **kw)
        assert info["graph"] == graph and info["n_run"] == (5 if kw["strength"] == 1.0 else 3)
        assert torch.equal(cv1, z) and torch.equal(rec1, win), kw.keys()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("R,W", [(1, 5), (2, 3)])
def test_native_loop_matches_hostloop_ldm(R, W, dtype, graph, order):
    """sample_long(init=, mask=) (eegldm_sample_long_edit) against sample_long_hostloop -- the encode per window and its cross-fade, the
    noised start, slicing, model, x0, taper, update, blend, decode per window, cross-fade and composite in torch -- with the 5e-5
    relative-L2 bound tests/test_gpu_long.py and tests/test_gpu_edit.py hold their loops to: LDM with z / scale_factor, (m, r) = (4, 8),
    6 steps; init only at strength 0.5, init + mask at strength 0.5 and 1, mask_erode 5 at strength 1.  Two native runs are bit-identical;
    the composite's kept samples are the input's bytes."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample_long, sample_long_hostloop
    _cfg, _sd, net = _tiny(721, dtype)
    ae = _ae(722, dtype)
    L = 64
    lay = _lay(W, L, 4, 8)
    n = 4 * lay.canvas_len
    noise = torch.from_numpy(normal((R, 1, lay.canvas_len), seed=723))
    init = torch.from_numpy(normal((R, 1, n), seed=724)) * 0.5
    sched = make_sampling_scheduler(6, sampler="dpmpp_2m", solver_order=order)
    base = dict(margin=4, ramp=8, scale_factor=0.7, crop=8, init=init)
    for name, kw in (("init s=0.5", dict(strength=0.5)), ("init + mask s=0.5", dict(strength=0.5, mask=_rec_mask(R, n))),
                     ("init + mask s=1", dict(strength=1.0, mask=_rec_mask(R, n))), ("init + mask s=1 erode 5", dict(mask=_rec_mask(R, n), mask_erode=5))):
        info = {}
        rec, cv = sample_long(net, ae, sched, noise, W, use_graph=graph, info=info, **base, **kw)
        assert info["graph"] == graph
        assert rec.shape == (R, 1, n - 16) and cv.shape == (R, 1, lay.canvas_len) and torch.isfinite(rec).all()
        rec2, cv2 = sample_long(net, ae, sched, noise, W, use_graph=graph, **base, **kw)
        assert torch.equal(cv2, cv) and torch.equal(rec2, rec)
        rech, cvh = sample_long_hostloop(net, ae, sched, noise, W, **base, **kw)
        print(f"{dtype} R={R} W={W} graph={graph} order={order} {name}: canvas rel-L2 {G.rel_l2(cv, cvh):.3e}, recording {G.rel_l2(rec, rech):.3e}")
        assert G.rel_l2(cv, cvh) < 5e-5 and G.rel_l2(rec, rech) < 5e-5
        if "mask" in kw:
            keep = kw["mask"][:, :, 8:-8].to(rec.device) == 1.0
            assert torch.equal(rec[keep], init[:, :, 8:-8].to(rec.device)[keep])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("R,W", [(1, 5), (2, 3)])
def test_native_loop_matches_hostloop_conditional_and_guided_pixel_space(R, W, graph, order):
    """Class-conditional fp32 UNet, pixel-space call (autoencoder=None: init and mask at the canvas's resolution, the composite on the
    canvas), (m, r) = (3, 5) (odd stride): plain conditional at strength 0.5 and guided (w = 3) at strength 1, both with a mask, against
    the host loop (5e-5 as above); guidance changes the result; repeats are bit-identical."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample_long, sample_long_hostloop
    _cfg, _sd, net = _tiny(731, num_classes=3)
    L = 64
    lay = _lay(W, L, 3, 5)
    Lc = lay.canvas_len
    noise = torch.from_numpy(normal((R, 1, Lc), seed=732))
    init = torch.from_numpy(normal((R, 1, Lc), seed=733)) * 0.6
    mask = _rec_mask(R, Lc)
    lab = [2, 0, 1, 2, 0, 1][:R * W]
    sched = make_sampling_scheduler(6, sampler="dpmpp_2m", solver_order=order)
    kw = dict(margin=3, ramp=5, crop=4, init=init, mask=mask, labels=lab)
    rec, cv = sample_long(net, None, sched, noise, W, use_graph=graph, strength=0.5, **kw)
    keep = (mask == 1.0).to(cv.device)
    assert rec.shape == (R, 1, Lc - 8) and torch.equal(rec, cv[:, :, 4:-4]) and torch.equal(cv[keep], init.to(cv.device)[keep])
    _r, cvh = sample_long_hostloop(net, None, sched, noise, W, strength=0.5, **kw)
    g = dict(guidance_scale=3.0, null_class=1)
    _r, cvg = sample_long(net, None, sched, noise, W, use_graph=graph, **g, **kw)
    _r, cvgh = sample_long_hostloop(net, None, sched, noise, W, **g, **kw)
    print(f"R={R} W={W} graph={graph} order={order}: conditional rel-L2 {G.rel_l2(cv, cvh):.3e}, guided {G.rel_l2(cvg, cvgh):.3e}")
    assert G.rel_l2(cv, cvh) < 5e-5 and G.rel_l2(cvg, cvgh) < 5e-5
    _r, cvp = sample_long(net, None, sched, noise, W, use_graph=graph, **kw)
    assert G.rel_l2(cvg, cvp) > 1e-3
    assert torch.equal(sample_long(net, None, sched, noise, W, use_graph=graph, **g, **kw)[1], cvg)
    assert torch.equal(sample_long(net, None, sched, noise, W, use_graph=graph, init_canvas=init, **g, **{k: v for k, v in kw.items() if k != "init"},
                                   composite=False)[1], cvg)


@pytest.mark.parametrize("graph", [False, True])
def test_exact_properties_of_masks_on_the_canvas(graph):
    """fp32 LDM, (R, W) = (2, 3), (m, r) = (4, 8), 6 steps of 2M; the last step lands on final_alpha_cumprod = 1, so k = z0 there.
      * an all-one mask returns z0 = encode_long(...) as the canvas and, composited, the input's bytes;
      * an all-zero mask equals the run with init only (canvas and recording);
      * with a kept span the final canvas holds z0 there bit for bit, and the regenerated positions differ from z0;
      * the continuation case -- mask 1 on the first W0 = 2 windows' samples, 0 beyond, init zero there: the kept latents equal z0, the
        composite's kept samples are the input's bytes, and the extension does not depend on what init holds where the mask is 0 at
        strength 1 ... except through the encoder: latents beside the boundary are contaminated, which is what mask_erode is for."""
    import gpu_util as G
    from eegldm.sampling import encode_long, make_sampling_scheduler, sample_long
    _cfg, _sd, net = _tiny(741)
    ae = _ae(742)
    R, W, L, sf = 2, 3, 64, 0.7
    lay = _lay(W, L, 4, 8)
    Lc, n = lay.canvas_len, 4 * lay.canvas_len
    noise = torch.from_numpy(normal((R, 1, Lc), seed=743)).to(G.DEV)
    init = (torch.from_numpy(normal((R, 1, n), seed=744)) * 0.5).to(G.DEV)
    sched = make_sampling_scheduler(6, sampler="dpmpp_2m")
    assert sched.final_alpha_cumprod == 1.0
    run = lambda **kw: sample_long(net, ae, sched, noise, W, margin=4, ramp=8, scale_factor=sf, crop=0, use_graph=graph, **kw)
    z0 = encode_long(ae, init, lay, sf)
    rec, cv = run(init=init, mask=torch.ones(R, 1, n), strength=0.5)
    assert torch.equal(cv, z0) and torch.equal(rec, init)
    raw, cv_r = run(init=init, mask=torch.ones(R, 1, n), strength=0.5, composite=False)
    assert torch.equal(cv_r, z0) and not torch.equal(raw, init)
    rec0, cv0 = run(init=init, mask=torch.zeros(R, 1, n), strength=0.5)
    reci, cvi = run(init=init, strength=0.5)
    assert torch.equal(cv0, cvi) and torch.equal(rec0, reci) and not torch.equal(cvi, z0)
    assert torch.equal(run(init_canvas=z0, strength=0.5)[1], cvi)
    mask = _rec_mask(R, n).to(G.DEV)
    recm, cvm = run(init=init, mask=mask)
    keep_lat = (-torch.nn.functional.max_pool1d(-mask, 4, 4)) == 1.0
    assert torch.equal(cvm[keep_lat], z0[keep_lat]) and (cvm[~keep_lat] != z0[~keep_lat]).float().mean() > 0.9
    assert torch.equal(recm[mask == 1.0], init[mask == 1.0]) and not torch.equal(recm[mask == 0.0], init[mask == 0.0])
    # continuation: the first two windows' samples are real, the rest is generated
    n0 = 4 * ((2 - 1) * lay.stride + L)
    cont, cmask = init.clone(), torch.zeros(R, 1, n, device=G.DEV)
    cont[:, :, n0:] = 0.0
    cmask[:, :, :n0] = 1.0
    z0c = encode_long(ae, cont, lay, sf)
    recc, cvc = run(init=cont, mask=cmask)
    assert torch.equal(cvc[:, :, :n0 // 4], z0c[:, :, :n0 // 4]) and torch.equal(recc[:, :, :n0], cont[:, :, :n0])
    assert torch.isfinite(recc).all() and float(recc[:, :, n0:].abs().max()) > 0
    rece, cve = run(init=cont, mask=cmask, mask_erode=16)
    assert torch.equal(cve[:, :, :n0 // 4 - 4], z0c[:, :, :n0 // 4 - 4]) and not torch.equal(cve[:, :, n0 // 4 - 4:n0 // 4], z0c[:, :, n0 // 4 - 4:n0 // 4])
    assert torch.equal(rece[:, :, :n0], cont[:, :, :n0])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        run(init=init, mask=torch.full((R, 1, n), 1.5))


def test_zero_network_gives_the_elementwise_recursion_with_the_blend():
    """All weights zero: the model output is 0, both windows of a ramp predict the same x0, so the canvas has to follow the plain recursion
    of step + blend element by element.  Outside the ramps: eegldm_edit_start and eegldm_edit_step (multistep form) applied to the
    canvas-shaped buffers, bit for bit.  Inside: the bound of test_zero_network_gives_the_elementwise_recursion (tests/test_gpu_long.py)
    for the step, E' = |cx| E + |c0| d0_i + |c1| d0_{i-1} + 6 u S, and through the blend E <- (1 - m) E' + 8 u (|m k| + |(1 - m) x'|): both
    sides blend with the same function (k is the same bytes), each with the blend's three roundings, 4 u allowed as in tests/test_gpu_edit.py."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample_long
    from eegldm.schedulers import scheduler_edit_tables
    _cfg, sd, net = _tiny(751)
    net.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()})
    R, W, L = 2, 3, 64
    lay = _lay(W, L, 4, 8)
    Lc = lay.canvas_len
    noise = torch.from_numpy(normal((R, 1, Lc), seed=752)).to(G.DEV)
    z0 = (torch.from_numpy(normal((R, 1, Lc), seed=753)) * 0.7).to(G.DEV)
    mask = _canvas_mask("fractional", lay, R, 1, 754)
    mask[:, :, :20] = 1.0
    mask[:, :, lay.stride + 6:lay.stride + 9] = 0.0                       # inside the first ramp: the blend's exact ends too
    mask = mask.to(G.DEV)
    sched = make_sampling_scheduler(6, sampler="dpmpp_2m")
    _rec, cv = sample_long(net, None, sched, noise, W, margin=4, ramp=8, crop=0, init=z0, mask=mask, strength=0.7)
    tab = scheduler_edit_tables(sched, 0.7)
    nn = noise.numel()
    x, hist, zero = torch.empty(nn, device=G.DEV), torch.zeros(nn, device=G.DEV), torch.zeros(nn, device=G.DEV)
    G.check(G.lib.eegldm_edit_start(G.ctx().h, G.ptr(z0), 1.0, G.ptr(noise), tab["a_t"][0], None, G.ptr(x), nn))
    E, d_prev, md = torch.zeros(nn, dtype=torch.float64), torch.zeros(nn, dtype=torch.float64), mask.double().cpu().reshape(-1)
    for i in range(len(tab["timesteps"])):
        a_t, a_next, cx, c0, c1 = (tab[k][i] for k in ("a_t", "a_next", "cx", "c0", "c1"))
        xd, hd = x.double().cpu(), hist.double().cpu()
        x0, plain = torch.empty_like(x), torch.empty_like(x)
        G.check(G.lib.eegldm_multistep_step(G.ctx().h, G.ptr(zero), 0.0, 0, G.ptr(x), G.ptr(hist.clone()), a_t, 0, 0, cx, c0, c1, G.ptr(plain), None,
                                            G.ptr(x0), nn))
        kd = torch.empty_like(x)
        G.check(G.lib.eegldm_edit_start(G.ctx().h, G.ptr(z0), 1.0, G.ptr(noise), a_next, None, G.ptr(kd), nn))
        G.check(G.lib.eegldm_edit_step(G.ctx().h, G.ptr(zero), 0.0, 0, G.ptr(x), G.ptr(hist), a_t, a_next, 0, 0, (C.c_float * 3)(cx, c0, c1), G.ptr(z0),
                                       G.ptr(noise), G.ptr(mask), G.ptr(x), None, None, nn))
        x0d = x0.double().cpu()
        d0 = E / a_t ** 0.5 + 5.0 * U24 * x0d.abs()
        S = (cx * xd).abs() + (c0 * x0d).abs() + (c1 * hd).abs()
        E = abs(cx) * E + abs(c0) * d0 + abs(c1) * d_prev + 6.0 * U24 * S
        E = (1.0 - md) * E + 8.0 * U24 * ((md * kd.double().cpu()).abs() + ((1.0 - md) * plain.double().cpu()).abs())
        d_prev = d0
    ramp = torch.zeros(Lc, dtype=torch.bool)
    for a, b in lay.seams():
        ramp[a:b] = True
    got, want = cv.cpu().reshape(R, Lc), x.cpu().reshape(R, Lc)
    assert torch.equal(got[:, ~ramp], want[:, ~ramp])
    err = (got.double() - want.double()).abs()
    print(f"zero network: max |canvas - recursion| inside the ramps {float(err[:, ramp].max()):.3e}, bound {float(E.reshape(R, -1)[:, ramp].max()):.3e}")
    assert (err <= E.reshape(R, -1)).all()
    assert float(want.abs().max()) > 0.1


# ------------------------------------------------------------------ 4. entry script
def test_entry_script_repairs_and_extends_a_recording(tmp_path):
    """edit_long.py on the tiny seeded checkpoints of the entry-script pin, 4 steps, margin 100 / ramp 150 latents (stride 1672 samples):
    an input of 2 windows plus 50 samples; --mask_span keeps everything outside the span bit for bit and writes the mask; --extend_minutes
    appends windows behind the kept input; the layout file is the one tools/seam_report.py reads; the pixel-space twin."""
    import entry_pin_case as E
    from eegldm.entry import edit_long as EL
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import seam_report as SR
    out = str(tmp_path)
    a_yaml, l_yaml, run_a, run_l, run_d = E.write_checkpoints(out)
    ldm = ["--output_dir", out, "--num_inference_steps", "4", "--best_model_path", run_a, "--diffusion_path", run_l,
           "--autoencoderkl_config_file_path", a_yaml, "--ldm_config_file_path", l_yaml, "--latent_channels", "1", "--margin", "100", "--ramp", "150"]
    dm = ["--output_dir", out, "--num_inference_steps", "4", "--pixel", "--config_file", l_yaml, "--diffusion_path", run_d, "--margin", "400",
          "--ramp", "600"]
    S = 3072 - 1400
    n = 3000 + S + 50
    x_in = (normal((n,), seed=95) * 0.3).astype(np.float32)
    inp = os.path.join(out, "recording.npy")
    np.save(inp, x_in)

    def run(base, *extra, seed=0):
        d = EL.main(EL.parse_args(base + ["--input", inp, "--seed", str(seed)] + list(extra)))
        return (np.load(os.path.join(d, f"edit_long_{seed}.npy")), np.load(os.path.join(d, f"edit_long_{seed}_mask.npy")),
                json.load(open(os.path.join(d, f"edit_long_{seed}_layout.json"))), os.path.join(d, f"edit_long_{seed}"))

    for base, down, m, r in ((ldm, 4, 100, 150), (dm, 1, 400, 600)):
        used = 3000 + S
        a, b = 2900, 3300                                   # crosses the boundary of the first 30-s window
        rec, mk, lj, stem = run(base, "--mask_span", f"{a}:{b}", "--strength", "0.75")
        lay = _lay(2, 3072 // down, m, r).scaled(down)
        assert rec.shape == mk.shape == (1, 1, used) and rec.dtype == np.float32 and np.isfinite(rec).all()
        assert lj["samples"] == used and lj["n_windows"] == 2 and lj["S"] == lay.stride and lj["left_out"] == 50 and lj["input_samples"] == n
        assert lj["seams"] == [[s - 36, e - 36] for s, e in lay.seams()]
        keep = np.ones(used, bool); keep[a:b] = False
        assert np.array_equal(mk[0, 0] == 1.0, keep)
        assert rec[0, 0, keep].tobytes() == x_in[:used][keep].tobytes() and not np.array_equal(rec[0, 0, ~keep], x_in[:used][~keep])
        rep = SR.seam_report(rec, lj)
        assert len(rep["seams"]) == 1 and rep["seams"][0]["span"] == lj["seams"][0] and np.isfinite(rep["seams"][0]["ratio_diff_rms"])
        assert SR.main([stem + ".npy", stem + "_layout.json", "--json"]) == rep
        again, _m, _j, _s = run(base, "--mask_span", f"{a}:{b}", "--strength", "0.75")
        assert again.tobytes() == rec.tobytes()
        ext, mke, lje, _s = run(base, "--extend_minutes", "0.2")
        assert lje["n_windows"] == 3 and lje["kept_windows"] == 2 and ext.shape == (1, 1, used + S)
        assert ext[0, 0, :used].tobytes() == x_in[:used].tobytes() and np.isfinite(ext).all() and float(np.abs(ext[0, 0, used:-36]).max()) > 0
        assert (mke[0, 0, :used] == 1).all() and (mke[0, 0, used:] == 0).all()
        var, mkv, _j, _s = run(base, "--strength", "0.5")
        assert var.shape == (1, 1, used) and not np.array_equal(var, x_in[None, None, :used]) and (mkv == 0).all()
