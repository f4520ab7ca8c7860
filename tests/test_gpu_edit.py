"""-m gpu: sampling from an input with a keep-mask -- eegldm_edit_step against the float64 recursion, the start and window kernels, the
native loop (eegldm_sample_edit) against the host loop, the exact properties of the whole loop, what strength means on the closed-form
Gaussian denoiser, and the entry script."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from make_golden_cases import UNET_CASES  # noqa: E402
from param_gen import gen_param, normal  # noqa: E402
from test_gpu_dpm_solver import SCHED, U24, _ae, _carve, _step_reference, _tiny  # noqa: E402

NUL = C.POINTER(C.c_float)()


def _coef(*v):
    return (C.c_float * 3)(*v)


def _f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------ 1. one step against the float64 recursion
def _ddim_reference(mo, w, guided, x, a_t, a_prev, pred, clip):
    """float64 restatement of the DDIM (eta 0) step -> (prev, x0, prev bound); the bound is the docstring's of test_edit_step."""
    mo, x = mo.double(), x.double()
    n = x.numel()
    sa, sb, sap, sbp = a_t ** 0.5, (1.0 - a_t) ** 0.5, a_prev ** 0.5, (1.0 - a_prev) ** 0.5
    if guided:
        oc, ou = mo[:n], mo[n:]
        o = ou + w * (oc - ou)
        mix = 3.0 * U24 * (abs(w) * (oc - ou).abs() + o.abs())
    else:
        o, mix = mo, torch.zeros_like(x)
    if pred == "epsilon":
        x0, dxdo = (x - sb * o) / sa, sb / sa
        e, e_tol = o, mix
    elif pred == "v_prediction":
        x0, dxdo = sa * x - sb * o, sb
        e = sa * o + sb * x
        e_tol = 5.0 * U24 * ((sa * o).abs() + (sb * x).abs()) + sa * mix
    else:
        x0, dxdo = o, 1.0
        e = (x - sa * x0) / sb
        e_tol = 5.0 * U24 * (x.abs() + (sa * x0).abs()) / sb + (sa / sb) * mix
    x0_tol = 2e-5 * x0.abs() + 2e-5 + dxdo * mix
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    prev = sap * x0 + sbp * e
    tol = 5.0 * U24 * ((sap * x0).abs() + (sbp * e).abs()) + sap * x0_tol + sbp * e_tol
    return prev, x0, tol


LAYOUTS = {"aligned": [0] * 9, "all+4B": [1] * 9, "all+8B": [2] * 9, "mixed": [0, 1, 2, 3, 0, 2, 1, 3, 2]}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1023, 2052])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
def test_edit_step_vs_float64_recursion(pred, clip, guided, n, layout):
    """eegldm_edit_step, DDIM form and multistep form (c1 = 0 and c1 != 0), masks {all 0, all 1, random 0/1, random fractional}, against
    the float64 recursion  x' = step(...),  k = sqrt(a_next) z0 + sqrt(1 - a_next) noise,  out = m k + (1 - m) x'.

    Bound, from the operation count (u = 2^-24, one float32 rounding):
      * x', multistep form: the bound of test_single_step_vs_float64_recursion (tests/test_gpu_dpm_solver.py: 4 u S + |c0| x0_tol).
      * x', DDIM form: sqrt(a') x0 + sqrt(1 - a') e is two products and a sum (or a product and an fma) of two rounded sqrtf: 5 u
        (|a' x0| + |s' e|), the count tests/test_gpu_dpm_solver.py uses for the DDIM step; x0 carries that file's x0_tol (rtol 2e-5, atol
        2e-5, plus the guided mix's 3 u (|w| |o_c - o_u| + |o|) times |d x0 / d o|) and enters times sqrt(a'); e enters times sqrt(1 - a'):
        e = o for epsilon (the mix error alone), sa o + sb x for v (5 u (|sa o| + |sb x|) by the same count, plus sa x mix), (x - sa x0) /
        sb for sample (product, difference, quotient, two rounded sqrtf: 5 u (|x| + |sa x0|) / sb, plus (sa / sb) x mix).
      * k = fma(ka, z0, kb * noise): two roundings of values no larger than K = |ka z0| + |kb noise|, and ka, kb are each a rounded
        sqrtf (one u on each term): |d k| <= 3 u K.  4 u K is allowed.  a_next == 1: k = z0, no rounding at all.
      * the blend fma(m, k, (1 - m) * x'): 1 - m, the product and the fma are three roundings of values no larger than
        |m k| + |(1 - m) x'|: 3 u of that, 4 u allowed; the operands' own errors enter as m |d k| + (1 - m) |d x'|.
    m == 0 and m == 1 are asserted bit for bit instead (against the unblended step and against eegldm_edit_start's x_start).  Also:
    prev2 == prev, hist == pred_x0 == the plain step's x0, inputs unwritten, prev over sample == separate prev, mask = NULL == the
    existing eegldm_ddim_step / eegldm_multistep_step bit for bit.  Sizes and layouts as in that file, the three new
    inputs included: n = 1023 (scalar loop when guided), n = 2052 (float4 body with the layout's head / tail), mixed offsets (scalar)."""
    import gpu_util as G
    from eegldm.schedulers import PRED
    lib, ctx = G.lib, G.ctx()
    offs = LAYOUTS[layout]
    w = 3.0
    forms = [("ddim", 0.0123, 0.0456, None), ("ddim", 0.97, 1.0, None), ("ms", 0.31, 0.52, (0.78, 0.9, -0.37)), ("ms", 0.0123, 0.05, (0.93, 0.41, 0.0)),
             ("ms", 0.97, 1.0, (0.0, 1.0, 0.0))]
    worst = 0.0
    for case, (form, a_t, a_next, cf) in enumerate(forms):
        a_t, a_next = _f32(a_t), _f32(a_next)
        cf = None if cf is None else tuple(_f32(v) for v in cf)
        mo_h = torch.from_numpy(normal((2 * n if guided else n,), seed=100 + case)) * (0.6 if pred == "sample" else 1.0)
        x_h, h_h = torch.from_numpy(normal((n,), seed=200 + case)), torch.from_numpy(normal((n,), seed=300 + case)) * 0.8
        z_h, nz_h = torch.from_numpy(normal((n,), seed=400 + case)) * 0.7, torch.from_numpy(normal((n,), seed=500 + case))
        rnd = torch.from_numpy(np.random.default_rng(600 + case).random(n).astype(np.float32))
        masks = {"zeros": torch.zeros(n), "ones": torch.ones(n), "binary": (rnd > 0.5).float(), "fractional": rnd}
        mo, x, hist = _carve(mo_h, mo_h.numel(), offs[0]), _carve(x_h, n, offs[1]), _carve(h_h, n, offs[2])
        known, noise = _carve(z_h, n, offs[6]), _carve(nz_h, n, offs[7])
        cptr = NUL if cf is None else _coef(*cf)

        def call(xb, hb, pb, p2, zb, mb):
            G.check(lib.eegldm_edit_step(ctx.h, G.ptr(mo), w, int(guided), G.ptr(xb), G.ptr(hb), a_t, a_next, PRED[pred], int(clip), cptr,
                                         G.ptr(known), G.ptr(noise), G.ptr(mb), G.ptr(pb), G.ptr(p2), G.ptr(zb), n))
        # the unblended step: mask = NULL, against the existing kernels bit for bit
        plain, plain0 = _carve(None, n, offs[3]), _carve(None, n, offs[5])
        hist0 = _carve(h_h, n, offs[2])
        call(x, hist0, plain, None, plain0, None)
        old, old0, hist1 = torch.empty(n, device=G.DEV), torch.empty(n, device=G.DEV), h_h.to(G.DEV).clone()
        if cf is not None:
            G.check(lib.eegldm_multistep_step(ctx.h, G.ptr(mo), w, int(guided), G.ptr(x), G.ptr(hist1), a_t, PRED[pred], int(clip), *cf, G.ptr(old),
                                              None, G.ptr(old0), n))
            assert torch.equal(plain0, old0)
            assert torch.equal(plain, old), f"{form}: mask = NULL differs from eegldm_multistep_step"
        elif not guided:
            G.check(lib.eegldm_ddim_step(ctx.h, G.ptr(mo), G.ptr(x), a_t, a_next, PRED[pred], int(clip), G.ptr(old), G.ptr(old0), n))
            assert torch.equal(plain0, old0)
            assert torch.equal(plain, old), f"{form}: mask = NULL differs from eegldm_ddim_step"
        # (guided DDIM has no counterpart among the two: eegldm_guided_step shares its update with the ancestral step and the compiler
        # contracts it differently; the float64 bound below holds for that form like for the others)
        assert torch.equal(hist0, plain0)
        # the re-noised known value by the start kernel's formula
        kdev = _carve(None, n, offs[3])
        G.check(lib.eegldm_edit_start(ctx.h, G.ptr(known), 1.0, G.ptr(noise), a_next, None, G.ptr(kdev), n))
        if cf is None:
            rp, r0, tolp = _ddim_reference(mo_h, w, guided, x_h, a_t, a_next, pred, clip)
        else:
            rp, r0, _t0, tolp = _step_reference(mo_h, w, guided, x_h, h_h, a_t, pred, clip, *cf)
        ka, kb = a_next ** 0.5, (1.0 - a_next) ** 0.5
        rk = ka * z_h.double() + kb * nz_h.double()
        tolk = 4.0 * U24 * ((ka * z_h.double()).abs() + (kb * nz_h.double()).abs()) if a_next < 1.0 else torch.zeros(n, dtype=torch.float64)
        ek = (kdev.cpu().double() - rk).abs()
        assert (ek <= tolk).all(), float((ek / tolk).max())
        if a_next == 1.0:
            assert torch.equal(kdev, known)
        for mname, m_h in masks.items():
            mask = _carve(m_h, n, offs[8])
            hist2 = _carve(h_h, n, offs[2])
            prev, prev2, x0 = _carve(None, n, offs[3]), _carve(None, n, offs[4]), _carve(None, n, offs[5])
            call(x, hist2, prev, prev2, x0, mask)
            md = m_h.double()
            ref = md * rk + (1.0 - md) * rp
            tol = 4.0 * U24 * ((md * rk).abs() + ((1.0 - md) * rp).abs()) + md * tolk + (1.0 - md) * tolp
            err = (prev.cpu().double() - ref).abs()
            worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
            assert (err <= tol).all(), (form, mname, float((err / tol).max()))
            assert torch.equal(prev2, prev)
            assert torch.equal(hist2, x0) and torch.equal(x0, plain0), "the history / pred_x0 must hold the model's own x0"
            for buf, host in ((x, x_h), (mo, mo_h), (known, z_h), (noise, nz_h), (mask, m_h)):
                assert torch.equal(buf, host.to(G.DEV)), "an input was written"
            if mname == "zeros":
                assert torch.equal(prev, plain)
            if mname == "ones":
                assert torch.equal(prev, kdev)
            if mname == "binary":
                assert torch.equal(prev, torch.where(mask == 1.0, kdev, plain))
            # prev over sample; nullable outputs left out
            x2, hist3 = _carve(x_h, n, offs[1]), _carve(h_h, n, offs[2])
            call(x2, hist3, x2, None, None, mask)
            assert torch.equal(x2, prev) and torch.equal(hist3, x0)
            if cf is None or cf[2] == 0.0:          # no history needed
                x3, p3 = _carve(x_h, n, offs[1]), _carve(None, n, offs[3])
                call(x3, None, p3, None, None, mask)
                assert torch.equal(p3, prev)
    print(f"{pred} clip={clip} guided={guided} n={n} {layout}: worst err / tol {worst:.3f}")


def test_edit_step_argument_checks():
    import gpu_util as G
    lib, ctx = G.lib, G.ctx()
    n = 64
    mo, x, hist, prev, kn, nz, m = (torch.zeros(n, device=G.DEV) for _ in range(7))
    p = G.ptr
    ok = lambda *a: lib.eegldm_edit_step(ctx.h, *a)
    assert ok(p(mo), 0.0, 0, p(x), p(hist), 0.5, 0.6, 0, 0, NUL, p(kn), p(nz), p(m), p(prev), None, None, n) == 0
    assert ok(p(mo), 0.0, 0, p(x), None, 0.5, 0.6, 0, 0, NUL, None, None, None, p(prev), None, None, n) == 0
    assert ok(p(mo), 0.0, 0, p(x), None, 0.5, 0.6, 0, 0, NUL, None, p(nz), p(m), p(prev), None, None, n) != 0          # mask without known
    assert ok(p(mo), 0.0, 0, p(x), None, 0.5, 0.6, 0, 0, _coef(1.0, 1.0, 0.5), p(kn), p(nz), p(m), p(prev), None, None, n) != 0      # c1 without history
    assert ok(p(mo), 0.0, 0, p(x), None, 0.5, 0.0, 0, 0, NUL, p(kn), p(nz), p(m), p(prev), None, None, n) != 0         # a_next = 0
    assert ok(p(mo), 0.0, 0, p(x), None, 0.5, 0.6, 0, 0, NUL, p(kn), p(nz), p(prev), p(prev), None, None, n) != 0      # mask over prev
    assert ok(p(mo), 0.0, 0, p(x), None, 0.5, 0.6, 0, 0, NUL, p(x), p(nz), p(m), p(x), None, None, n) != 0             # known over an in-place prev
    assert ok(p(mo), 0.0, 0, p(x), None, 0.5, 0.6, 3, 0, NUL, p(kn), p(nz), p(m), p(prev), None, None, n) != 0
    assert ok(p(mo), 0.0, 0, p(x), None, 0.5, 0.6, 0, 0, NUL, p(kn), p(nz), p(m), p(prev), None, None, 0) == 0


# ------------------------------------------------------------------ 2. start and window kernels
@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 2, 3)])
@pytest.mark.parametrize("n", [1, 1023, 2052])
def test_edit_start_vs_float64(n, offs):
    """z0 = sf * z_mu is one product: |d z0| <= u |z0|.  x = fma(ka, z0, kb * noise) with ka, kb rounded sqrtf: the product and the fma
    are the 2 roundings of values no larger than K = |ka z0| + |kb noise| the bound names; the two rounded sqrtf add one u on each term
    and z0's own rounding enters times ka -- together at most 4 u K."""
    import gpu_util as G
    lib, ctx = G.lib, G.ctx()
    zm_h, nz_h = torch.from_numpy(normal((n,), seed=11)), torch.from_numpy(normal((n,), seed=12))
    for sf, a in ((0.8125, 0.31), (1.0, 0.0123), (1.7, 1.0), (1.0, 1.0)):
        a = _f32(a)
        zm, nz = _carve(zm_h, n, offs[0]), _carve(nz_h, n, offs[1])
        z0, xs = _carve(None, n, offs[2]), _carve(None, n, offs[3])
        G.check(lib.eegldm_edit_start(ctx.h, G.ptr(zm), sf, G.ptr(nz), a, G.ptr(z0), G.ptr(xs), n))
        rz = _f32(sf) * zm_h.double()
        assert ((z0.cpu().double() - rz).abs() <= U24 * rz.abs()).all()
        ka, kb = a ** 0.5, (1.0 - a) ** 0.5
        rx = ka * rz + kb * nz_h.double()
        K = (ka * rz).abs() + (kb * nz_h.double()).abs()
        assert ((xs.cpu().double() - rx).abs() <= 4.0 * U24 * K).all()
        if sf == 1.0:
            assert torch.equal(z0, zm)
        if a == 1.0:
            assert torch.equal(xs, z0)
        assert torch.equal(zm, zm_h.to(G.DEV)) and torch.equal(nz, nz_h.to(G.DEV))
        only = _carve(None, n, offs[2])
        G.check(lib.eegldm_edit_start(ctx.h, G.ptr(zm), sf, None, 1.0, G.ptr(only), None, n))
        assert torch.equal(only, z0)
        only_x = _carve(None, n, offs[3])
        G.check(lib.eegldm_edit_start(ctx.h, G.ptr(zm), sf, G.ptr(nz), a, None, G.ptr(only_x), n))
        assert torch.equal(only_x, xs)


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("B,C_lat,Co,Lw,down", [(1, 1, 1, 256, 4), (3, 1, 1, 3072, 4), (5, 3, 2, 96, 4), (7, 2, 1, 64, 1), (2, 1, 1, 48, 8)])
def test_edit_window_minpool_and_composite(B, C_lat, Co, Lw, down, off):
    """The pooled mask == -max_pool1d(-mask) exactly, every latent channel the same row; the composite: kept samples are the input's
    bytes, regenerated ones the decode's, fractional ones fma(m, input, (1 - m) * decoded) within 4 u (|m input| + |(1 - m) decoded|)
    (three roundings); in place over `decoded` == out of place.  Odd batch sizes, views 4 and 12 bytes past a 16-byte line."""
    import gpu_util as G
    lib, ctx = G.lib, G.ctx()
    rng = np.random.default_rng(B * 100 + Lw)
    for kind in ("binary", "fractional"):
        r = rng.random((B, 1, Lw)).astype(np.float32)
        m_h = torch.from_numpy((r > 0.3).astype(np.float32) if kind == "binary" else np.where(r < 0.2, 0.0, np.where(r > 0.8, 1.0, r)).astype(np.float32))
        m_h[0, 0, : Lw // 2] = 1.0                        # a run of kept samples, so that some latent positions are kept
        x_h, d_h = torch.from_numpy(normal((B, Co, Lw), seed=21)), torch.from_numpy(normal((B, Co, Lw), seed=22))
        m, x, d = (_carve(t.reshape(-1), t.numel(), off).view(t.shape) for t in (m_h, x_h, d_h))
        ml = _carve(None, B * C_lat * (Lw // down), off).view(B, C_lat, Lw // down)
        out = _carve(None, B * Co * Lw, off).view(B, Co, Lw)
        G.check(lib.eegldm_edit_window(ctx.h, G.ptr(m), B, Lw, down, C_lat, G.ptr(ml), G.ptr(x), G.ptr(d), Co, G.ptr(out)))
        want = (-torch.nn.functional.max_pool1d(-m_h, down, down)).expand(B, C_lat, Lw // down)
        assert torch.equal(ml.cpu(), want)
        assert float(ml.sum()) > 0
        o, mm = out.cpu(), m_h.expand(B, Co, Lw)
        assert torch.equal(o[mm == 1.0], x_h[mm == 1.0]) and torch.equal(o[mm == 0.0], d_h[mm == 0.0])
        md = mm.double()
        ref = md * x_h.double() + (1 - md) * d_h.double()
        assert ((o.double() - ref).abs() <= 4.0 * U24 * ((md * x_h.double()).abs() + ((1 - md) * d_h.double()).abs())).all()
        for buf, host in ((m, m_h), (x, x_h), (d, d_h)):
            assert torch.equal(buf.cpu(), host), "an input was written"
        G.check(lib.eegldm_edit_window(ctx.h, G.ptr(m), B, Lw, down, 0, None, G.ptr(x), G.ptr(d), Co, G.ptr(d)))
        assert torch.equal(d, out)
        ml2 = torch.empty(B, C_lat, Lw // down, device=G.DEV)
        G.check(lib.eegldm_edit_window(ctx.h, G.ptr(m), B, Lw, down, C_lat, G.ptr(ml2), None, None, 0, None))
        assert torch.equal(ml2, ml)


# ------------------------------------------------------------------ 3. native loop against the host loop
def _span_mask(B, Lw, down):
    """keep-mask (B, 1, Lw): a contiguous regenerated span plus a few scattered regenerated samples (each of which knocks out the whole
    latent position it falls in: the min-pool matters)"""
    m = torch.ones(B, 1, Lw)
    m[:, :, Lw // 4: Lw // 4 + Lw // 5 + 1] = 0.0
    for b in range(B):
        for t in (3 + b, Lw // 2 + 1 + 2 * b, Lw - 6 - b):
            m[b, 0, t] = 0.0
    return m


def _edit_variants(B, Lw, down):
    return [("init s=0.5", dict(strength=0.5)), ("init + mask s=0.5", dict(strength=0.5, mask=_span_mask(B, Lw, down))),
            ("init + mask s=1", dict(strength=1.0, mask=_span_mask(B, Lw, down))), ("init s=1", dict(strength=1.0))]


@pytest.mark.parametrize("sampler,steps", [("ddim", 10), ("dpmpp_2m", 12), ("dpmpp_2m", 16)])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("dtype,case,B", [("float32", "tiny_l64", 1), ("float32", "tiny_l64", 5), ("bfloat16", "tiny_l64", 1),
                                          ("bfloat16", "small_l256", 128)])
def test_native_loop_matches_hostloop_unconditional(dtype, case, B, graph, sampler, steps):
    """sample(init=...) (eegldm_sample_edit) against ddim_sample_hostloop(init=...) -- scheduler.step per timestep, the start, the blend,
    the pooled mask and the composite in torch -- on the cases and with the 5e-5 relative-L2 bound of
    test_native_loop_matches_hostloop_unconditional in tests/test_gpu_dpm_solver.py: LDM with z / scale_factor, decode and composite, DDIM and
    2M (12 steps: lower_order_final; 16: second order up to the last step), init only at strength 0.5, init + mask at strength 0.5 and
    1, init at strength 1.  Two native runs from the same inputs are bit-identical."""
    import gpu_util as G
    from eegldm.sampling import ddim_sample_hostloop, make_sampling_scheduler, sample
    _cfg, _sd, net = _tiny(501, dtype, case)
    ae = _ae(502, dtype)
    L = UNET_CASES[case][2]
    noise = torch.from_numpy(normal((B, 1, L), seed=503))
    init = torch.from_numpy(normal((B, 1, 4 * L), seed=504)) * 0.5
    sched = make_sampling_scheduler(steps, sampler=sampler)
    for name, kw in _edit_variants(B, 4 * L, 4):
        info = {}
        win, z = sample(net, ae, sched, noise, scale_factor=0.7, crop=8, use_graph=graph, info=info, init=init, **kw)
        assert info["graph"] == graph
        assert win.shape == (B, 1, 4 * L - 16) and torch.isfinite(win).all()
        win2, z2 = sample(net, ae, sched, noise, scale_factor=0.7, crop=8, use_graph=graph, init=init, **kw)
        assert torch.equal(z2, z) and torch.equal(win2, win)
        winh, zh = ddim_sample_hostloop(net, ae, sched, noise, scale_factor=0.7, crop=8, init=init, **kw)
        print(f"{dtype} {case} B={B} graph={graph} {sampler}-{steps} {name}: latents rel-L2 {G.rel_l2(z, zh):.3e}, windows {G.rel_l2(win, winh):.3e}")
        assert G.rel_l2(z, zh) < 5e-5 and G.rel_l2(win, winh) < 5e-5
        if "mask" in kw:
            keep = kw["mask"][:, :, 8:-8].to(win.device) == 1.0
            assert torch.equal(win[keep], init[:, :, 8:-8].to(win.device)[keep])


@pytest.mark.parametrize("sampler,steps", [("ddim", 10), ("dpmpp_2m", 12)])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [1, 5])
def test_native_loop_matches_hostloop_conditional_and_guided(B, graph, sampler, steps):
    """Class-conditional fp32 UNet, pixel-space call (autoencoder=None): plain conditional and guided with w = 3 against the host loop, each
    edit variant, 5e-5 as above; the guided run's null-class half has to receive the blended latents for this to hold over several steps.
    Repeats are bit-identical."""
    import gpu_util as G
    from eegldm.sampling import ddim_sample_hostloop, make_sampling_scheduler, sample
    _cfg, _sd, net = _tiny(511, num_classes=3)
    L = 64
    noise = torch.from_numpy(normal((B, 1, L), seed=512))
    init = torch.from_numpy(normal((B, 1, L), seed=513)) * 0.5
    lab = [2, 0, 1, 2, 0][:B]
    sched = make_sampling_scheduler(steps, sampler=sampler)
    for name, kw in _edit_variants(B, L, 1):
        for g in (dict(labels=lab), dict(labels=lab, guidance_scale=3.0, null_class=1)):
            win, z = sample(net, None, sched, noise, crop=4, use_graph=graph, init=init, **g, **kw)
            _w, zh = ddim_sample_hostloop(net, None, sched, noise, crop=4, init=init, **g, **kw)
            print(f"B={B} graph={graph} {sampler} {name} guided={'null_class' in g}: rel-L2 {G.rel_l2(z, zh):.3e}")
            assert G.rel_l2(z, zh) < 5e-5
            assert torch.equal(sample(net, None, sched, noise, crop=4, use_graph=graph, init=init, **g, **kw)[1], z)
            assert win.shape == (B, 1, L - 8)


# ------------------------------------------------------------------ 4. exact properties of the whole loop
@pytest.mark.parametrize("sampler,steps", [("ddim", 10), ("dpmpp_2m", 12)])
@pytest.mark.parametrize("graph", [False, True])
def test_exact_properties_of_the_loop(graph, sampler, steps):
    import gpu_util as G
    from eegldm.sampling import _multistep_tables, _step_tables, make_sampling_scheduler, sample
    from eegldm.schedulers import PRED
    _cfg, _sd, net = _tiny(531)
    ae = _ae(532)
    B, L = 3, 64
    noise = torch.from_numpy(normal((B, 1, L), seed=533)).to(G.DEV)
    init = (torch.from_numpy(normal((B, 1, 4 * L), seed=534)) * 0.5).to(G.DEV)
    sched = make_sampling_scheduler(steps, sampler=sampler)
    assert sched.final_alpha_cumprod == 1.0
    # init = None, mask = None: today's bytes, against a call made through the old export
    win, z = sample(net, ae, sched, noise, scale_factor=0.7, crop=0, use_graph=graph)
    lat, w_old = torch.empty_like(noise), torch.empty(B, 1, 4 * L, device=G.DEV)
    i64, f32 = (lambda v: (C.c_int64 * len(v))(*v)), (lambda v: (C.c_float * len(v))(*v))
    tail = (G.ptr(lat), G.ptr(w_old), B, L, int(graph), None)
    if sampler == "ddim":
        ts, a_t, a_prev, beta, _anc = _step_tables(sched)
        G.check(G.lib.eegldm_sample(net.h, ae.h, G.ptr(noise), i64(ts), f32(a_t), f32(a_prev), f32(beta), len(ts), 0, PRED["epsilon"], 0, 1.0 / 0.7, 0, *tail))
    else:
        ts, a_t, cx, c0, c1 = _multistep_tables(sched)
        G.check(G.lib.eegldm_sample_multistep(net.h, ae.h, G.ptr(noise), i64(ts), f32(a_t), f32(cx), f32(c0), f32(c1), len(ts), PRED["epsilon"], 0, 1.0 / 0.7,
                                              *tail, None, 1.0, 0))
    assert torch.equal(z, lat) and torch.equal(win, w_old)
    # the new export without the edit block is that loop too
    lat2, w2 = torch.empty_like(lat), torch.empty_like(w_old)
    coef = (NUL, NUL, NUL) if sampler == "ddim" else (f32(cx), f32(c0), f32(c1))
    G.check(G.lib.eegldm_sample_edit(net.h, ae.h, G.ptr(noise), None, None, i64(ts), f32(a_t), f32(a_prev) if sampler == "ddim" else NUL, *coef, NUL,
                                     len(ts), PRED["epsilon"], 0, 1.0 / 0.7, G.ptr(lat2), G.ptr(w2), B, L, int(graph), None, None, 1.0, 0))
    assert torch.equal(lat2, lat) and torch.equal(w2, w_old)
    for s in (0.5, 1.0):
        # an all-zero mask == init only
        w_i, z_i = sample(net, ae, sched, noise, scale_factor=0.7, crop=0, use_graph=graph, init=init, strength=s)
        w_0, z_0 = sample(net, ae, sched, noise, scale_factor=0.7, crop=0, use_graph=graph, init=init, strength=s, mask=torch.zeros(B, 1, 4 * L))
        assert torch.equal(z_0, z_i) and torch.equal(w_0, w_i)
        # an all-one mask: the final latents are z0, the composited windows the input
        mu, _sg = ae.encode(init)
        z0 = torch.empty_like(mu)
        G.check(G.lib.eegldm_edit_start(G.ctx().h, G.ptr(mu), 0.7, None, 1.0, G.ptr(z0), None, z0.numel()))
        w_1, z_1 = sample(net, ae, sched, noise, scale_factor=0.7, crop=0, use_graph=graph, init=init, strength=s, mask=torch.ones(B, 1, 4 * L))
        assert torch.equal(z_1, z0) and torch.equal(w_1, init)
        # a span mask: the kept part of the latents is z0, the rest is not; kept window samples are the input's
        m = _span_mask(B, 4 * L, 4)
        m_lat = (-torch.nn.functional.max_pool1d(-m, 4, 4)).to(G.DEV) == 1.0
        w_s, z_s = sample(net, ae, sched, noise, scale_factor=0.7, crop=0, use_graph=graph, init=init, strength=s, mask=m)
        assert torch.equal(z_s[m_lat], z0[m_lat]) and not (z_s[~m_lat] == z0[~m_lat]).any()
        assert 0 < int(m_lat.sum()) < m_lat.numel()
        keep = m.to(G.DEV) == 1.0
        assert torch.equal(w_s[keep], init[keep]) and not torch.equal(w_s[~keep], init[~keep])
        w_n, z_n = sample(net, ae, sched, noise, scale_factor=0.7, crop=0, use_graph=graph, init=init, strength=s, mask=m, composite=False)
        assert torch.equal(z_n, z_s) and torch.equal(w_n[~keep], w_s[~keep]) and not torch.equal(w_n[keep], init[keep])
        # init_latents = the same z0 is the same run
        w_l, z_l = sample(net, ae, sched, noise, scale_factor=0.7, crop=0, use_graph=graph, init_latents=z0, strength=s, mask=m)
        assert torch.equal(z_l, z_s) and torch.equal(w_l, w_n)
    assert not torch.equal(sample(net, ae, sched, noise, scale_factor=0.7, crop=0, init=init, strength=0.5)[1], z)


# ------------------------------------------------------------------ 5. strength means something
def _gaussian_edit_run(N, order, strength, s=2.0, n=512):
    """The truncated run over the optimal denoiser of N(0, s^2) data, driven through the library: eegldm_edit_start, then one
    eegldm_edit_step per executed step with eps computed in closed form (eps = sigma x / (a s^2 + 1 - a)).  -> (final x, exact
    probability-flow solution from the start onto a = 1, z0), float64 on the host."""
    import gpu_util as G
    from eegldm.schedulers import PRED, _betas, edit_tables, multistep_coefficients, multistep_timesteps
    lib, ctx = G.lib, G.ctx()
    acp = torch.cumprod(1.0 - _betas("scaled_linear_beta", 1000, 0.0015, 0.0205), 0)
    ts = multistep_timesteps(1000, N, "linspace")
    cx, c0, c1 = multistep_coefficients(acp, ts, 1.0, order)
    tab = edit_tables(acp, ts, strength, 1.0, multistep=dict(cx=cx, c0=c0, c1=c1))
    z0 = (torch.from_numpy(normal((n,), seed=71)) * s).to(G.DEV)
    nz = torch.from_numpy(normal((n,), seed=72)).to(G.DEV)
    x, hist = torch.empty_like(z0), torch.zeros_like(z0)
    a0 = tab["a_t"][0]
    G.check(lib.eegldm_edit_start(ctx.h, G.ptr(z0), 1.0, G.ptr(nz), a0, None, G.ptr(x), n))
    x_start = x.double().cpu()
    for i, a in enumerate(tab["a_t"]):
        eps = (math.sqrt(1.0 - a) / (a * s * s + 1.0 - a)) * x
        G.check(lib.eegldm_edit_step(ctx.h, G.ptr(eps), 0.0, 0, G.ptr(x), G.ptr(hist), a, tab["a_next"][i], PRED["epsilon"], 0,
                                     _coef(tab["cx"][i], tab["c0"][i], tab["c1"][i]), None, None, None, G.ptr(x), None, None, n))
    exact = x_start * math.sqrt(s * s / (a0 * s * s + 1.0 - a0))
    return x.double().cpu(), exact, z0.double().cpu()


def test_strength_means_something_on_the_gaussian_denoiser():
    """For N(0, s^2) data the probability-flow ODE from (x_start, t_start) has the closed form x(t') = x(t) sqrt((a' v + 1 - a') /
    (a v + 1 - a)), v = s^2.  Orderings only: the truncated run's error against it falls as N grows; 2M is closer than first order at
    each N; the distance of the result from z0 grows over strengths 0.2, 0.5, 0.8."""
    rms = lambda v: float(v.pow(2).mean().sqrt())
    errs = {}
    for N in (10, 20, 40):
        for order in (1, 2):
            x, exact, _z0 = _gaussian_edit_run(N, order, 0.5)
            errs[N, order] = rms(x - exact) / rms(exact)
        print(f"N={N} strength 0.5: first order {errs[N, 1]:.3e}, 2M {errs[N, 2]:.3e}")
    for N in (10, 20, 40):
        assert errs[N, 2] < errs[N, 1], (N, errs[N, 1], errs[N, 2])
    for order in (1, 2):
        assert errs[10, order] > errs[20, order] > errs[40, order], [errs[N, order] for N in (10, 20, 40)]
    dist = []
    for strength in (0.2, 0.5, 0.8):
        x, _exact, z0 = _gaussian_edit_run(20, 2, strength)
        dist.append(rms(x - z0))
    print(f"distance from z0 at strengths 0.2 / 0.5 / 0.8: {dist[0]:.3e} {dist[1]:.3e} {dist[2]:.3e}")
    assert dist[0] < dist[1] < dist[2], dist


# ------------------------------------------------------------------ 6. entry script
def test_entry_script_writes_edits(tmp_path):
    """edit_trials.py on the tiny checkpoints of the entry-script pin: files and shapes, --mask_span leaves the samples outside the span
    bit-equal to the input, --strength changes the output; the pixel-space twin (--pixel) likewise."""
    import entry_pin_case as E
    from eegldm.entry import edit_trials as ET
    out = str(tmp_path)
    a_yaml, l_yaml, run_a, run_l, run_d = E.write_checkpoints(out)
    N = 3
    x_in = (normal((N, 3072), seed=91) * 0.3).astype(np.float32)
    inp = os.path.join(out, "windows.npy")
    np.save(inp, x_in)
    ldm = ["--output_dir", out, "--best_model_path", run_a, "--diffusion_path", run_l, "--autoencoderkl_config_file_path", a_yaml,
           "--ldm_config_file_path", l_yaml, "--num_inference_steps", "6", "--latent_channels", "1", "--input", inp]
    dm = ["--output_dir", out, "--pixel", "--config_file", l_yaml, "--diffusion_path", run_d, "--num_inference_steps", "6", "--input", inp]

    def run(base, *extra):
        d = ET.main(ET.parse_args(base + list(extra)))
        got = np.stack([np.load(os.path.join(d, f"edit_{i}.npy")) for i in range(N)])
        masks = [os.path.join(d, f"edit_{i}_mask.npy") for i in range(N)]
        return got, masks

    for base in (ldm, dm):
        e5, masks = run(base, "--strength", "0.5")
        assert e5.shape == (N, 1, 1, 3000) and e5.dtype == np.float32 and np.isfinite(e5).all()
        assert not any(os.path.exists(m) for m in masks)
        e8, _ = run(base, "--strength", "0.8")
        assert not np.array_equal(e8, e5)
        again, _ = run(base, "--strength", "0.5")
        assert np.array_equal(again, e5)
        other, _ = run(base, "--strength", "0.5", "--seed", "9")
        assert not np.array_equal(other, e5)
        for sampler in ("ddim", "dpmpp_2m"):
            em, masks = run(base, "--strength", "0.7", "--mask_span", "500:900", "--mask_span", "2000:2003", "--sampler", sampler)
            crop = x_in[:, None, None, 36:-36]
            keep = np.ones(3000, bool); keep[500 - 36:900 - 36] = False; keep[2000 - 36:2003 - 36] = False
            assert em.shape == (N, 1, 1, 3000) and np.isfinite(em).all()
            assert em[..., keep].tobytes() == np.ascontiguousarray(crop[..., keep]).tobytes()
            assert not np.array_equal(em[..., ~keep], crop[..., ~keep])
            for p in masks:
                mk = np.load(p)
                assert mk.shape == (1, 1, 3000) and np.array_equal(mk[0, 0] == 1.0, keep)
        raw, _ = run(base, "--strength", "0.7", "--mask_span", "500:900", "--no_composite")
        assert np.isfinite(raw).all()
        if base is ldm:
            assert not np.array_equal(raw[..., keep], crop[..., keep])          # the decode of kept latents is not the input itself
