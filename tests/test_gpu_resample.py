"""-m gpu: resampled repair (RePaint) -- eegldm_edit_jump against float64 and its exact anchors, the draw in registers against
eegldm_randn bit for bit, eegldm_randn against bytes pinned before its Philox code moved, the native loops (eegldm_sample_edit_resample /
eegldm_sample_long_edit_resample) against the host loops, the exact properties of the loops, what resampling is for on a correlated
Gaussian pair, and the entry scripts."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from make_golden_cases import UNET_CASES  # noqa: E402
from param_gen import normal  # noqa: E402
from test_gpu_dpm_solver import U24, _ae, _carve, _tiny  # noqa: E402
from test_gpu_edit import NUL, _coef, _f32, _span_mask  # noqa: E402
from test_gpu_long import _lay  # noqa: E402
from test_gpu_long_edit import _rec_mask  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i64, f32 = (lambda v: (C.c_int64 * len(v))(*v)), (lambda v: (C.c_float * len(v))(*v))


def formula(n_run, j, r):
    return n_run + (r - 1) * j * len(range(0, n_run - j, j))


def _jump(G, x, jx, jn, fresh, seed, offset, known, noise, mask, a_level, out, out2, n):
    G.check(G.lib.eegldm_edit_jump(G.ctx().h, G.ptr(x), jx, jn, G.ptr(fresh), seed, offset, G.ptr(known), G.ptr(noise), G.ptr(mask), a_level,
                                   G.ptr(out), G.ptr(out2), n))


def _edges_mask(n, seed):
    """binary keep-mask whose value toggles at edges on every residue mod 4 (1, 6, 11, 12, as far as n reaches) and at one more place"""
    m, v = torch.ones(n), 1.0
    at = sorted(set(e for e in (1, 6, 11, 12, 17 + seed % 5) if 0 < e < n))
    for a, b in zip(at, at[1:] + [n]):
        v = 1.0 - v
        m[a:b] = v
    return m


# ------------------------------------------------------------------ 1. + 2. the jump kernel with `fresh` given
@pytest.mark.parametrize("layout", ["aligned", "all+4B", "all+8B", "all+12B", "mixed"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 2052])
def test_edit_jump_vs_float64_and_exact_anchors(n, layout):
    """eegldm_edit_jump with eps = fresh against float64:  p = jx x + jn eps,  k = sqrt(a) z0 + sqrt(1 - a) noise,  out = m k + (1 - m) p.

    Bound, from the operation count (u = 2^-24, one float32 rounding; jx, jn are float32 values the reference takes as they are):
      * p = fma(jx, x, jn * eps): the product and the fma are two roundings of values no larger than P = |jx x| + |jn eps|: |d p| <= 2 u P;
        3 u P is allowed (one u of slack, as test_edit_step_vs_float64_recursion allows 4 for its 3).
      * k = fma(ka, z0, kb * noise): the count of that test -- two roundings and the two rounded sqrtf, 3 u K with K = |ka z0| + |kb noise|,
        4 u K allowed; a_level == 1: k = z0, no rounding.
      * the blend fma(m, k, (1 - m) * p): three roundings of values no larger than |m k| + |(1 - m) p|, 4 u of that allowed, as there; the
        operands' errors enter as m |d k| + (1 - m) |d p|.
    Masks NULL, all 0, all 1, binary with edges on every residue mod 4, fractional; a_level 1 and below 1; every buffer carved at the
    layout's offset from a 16-byte line (mixed: the scalar path).  Exact: mask == 1 returns eegldm_edit_start's x_start at a_level;
    mask == 0 and mask == NULL give the same bytes, a binary mask picks between the two; out2 == out; in place == out of place; a repeat
    gives the same bytes; inputs unwritten."""
    import gpu_util as G
    offs = {"aligned": [0] * 7, "all+4B": [1] * 7, "all+8B": [2] * 7, "all+12B": [3] * 7, "mixed": [0, 1, 2, 3, 0, 2, 1]}[layout]
    worst = 0.0
    for case, (jx, jn, a_level) in enumerate([(0.83, 0.5577, 0.31), (0.999, 0.0447, 1.0), (0.1, 0.995, 0.0123)]):
        jx, jn, a_level = _f32(jx), _f32(jn), _f32(a_level)
        x_h, e_h = torch.from_numpy(normal((n,), seed=100 + case)), torch.from_numpy(normal((n,), seed=200 + case))
        z_h, nz_h = torch.from_numpy(normal((n,), seed=300 + case)) * 0.7, torch.from_numpy(normal((n,), seed=400 + case))
        rnd = torch.from_numpy(np.random.default_rng(500 + case).random(n).astype(np.float32))
        masks = {"null": None, "zeros": torch.zeros(n), "ones": torch.ones(n), "binary": _edges_mask(n, case), "fractional": rnd}
        x, fresh, known, noise = (_carve(h, n, offs[i]) for i, h in enumerate((x_h, e_h, z_h, nz_h)))
        kdev = _carve(None, n, offs[5])
        G.check(G.lib.eegldm_edit_start(G.ctx().h, G.ptr(known), 1.0, G.ptr(noise), a_level, None, G.ptr(kdev), n))
        if a_level == 1.0:
            assert torch.equal(kdev, known)
        rp = jx * x_h.double() + jn * e_h.double()
        tolp = 3.0 * U24 * ((jx * x_h.double()).abs() + (jn * e_h.double()).abs())
        ka, kb = a_level ** 0.5, (1.0 - a_level) ** 0.5
        rk = ka * z_h.double() + kb * nz_h.double()
        tolk = 4.0 * U24 * ((ka * z_h.double()).abs() + (kb * nz_h.double()).abs()) if a_level < 1.0 else torch.zeros(n, dtype=torch.float64)
        plain = None
        for mname, m_h in masks.items():
            mask = None if m_h is None else _carve(m_h, n, offs[4])
            out, out2 = _carve(None, n, offs[5]), _carve(None, n, offs[6])
            _jump(G, x, jx, jn, fresh, 0, 0, known if mask is not None else None, noise if mask is not None else None, mask, a_level, out, out2, n)
            md = torch.zeros(n, dtype=torch.float64) if m_h is None else m_h.double()
            ref = md * rk + (1.0 - md) * rp
            tol = 4.0 * U24 * ((md * rk).abs() + ((1.0 - md) * rp).abs()) * (m_h is not None) + md * tolk + (1.0 - md) * tolp
            err = (out.cpu().double() - ref).abs()
            worst = max(worst, float((err / tol.clamp_min(1e-300)).max()))
            assert (err <= tol).all(), (case, mname, float((err / tol.clamp_min(1e-300)).max()))
            assert torch.equal(out2, out)
            for buf, host in ((x, x_h), (fresh, e_h), (known, z_h), (noise, nz_h)) + (() if m_h is None else ((mask, m_h),)):
                assert torch.equal(buf, host.to(G.DEV)), "an input was written"
            if mname == "null":
                plain = out.clone()
                # known / noise are not read without a mask
                o3 = _carve(None, n, offs[5])
                _jump(G, x, jx, jn, fresh, 0, 0, None, None, None, a_level, o3, None, n)
                assert torch.equal(o3, plain)
            if mname == "zeros":
                assert torch.equal(out, plain)
            if mname == "ones":
                assert torch.equal(out, kdev)
            if mname == "binary":
                assert torch.equal(out, torch.where(mask == 1.0, kdev, plain))
            # in place, out2 left out; a repeat
            x2 = _carve(x_h, n, offs[0])
            _jump(G, x2, jx, jn, fresh, 0, 0, known if mask is not None else None, noise if mask is not None else None, mask, a_level, x2, None, n)
            assert torch.equal(x2, out)
            o4 = _carve(None, n, offs[5])
            _jump(G, x, jx, jn, fresh, 0, 0, known if mask is not None else None, noise if mask is not None else None, mask, a_level, o4, None, n)
            assert o4.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    print(f"n={n} {layout}: worst err / tol {worst:.3f}")


def test_edit_jump_argument_checks():
    import gpu_util as G
    lib, ctx, p = G.lib, G.ctx(), G.ptr
    n = 64
    x, fr, kn, nz, m, out, out2 = (torch.zeros(n, device=G.DEV) for _ in range(7))
    ok = lambda *a: lib.eegldm_edit_jump(ctx.h, *a)
    assert ok(p(x), 0.8, 0.6, p(fr), 0, 0, p(kn), p(nz), p(m), 0.5, p(out), p(out2), n) == 0
    assert ok(p(x), 0.8, 0.6, None, 1, 2, None, None, None, 1.0, p(x), None, n) == 0
    assert ok(p(x), 0.8, 0.6, None, 1, 2, None, None, None, 0.5, p(out), None, 0) == 0
    assert ok(None, 0.8, 0.6, None, 0, 0, None, None, None, 0.5, p(out), None, n) != 0
    assert ok(p(x), 0.8, 0.6, None, 0, 0, None, None, None, 0.5, None, None, n) != 0
    assert ok(p(x), float("nan"), 0.6, None, 0, 0, None, None, None, 0.5, p(out), None, n) != 0
    assert ok(p(x), 0.8, float("nan"), None, 0, 0, None, None, None, 0.5, p(out), None, n) != 0
    assert ok(p(x), 0.8, 0.6, None, 0, 0, None, None, None, 0.0, p(out), None, n) != 0              # a_level outside (0, 1]
    assert ok(p(x), 0.8, 0.6, None, 0, 0, None, None, None, 1.5, p(out), None, n) != 0
    assert ok(p(x), 0.8, 0.6, None, 0, 0, None, p(nz), p(m), 0.5, p(out), None, n) != 0             # a mask without known
    assert ok(p(x), 0.8, 0.6, None, 0, 0, p(kn), None, p(m), 0.5, p(out), None, n) != 0             # ... without noise
    assert ok(p(x), 0.8, 0.6, None, 0, 0, p(kn), p(nz), p(out), 0.5, p(out), None, n) != 0          # mask over out
    assert ok(p(x), 0.8, 0.6, None, 0, 0, p(x), p(nz), p(m), 0.5, p(x), None, n) != 0               # known over an in-place out
    assert ok(p(x), 0.8, 0.6, p(out), 0, 0, None, None, None, 0.5, p(out), None, n) != 0            # fresh over out
    assert ok(p(x), 0.8, 0.6, None, 0, 0, None, None, None, 0.5, p(out), p(out), n) != 0            # out2 over out
    assert ok(p(x), 0.8, 0.6, None, 0, 0, None, None, None, 0.5, p(out), p(x), n) != 0              # out2 over x
    assert ok(p(x), 0.8, 0.6, None, 0, 0, None, None, None, 0.5, p(x[4:]), None, n - 4) != 0        # a shifted view of x
    assert ok(C.c_void_p(x.data_ptr() + 2), 0.8, 0.6, None, 0, 0, None, None, None, 0.5, p(out), None, 8) != 0      # 4-byte alignment


# ------------------------------------------------------------------ 3. the draw in registers
@pytest.mark.parametrize("n", [1, 2, 5, 7, 1023, 1024, 1025, 4099])
def test_draw_in_registers_is_randn_bit_for_bit(n):
    """fresh = NULL against fresh = eegldm_randn(n, seed, offset), bit for bit: every combination of 0..3 floats of misalignment of x, out
    and the three mask-side buffers (equal offsets: the float4 body, starting at element 0, 3, 2 or 1 -- the last three straddle two
    Philox quads per thread; unequal: the scalar path), offsets 0 and 2^33 + 5, two seeds; without a mask, in place and with out2 over the
    offsets of x and out.  Two calls repeat bit for bit."""
    import gpu_util as G
    jx, jn, a_level = _f32(0.83), _f32(0.5577), _f32(0.31)
    hosts = [torch.from_numpy(normal((n,), seed=600 + k)) for k in range(3)] + [_edges_mask(n, 1) if n > 2 else torch.full((n,), 0.5)]
    # one base per buffer and offset: views, made once
    views = [[_carve(h, n, off) for off in range(4)] for h in hosts]              # x, known, noise, mask
    outs = [_carve(None, n, off) for off in range(4)]
    outs2 = [_carve(None, n, off) for off in range(4)]
    heads = set()
    for seed, offset in ((7, 0), (7, 2 ** 33 + 5), (0xC0FFEE0012345678, 0), (0xC0FFEE0012345678, 2 ** 33 + 5)):
        fresh = torch.empty(n, device=G.DEV)
        G.check(G.lib.eegldm_randn(G.ctx().h, G.ptr(fresh), n, seed, offset))
        want = torch.empty(n, device=G.DEV)
        _jump(G, views[0][0], jx, jn, fresh, 0, 0, views[1][0], views[2][0], views[3][0], a_level, want, None, n)
        want_plain = torch.empty(n, device=G.DEV)
        _jump(G, views[0][0], jx, jn, fresh, 0, 0, None, None, None, a_level, want_plain, None, n)
        assert not torch.equal(want_plain, jx * views[0][0])                     # (the noise is in there)
        for ox, oo, ok, on, om in itertools.product(range(4), repeat=5):
            out = outs[oo]
            _jump(G, views[0][ox], jx, jn, None, seed, offset, views[1][ok], views[2][on], views[3][om], a_level, out, None, n)
            assert torch.equal(out, want), (seed, offset, ox, oo, ok, on, om)
            if ox == oo == ok == on == om:
                heads.add((4 - ox) % 4)          # scalar elements ahead of the body = the body's first element index
        for ox, oo in itertools.product(range(4), repeat=2):
            out, out2 = outs[oo], outs2[ox]
            _jump(G, views[0][ox], jx, jn, None, seed, offset, None, None, None, a_level, out, out2, n)
            assert torch.equal(out, want_plain) and torch.equal(out2, want_plain), (seed, offset, ox, oo)
            _jump(G, views[0][ox], jx, jn, None, seed, offset, None, None, None, a_level, out, None, n)
            assert torch.equal(out, want_plain)
        for ox in range(4):
            xi = _carve(hosts[0], n, ox)
            _jump(G, xi, jx, jn, None, seed, offset, views[1][ox], views[2][ox], views[3][ox], a_level, xi, None, n)
            assert torch.equal(xi, want)
    if n >= 8:
        assert heads == {0, 1, 2, 3}, heads          # the body started at element indices 0, 1, 2 and 3 mod 4
    for v, h in zip(views, hosts):
        for off in range(4):
            assert torch.equal(v[off], h.to(G.DEV)), "an input was written"


# ------------------------------------------------------------------ 4. eegldm_randn is unchanged
def test_randn_bytes_are_pinned():
    """tests/golden/randn_pin.npz was written by tests/golden/make_randn_pin.py from a library built before Philox and the Box-Muller quad
    moved into csrc/elementwise.h: the same bytes now."""
    import gpu_util as G
    pin = np.load(os.path.join(ROOT, "tests", "golden", "randn_pin.npz"))
    cases = pin["cases"]
    assert cases.shape == (3, 3)
    for i, (seed, offset, n) in enumerate(cases.tolist()):
        assert n <= 64
        out = torch.empty(n, device=G.DEV)
        G.check(G.lib.eegldm_randn(G.ctx().h, G.ptr(out), n, seed, offset))
        assert out.cpu().numpy().tobytes() == pin[f"out{i}"].tobytes(), (i, seed, offset, n)


# ------------------------------------------------------------------ 5. the native loops against the host loops
SCHEDULES = [("ddim", 10, 2, 3), ("dpmpp_2m", 12, 3, 2), ("dpmpp_2m", 12, 1, 3)]


@pytest.mark.parametrize("sampler,steps,j,r", SCHEDULES)
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("dtype,case,B", [("float32", "tiny_l64", 1), ("float32", "tiny_l64", 5), ("bfloat16", "tiny_l64", 1),
                                          ("bfloat16", "small_l256", 128)])
def test_native_loop_matches_hostloop_ldm(dtype, case, B, graph, sampler, steps, j, r, env_switches):
    """sample(init=, mask=, resamples=, jump_length=) (eegldm_sample_edit_resample) against ddim_sample_hostloop -- scheduler.step per
    forward (first_order=True behind a jump), the jump with eps = training.randn and its blend in torch -- at the 5e-5 relative-L2 bound
    of tests/test_gpu_edit.py, on its cases: LDM with z / scale_factor, decode and composite, strength 0.5 and 1; bfloat16 at B = 128,
    L = 256 on the big-tile GEMM (EEGLDM_GEMM_BIG_MIN_TILES=1).  info["forwards"] is the formula; the composite's kept samples are the
    input's bytes; two native runs are bit-identical."""
    import gpu_util as G
    from eegldm.sampling import ddim_sample_hostloop, make_sampling_scheduler, sample
    if B == 128:
        env_switches(EEGLDM_GEMM_BIG_MIN_TILES="1")
    _cfg, _sd, net = _tiny(801, dtype, case)
    ae = _ae(802, dtype)
    L = UNET_CASES[case][2]
    noise = torch.from_numpy(normal((B, 1, L), seed=803))
    init = torch.from_numpy(normal((B, 1, 4 * L), seed=804)) * 0.5
    mask = _span_mask(B, 4 * L, 4)
    sched = make_sampling_scheduler(steps, sampler=sampler)
    for strength in (0.5, 1.0):
        kw = dict(scale_factor=0.7, crop=8, init=init, mask=mask, strength=strength, resamples=r, jump_length=j, seed=3)
        info = {}
        win, z = sample(net, ae, sched, noise, use_graph=graph, info=info, **kw)
        n_run = steps if strength == 1.0 else steps // 2
        assert info["graph"] == graph and info["forwards"] == formula(n_run, j, r) > n_run
        assert win.shape == (B, 1, 4 * L - 16) and torch.isfinite(win).all()
        win2, z2 = sample(net, ae, sched, noise, use_graph=graph, **kw)
        assert torch.equal(z2, z) and torch.equal(win2, win)
        winh, zh = ddim_sample_hostloop(net, ae, sched, noise, **kw)
        print(f"{dtype} {case} B={B} graph={graph} {sampler}-{steps} j={j} r={r} s={strength}: latents rel-L2 {G.rel_l2(z, zh):.3e}, "
              f"windows {G.rel_l2(win, winh):.3e}")
        assert G.rel_l2(z, zh) < 5e-5 and G.rel_l2(win, winh) < 5e-5
        keep = mask[:, :, 8:-8].to(win.device) == 1.0
        assert torch.equal(win[keep], init[:, :, 8:-8].to(win.device)[keep])


@pytest.mark.parametrize("sampler,steps,j,r", SCHEDULES)
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("B", [1, 5])
def test_native_loop_matches_hostloop_conditional_and_guided_pixel_space(B, graph, sampler, steps, j, r):
    """Class-conditional fp32 UNet, pixel-space call (autoencoder=None): plain conditional and guided (w = 3) against the host loop, 5e-5
    as above, strength 0.5 and 1; the guided run's null-class half has to receive the jumped latents (out2) for this to hold."""
    import gpu_util as G
    from eegldm.sampling import ddim_sample_hostloop, make_sampling_scheduler, sample
    _cfg, _sd, net = _tiny(811, num_classes=3)
    L = 64
    noise = torch.from_numpy(normal((B, 1, L), seed=812))
    init = torch.from_numpy(normal((B, 1, L), seed=813)) * 0.5
    mask = _span_mask(B, L, 1)
    lab = [2, 0, 1, 2, 0][:B]
    sched = make_sampling_scheduler(steps, sampler=sampler)
    for strength in (0.5, 1.0):
        for g in (dict(labels=lab), dict(labels=lab, guidance_scale=3.0, null_class=1)):
            kw = dict(crop=4, init=init, mask=mask, strength=strength, resamples=r, jump_length=j, seed=5, **g)
            win, z = sample(net, None, sched, noise, use_graph=graph, **kw)
            _w, zh = ddim_sample_hostloop(net, None, sched, noise, **kw)
            print(f"B={B} graph={graph} {sampler} j={j} r={r} s={strength} guided={'null_class' in g}: rel-L2 {G.rel_l2(z, zh):.3e}")
            assert G.rel_l2(z, zh) < 5e-5
            assert torch.equal(sample(net, None, sched, noise, use_graph=graph, **kw)[1], z)
            assert win.shape == (B, 1, L - 8)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("m,r_", [(4, 8), (0, 0)])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_canvas_loop_matches_hostloop_ldm(dtype, m, r_, graph, order):
    """sample_long(init=, mask=, resamples=, jump_length=) (eegldm_sample_long_edit_resample: the jump on the canvas, then a gather)
    against sample_long_hostloop, W = 3, R = 2, LDM, 2M-12 with (j, r) = (3, 2) at strength 1 and (1, 3) at strength 0.5, 5e-5 as
    tests/test_gpu_long_edit.py holds its loops to."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample_long, sample_long_hostloop
    _cfg, _sd, net = _tiny(821, dtype)
    ae = _ae(822, dtype)
    R, W, L = 2, 3, 64
    lay = _lay(W, L, m, r_)
    n = 4 * lay.canvas_len
    noise = torch.from_numpy(normal((R, 1, lay.canvas_len), seed=823))
    init = torch.from_numpy(normal((R, 1, n), seed=824)) * 0.5
    mask = _rec_mask(R, n)
    sched = make_sampling_scheduler(12, sampler="dpmpp_2m", solver_order=order)
    for strength, j, r in ((1.0, 3, 2), (0.5, 1, 3)):
        kw = dict(margin=m, ramp=r_, scale_factor=0.7, crop=8, init=init, mask=mask, strength=strength, resamples=r, jump_length=j, seed=11)
        info = {}
        rec, cv = sample_long(net, ae, sched, noise, W, use_graph=graph, info=info, **kw)
        n_run = 12 if strength == 1.0 else 6
        assert info["graph"] == graph and info["forwards"] == formula(n_run, j, r) and info["n_run"] == n_run
        rec2, cv2 = sample_long(net, ae, sched, noise, W, use_graph=graph, **kw)
        assert torch.equal(cv2, cv) and torch.equal(rec2, rec)
        info_h = {}
        rech, cvh = sample_long_hostloop(net, ae, sched, noise, W, info=info_h, **kw)
        print(f"{dtype} (m, r)=({m}, {r_}) graph={graph} order={order} j={j} r={r} s={strength}: canvas rel-L2 {G.rel_l2(cv, cvh):.3e}, "
              f"recording {G.rel_l2(rec, rech):.3e}")
        assert info_h["forwards"] == info["forwards"]
        assert G.rel_l2(cv, cvh) < 5e-5 and G.rel_l2(rec, rech) < 5e-5
        keep = mask[:, :, 8:-8].to(rec.device) == 1.0
        assert torch.equal(rec[keep], init[:, :, 8:-8].to(rec.device)[keep])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("m,r_", [(4, 8), (0, 0)])
def test_canvas_loop_matches_hostloop_guided_pixel_space(m, r_, graph, order):
    """The same on a class-conditional fp32 UNet in pixel space, plain conditional and guided (w = 3): the gather behind the jump has to
    fill the null-class rows too."""
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample_long, sample_long_hostloop
    _cfg, _sd, net = _tiny(831, num_classes=3)
    R, W, L = 2, 3, 64
    lay = _lay(W, L, m, r_)
    Lc = lay.canvas_len
    noise = torch.from_numpy(normal((R, 1, Lc), seed=832))
    init = torch.from_numpy(normal((R, 1, Lc), seed=833)) * 0.6
    mask = _rec_mask(R, Lc)
    lab = [2, 0, 1, 2, 0, 1]
    sched = make_sampling_scheduler(12, sampler="dpmpp_2m", solver_order=order)
    for g in (dict(), dict(guidance_scale=3.0, null_class=1)):
        kw = dict(margin=m, ramp=r_, crop=4, init=init, mask=mask, labels=lab, strength=0.5, resamples=2, jump_length=3, seed=13, **g)
        _r, cv = sample_long(net, None, sched, noise, W, use_graph=graph, **kw)
        _r, cvh = sample_long_hostloop(net, None, sched, noise, W, **kw)
        print(f"(m, r)=({m}, {r_}) graph={graph} order={order} guided={bool(g)}: canvas rel-L2 {G.rel_l2(cv, cvh):.3e}")
        assert G.rel_l2(cv, cvh) < 5e-5
        assert torch.equal(sample_long(net, None, sched, noise, W, use_graph=graph, **kw)[1], cv)


# ------------------------------------------------------------------ 6. exact properties of the loops
@pytest.mark.parametrize("sampler,steps,j,r", SCHEDULES)
@pytest.mark.parametrize("graph", [False, True])
def test_exact_properties_of_the_loop(graph, sampler, steps, j, r):
    import gpu_util as G
    from eegldm.sampling import make_sampling_scheduler, sample
    from eegldm.schedulers import PRED, RESAMPLE_KEY, scheduler_edit_tables, scheduler_resample_tables
    from eegldm.training import randn
    _cfg, _sd, net = _tiny(841)
    ae = _ae(842)
    B, L = 3, 64
    K = 21                                      # the seed of the start noise AND of the call: the key constant has to keep them apart
    noise = randn(net.ctx, (B, 1, L), seed=K)
    init = (torch.from_numpy(normal((B, 1, 4 * L), seed=844)) * 0.5).to(G.DEV)
    sched = make_sampling_scheduler(steps, sampler=sampler)
    ms = sampler != "ddim"
    m = _span_mask(B, 4 * L, 4)
    m_lat_f = (-torch.nn.functional.max_pool1d(-m, 4, 4)).to(G.DEV).contiguous()
    m_lat = m_lat_f == 1.0
    mu, _sg = ae.encode(init)
    z0 = torch.empty_like(mu)
    G.check(G.lib.eegldm_edit_start(G.ctx().h, G.ptr(mu), 0.7, None, 1.0, G.ptr(z0), None, z0.numel()))
    base = dict(scale_factor=0.7, crop=0, use_graph=graph, init=init)

    def raw(tab, jx, jn, seed, fn=None):
        """a call through the export itself, on the latents"""
        lat, win = torch.empty(B, 1, L, device=G.DEV), torch.empty(B, 1, 4 * L, device=G.DEV)
        coef = (f32(tab["cx"]), f32(tab["c0"]), f32(tab["c1"])) if ms else (NUL, NUL, NUL)
        front = (net.h, ae.h, G.ptr(noise), G.ptr(z0), G.ptr(m_lat_f), i64(tab["timesteps"]), f32(tab["a_t"]), NUL if ms else f32(tab["a_prev"]), *coef,
                 f32(tab["a_next"]), len(tab["timesteps"]), PRED["epsilon"], 0, 1.0 / 0.7)
        back = (G.ptr(lat), G.ptr(win), B, L, int(graph), None, None, 1.0, 0)
        if fn is not None:
            G.check(fn(*front, *back))
        else:
            G.check(G.lib.eegldm_sample_edit_resample(*front, jx, jn, seed, *back))
        return win, lat

    for s in (0.5, 1.0):
        tab = scheduler_edit_tables(sched, s)
        n_run = len(tab["timesteps"])
        # resamples = 1 and NULL jump arrays: eegldm_sample_edit's bytes
        info = {}
        w_1, z_1 = sample(net, ae, sched, noise, mask=m, strength=s, composite=False, info=info, **base)
        w_o, z_o = raw(tab, None, None, 0, fn=G.lib.eegldm_sample_edit)
        assert torch.equal(z_1, z_o) and torch.equal(w_1, w_o) and info["forwards"] == n_run
        w_r, z_r = sample(net, ae, sched, noise, mask=m, strength=s, composite=False, resamples=1, jump_length=5, seed=9, **base)
        assert torch.equal(z_r, z_o) and torch.equal(w_r, w_o)
        w_n, z_n = raw(tab, NUL, NUL, 12345)
        assert torch.equal(z_n, z_o) and torch.equal(w_n, w_o)
        # an all-one mask returns z0 and the input's bytes for any (j, r)
        info = {}
        w_a, z_a = sample(net, ae, sched, noise, mask=torch.ones(B, 1, 4 * L), strength=s, resamples=r, jump_length=j, seed=K, info=info, **base)
        assert torch.equal(z_a, z0) and torch.equal(w_a, init) and info["forwards"] == formula(n_run, j, r)
        # a span: kept latents are z0, kept samples the input's; the regenerated part moved, and is not the plain repair's
        w_s, z_s = sample(net, ae, sched, noise, mask=m, strength=s, resamples=r, jump_length=j, seed=K, **base)
        assert torch.equal(z_s[m_lat], z0[m_lat]) and not (z_s[~m_lat] == z0[~m_lat]).any()
        keep = m.to(G.DEV) == 1.0
        assert torch.equal(w_s[keep], init[keep]) and not torch.equal(w_s[~keep], init[~keep])
        assert not (z_s[~m_lat] == z_1[~m_lat]).all()
        # repeats are bit-identical
        w_t, z_t = sample(net, ae, sched, noise, mask=m, strength=s, resamples=r, jump_length=j, seed=K, **base)
        assert torch.equal(z_t, z_s) and torch.equal(w_t, w_s)
        # another seed changes the regenerated part and nothing else
        w_u, z_u = sample(net, ae, sched, noise, mask=m, strength=s, resamples=r, jump_length=j, seed=K + 1, **base)
        assert torch.equal(z_u[m_lat], z_s[m_lat]) and torch.equal(w_u[keep], w_s[keep])
        assert (z_u[~m_lat] != z_s[~m_lat]).float().mean() > 0.9
        # the key: the call made with the export and RESAMPLE_KEY + K is sample(seed=K); with the bare K -- the key the start noise was drawn
        # from, so that the first jump would add the start noise once more -- it is another run
        rt = scheduler_resample_tables(sched, tab, r, j)
        _w, z_k = raw(rt, f32(rt["jump_x"]), f32(rt["jump_n"]), RESAMPLE_KEY + K)
        assert torch.equal(z_k, z_s)
        _w, z_b = raw(rt, f32(rt["jump_x"]), f32(rt["jump_n"]), K)
        assert torch.equal(z_b[m_lat], z_s[m_lat]) and (z_b[~m_lat] != z_s[~m_lat]).float().mean() > 0.9
    first = randn(net.ctx, (B, 1, L), seed=RESAMPLE_KEY + K)
    assert not (first == noise).any()
    # the checks ahead of the loop
    rt = scheduler_resample_tables(sched, scheduler_edit_tables(sched, 1.0), r, j)
    jx, jn = list(rt["jump_x"]), list(rt["jump_n"])
    if ms:          # ONE definition of the first-order coefficients: the arrays step(first_order=True) reads are those of the tables
        from eegldm.schedulers import multistep_coefficients
        fx, f0, _ = multistep_coefficients(sched.alphas_cumprod, sched.timesteps, sched.final_alpha_cumprod, 1, sched.lower_order_final)
        assert (list(sched._cx1), list(sched._c01)) == (list(fx), list(f0))
        assert all((rt["cx"][i], rt["c0"][i]) == (sched._cx1[st], sched._c01[st]) for i, st in enumerate(rt["step"]) if jn[i] != 0.0)
    lat = torch.empty(B, 1, L, device=G.DEV)
    coef = (f32(rt["cx"]), f32(rt["c0"]), f32(rt["c1"])) if ms else (NUL, NUL, NUL)

    def rc(known, mask, jxa, jna, c1=None):
        cf = coef if c1 is None else (coef[0], coef[1], f32(c1))
        return G.lib.eegldm_sample_edit_resample(net.h, ae.h, G.ptr(noise), G.ptr(known), G.ptr(mask), i64(rt["timesteps"]), f32(rt["a_t"]),
                                                 NUL if ms else f32(rt["a_prev"]), *cf, f32(rt["a_next"]), len(jx), PRED["epsilon"], 0, 1.0, jxa, jna, 0,
                                                 G.ptr(lat), None, B, L, 0, None, None, 1.0, 0)
    assert rc(z0, m_lat_f, f32(jx), NUL) != 0 and rc(z0, m_lat_f, NUL, f32(jn)) != 0          # one array without the other
    assert rc(z0, None, f32(jx), f32(jn)) != 0 and rc(None, None, f32(jx), f32(jn)) != 0      # no mask / no known signal
    assert rc(z0, m_lat_f, f32([0.9] + jx[1:]), f32([0.4] + jn[1:])) != 0                    # a jump in front of the first forward
    if ms:
        at = next(i for i, v in enumerate(jn) if v != 0.0)
        c1 = list(rt["c1"]); c1[at] = 0.25
        assert rc(z0, m_lat_f, f32(jx), f32(jn), c1) != 0                                    # a history read behind a jump
    assert rc(z0, m_lat_f, f32(jx), f32(jn)) == 0


@pytest.mark.parametrize("graph", [False, True])
def test_exact_properties_on_the_canvas(graph):
    """fp32 LDM, 2M-12.  resamples = 1 and NULL jump arrays return eegldm_sample_long_edit's bytes; W = 1 returns the flat export's bytes
    (canvas == latents, recording == windows) for (j, r) = (3, 2) and (1, 3); on (R, W) = (2, 3), (m, r) = (4, 8): an all-one mask returns
    z0 and the input, a span keeps z0 / the input bit for bit, repeats are bit-identical, another seed changes the regenerated canvas
    only, info["forwards"] is the formula."""
    import gpu_util as G
    from eegldm.sampling import encode_long, make_sampling_scheduler, sample, sample_long
    from eegldm.schedulers import scheduler_edit_tables
    _cfg, _sd, net = _tiny(851)
    ae = _ae(852)
    sf, L = 0.7, 64
    sched = make_sampling_scheduler(12, sampler="dpmpp_2m")
    # W = 1: the flat export
    noise1 = torch.from_numpy(normal((2, 1, L), seed=853)).to(G.DEV)
    init1 = torch.from_numpy(normal((2, 1, 4 * L), seed=854)) * 0.5
    m1 = _rec_mask(2, 4 * L)
    for s, j, r in ((1.0, 3, 2), (0.5, 1, 3)):
        kw = dict(scale_factor=sf, crop=8, use_graph=graph, init=init1, mask=m1, strength=s, resamples=r, jump_length=j, seed=4)
        win, z = sample(net, ae, sched, noise1, **kw)
        info = {}
        rec1, cv1 = sample_long(net, ae, sched, noise1, 1, margin=4, ramp=8, info=info, **kw)
        assert torch.equal(cv1, z) and torch.equal(rec1, win) and info["forwards"] == formula(12 if s == 1.0 else 6, j, r)
    R, W = 2, 3
    lay = _lay(W, L, 4, 8)
    Lc, n = lay.canvas_len, 4 * lay.canvas_len
    noise = torch.from_numpy(normal((R, 1, Lc), seed=855)).to(G.DEV)
    init = (torch.from_numpy(normal((R, 1, n), seed=856)) * 0.5).to(G.DEV)
    mask = _rec_mask(R, n).to(G.DEV)
    run = lambda **kw: sample_long(net, ae, sched, noise, W, margin=4, ramp=8, scale_factor=sf, crop=0, use_graph=graph, init=init, **kw)
    z0 = encode_long(ae, init, lay, sf)
    keep_lat = (-torch.nn.functional.max_pool1d(-mask, 4, 4)) == 1.0
    for s, j, r in ((1.0, 3, 2), (0.5, 1, 3)):
        rec_p, cv_p = run(mask=mask, strength=s)
        rec_q, cv_q = run(mask=mask, strength=s, resamples=1, jump_length=4, seed=3)
        assert torch.equal(cv_q, cv_p) and torch.equal(rec_q, rec_p)
        # NULL jump arrays through the export
        tab = scheduler_edit_tables(sched, s)
        m_lat = (-torch.nn.functional.max_pool1d(-mask, 4, 4)).contiguous()
        cv_n, rec_n = torch.empty_like(cv_p), torch.empty(R, 1, n, device=G.DEV)
        G.check(G.lib.eegldm_sample_long_edit_resample(net.h, ae.h, G.ptr(noise), G.ptr(z0), G.ptr(m_lat), i64(tab["timesteps"]), f32(tab["a_t"]),
                                                       f32(tab["cx"]), f32(tab["c0"]), f32(tab["c1"]), f32(tab["a_next"]), len(tab["timesteps"]), 0, 0,
                                                       1.0 / sf, NUL, NUL, 77, G.ptr(cv_n), G.ptr(rec_n), R, W, L, 4, 8, int(graph), None, None, 1.0, 0))
        rec_raw, _cv = run(mask=mask, strength=s, composite=False)
        assert torch.equal(cv_n, cv_p) and torch.equal(rec_n, rec_raw)
        info = {}
        rec_a, cv_a = run(mask=torch.ones(R, 1, n), strength=s, resamples=r, jump_length=j, info=info)
        assert torch.equal(cv_a, z0) and torch.equal(rec_a, init) and info["forwards"] == formula(len(tab["timesteps"]), j, r)
        rec_s, cv_s = run(mask=mask, strength=s, resamples=r, jump_length=j, seed=1)
        assert torch.equal(cv_s[keep_lat], z0[keep_lat]) and (cv_s[~keep_lat] != z0[~keep_lat]).float().mean() > 0.9
        assert torch.equal(rec_s[mask == 1.0], init[mask == 1.0]) and not torch.equal(rec_s[mask == 0.0], init[mask == 0.0])
        assert not torch.equal(cv_s, cv_p)
        rec_t, cv_t = run(mask=mask, strength=s, resamples=r, jump_length=j, seed=1)
        assert torch.equal(cv_t, cv_s) and torch.equal(rec_t, rec_s)
        rec_u, cv_u = run(mask=mask, strength=s, resamples=r, jump_length=j, seed=2)
        assert torch.equal(cv_u[keep_lat], cv_s[keep_lat]) and (cv_u[~keep_lat] != cv_s[~keep_lat]).float().mean() > 0.9
        assert torch.equal(rec_u[mask == 1.0], rec_s[mask == 1.0])


# ------------------------------------------------------------------ 7. it does what it is for
def _pair_run(order, r, j=2, N=20, c=0.95, pairs=65536):
    """Pairs (u, v) ~ N(0, [[1, c], [c, 1]]) laid out flat [u0, v0, u1, v1, ...] with the mask [1, 0] repeated: u is kept, v is
    regenerated.  The optimal linear denoiser of that prior (prediction_type "sample"), driven through the library: eegldm_edit_start,
    then per entry of resample_tables eegldm_edit_jump (fresh noise drawn in registers) and eegldm_edit_step.
    -> (slope of the generated v on u, residual variance), float64 on the host."""
    import gpu_util as G
    from eegldm.schedulers import PRED, RESAMPLE_KEY, _betas, edit_tables, multistep_coefficients, multistep_timesteps, resample_tables
    lib, ctx = G.lib, G.ctx()
    acp = torch.cumprod(1.0 - _betas("scaled_linear_beta", 1000, 0.0015, 0.0205), 0)
    ts = multistep_timesteps(1000, N, "linspace")
    cx, c0, c1 = multistep_coefficients(acp, ts, 1.0, order)
    tab = edit_tables(acp, ts, 1.0, 1.0, multistep=dict(cx=cx, c0=c0, c1=c1))
    fx, f0, _ = multistep_coefficients(acp, ts, 1.0, 1)
    rt = resample_tables(tab, (fx, f0), r, j)
    n = 2 * pairs
    g = torch.from_numpy(normal((2, pairs), seed=91)).double()
    u = g[0]
    v = c * g[0] + (1.0 - c * c) ** 0.5 * g[1]
    z0 = torch.stack([u, v], 1).reshape(-1).float().to(G.DEV)
    nz = torch.from_numpy(normal((n,), seed=92)).to(G.DEV)
    mask = torch.tensor([1.0, 0.0]).repeat(pairs).to(G.DEV)
    x, hist = torch.empty_like(z0), torch.zeros_like(z0)
    G.check(lib.eegldm_edit_start(ctx.h, G.ptr(z0), 1.0, G.ptr(nz), rt["a_t"][0], None, G.ptr(x), n))
    Sig = torch.tensor([[1.0, c], [c, 1.0]], dtype=torch.float64)
    jumps = 0
    for i, a in enumerate(rt["a_t"]):
        if rt["jump_n"][i] != 0.0:
            G.check(lib.eegldm_edit_jump(ctx.h, G.ptr(x), rt["jump_x"][i], rt["jump_n"][i], None, RESAMPLE_KEY + 1, jumps * ((n + 3) // 4), G.ptr(z0),
                                         G.ptr(nz), G.ptr(mask), a, G.ptr(x), None, n))
            jumps += 1
        # E[x0 | x_t] = sqrt(a) Sigma (a Sigma + (1 - a) I)^-1 x_t for the pair
        M = (a ** 0.5) * Sig @ torch.linalg.inv(a * Sig + (1.0 - a) * torch.eye(2, dtype=torch.float64))
        x0 = (x.reshape(pairs, 2).double() @ M.T.to(G.DEV)).float().reshape(-1).contiguous()
        G.check(lib.eegldm_edit_step(ctx.h, G.ptr(x0), 0.0, 0, G.ptr(x), G.ptr(hist), a, rt["a_next"][i], PRED["sample"], 0,
                                     _coef(rt["cx"][i], rt["c0"][i], rt["c1"][i]), G.ptr(z0), G.ptr(nz), G.ptr(mask), G.ptr(x), None, None, n))
    assert jumps == (r - 1) * len(range(0, N - j, j))
    out = x.reshape(pairs, 2).double().cpu()
    assert torch.equal(out[:, 0].float(), u.float())                       # the kept half is the input's bytes
    uu, vv = out[:, 0], out[:, 1]
    slope = float((uu * vv).mean() / (uu * uu).mean())
    return slope, float((vv - slope * uu).var())


@pytest.mark.parametrize("order", [1, 2])
def test_resampling_recovers_the_dependence_on_the_kept_part(order):
    """The simulation of the README section through the library: c = 0.95, 20 steps, jump length 2, r in {1, 3, 10}.  The regression slope
    of the generated v on the kept u should be c and the residual variance 1 - c^2.  Orderings only: |slope - c| falls strictly over
    r = 1, 3, 10, the residual variance likewise, and at r = 10 the slope error is under half of r = 1's (the float64 simulation gives
    0.100 against 0.404, a factor of 4; 2 is asked because this runs in float32 on 65 536 pairs, where the standard error of the slope is
    about 0.002)."""
    c = 0.95
    res = {r: _pair_run(order, r) for r in (1, 3, 10)}
    for r, (slope, var) in res.items():
        print(f"order {order} r={r}: slope {slope:.4f} (error {abs(slope - c):.4f}), residual variance {var:.4f} (ideal {1 - c * c:.4f})")
    e = {r: abs(res[r][0] - c) for r in res}
    assert e[1] > e[3] > e[10], e
    assert res[1][1] > res[3][1] > res[10][1], {r: res[r][1] for r in res}
    assert e[10] < 0.5 * e[1], e


# ------------------------------------------------------------------ 8. entry scripts
def test_entry_scripts_take_the_flags(tmp_path):
    """edit_trials.py / edit_long.py on the tiny checkpoints of the entry-script pin.  --resamples 3 --jump_length 2 writes the files and
    the JSON keys and keeps the samples outside the span bit for bit; without the flags the bytes are those of --resamples 1 (the call made
    before the flags existed), and no JSON key is added."""
    import entry_pin_case as E
    from eegldm.entry import edit_long as EL, edit_trials as ET
    out = str(tmp_path)
    a_yaml, l_yaml, run_a, run_l, run_d = E.write_checkpoints(out)
    N = 2
    x_in = (normal((N, 3072), seed=91) * 0.3).astype(np.float32)
    inp = os.path.join(out, "windows.npy")
    np.save(inp, x_in)
    ldm = ["--output_dir", out, "--best_model_path", run_a, "--diffusion_path", run_l, "--autoencoderkl_config_file_path", a_yaml,
           "--ldm_config_file_path", l_yaml, "--num_inference_steps", "6", "--latent_channels", "1"]

    def trials(*extra):
        d = ET.main(ET.parse_args(ldm + ["--input", inp, "--mask_span", "500:900", "--sampler", "dpmpp_2m"] + list(extra)))
        return np.stack([np.load(os.path.join(d, f"edit_{i}.npy")) for i in range(N)]), [os.path.join(d, f"edit_{i}_resample.json") for i in range(N)]

    plain, js = trials()
    assert not any(os.path.exists(p) for p in js)
    one, js = trials("--resamples", "1", "--jump_length", "2")
    assert one.tobytes() == plain.tobytes() and not any(os.path.exists(p) for p in js)
    res, js = trials("--resamples", "3", "--jump_length", "2")
    keep = np.ones(3000, bool); keep[500 - 36:900 - 36] = False
    assert res.shape == plain.shape == (N, 1, 1, 3000) and np.isfinite(res).all()
    assert res[..., keep].tobytes() == plain[..., keep].tobytes() and not np.array_equal(res[..., ~keep], plain[..., ~keep])
    for p in js:
        assert json.load(open(p)) == dict(resamples=3, jump_length=2, forwards=formula(6, 2, 3))
    with pytest.raises(ValueError):
        ET.main(ET.parse_args(ldm + ["--input", inp, "--resamples", "3"]))                  # no mask
    # every call draws its jump noise from its own key, --seed + the index of its first window: two batches do not share it
    seeds, real = [], ET.sample
    ET.sample = lambda *a, **kw: (seeds.append(kw["seed"]), real(*a, **kw))[1]
    try:
        split, _ = trials("--resamples", "3", "--jump_length", "2", "--batch", "1", "--seed", "4")
        whole, _ = trials("--resamples", "3", "--jump_length", "2", "--seed", "4")
    finally:
        ET.sample = real
    assert seeds == [4, 5, 4]
    # (kept samples are the input's either way; a window's regenerated span depends on the call it is in: the key, and its place in the stream)
    assert split[..., keep].tobytes() == whole[..., keep].tobytes()
    assert np.isfinite(split).all() and not np.array_equal(split[1, ..., ~keep], whole[1, ..., ~keep])

    S = 3072 - 1400
    n = 3000 + S + 50
    rec_in = (normal((n,), seed=95) * 0.3).astype(np.float32)
    rinp = os.path.join(out, "recording.npy")
    np.save(rinp, rec_in)

    def long(*extra):
        d = EL.main(EL.parse_args(ldm[:-4] + ["--num_inference_steps", "4", "--latent_channels", "1", "--margin", "100", "--ramp", "150", "--input", rinp,
                                              "--mask_span", "2900:3300"] + list(extra)))
        return np.load(os.path.join(d, "edit_long_0.npy")), open(os.path.join(d, "edit_long_0_layout.json")).read()

    plain, lj = long()
    one, lj1 = long("--resamples", "1")
    assert one.tobytes() == plain.tobytes() and lj1 == lj and "resamples" not in json.loads(lj)
    res, ljr = long("--resamples", "3", "--jump_length", "2")
    got = json.loads(ljr)
    assert (got["resamples"], got["jump_length"], got["forwards"]) == (3, 2, formula(4, 2, 3))
    assert {k: v for k, v in got.items() if k not in ("resamples", "jump_length", "forwards")} == json.loads(lj)
    used = 3000 + S
    keep = np.ones(used, bool); keep[2900:3300] = False
    assert res.shape == plain.shape == (1, 1, used) and np.isfinite(res).all()
    assert res[0, 0, keep].tobytes() == rec_in[:used][keep].tobytes() and not np.array_equal(res[0, 0, ~keep], plain[0, 0, ~keep])
