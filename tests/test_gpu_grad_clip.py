"""-m gpu: global gradient-norm clipping on the device -- the norm pass against float64, the coefficient and the inf/nan flag bit for bit,
the clipped Adam (+ EMA) update against the existing exports (bit for bit) and against torch's clip_grad_norm_ + Adam in float64,
Adam(max_grad_norm=) and GradScaler on a tiny UNet, gradient accumulation, and the entry scripts' flags."""
import os

import numpy as np
import pytest
import torch

from make_golden_cases import UNET_CASES
from param_gen import gen_param, normal, timesteps

pytestmark = pytest.mark.gpu

C = 16384                  # GN_CHUNK of csrc/elementwise.hip: elements per written partial
ADAM = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8)
ADAM_TOL = dict(rtol=1e-5, atol=1e-6)      # what tests/test_gpu_primitives.py::test_scheduler_mse_adam_rng applies to Adam
# D: the longest chain of fp32 roundings a term's running sum passes through in grad_norm_partial_kernel.  A thread adds at most
# GN_CHUNK / 4 / 256 = 16 float4s = 64 fused multiply-adds (the first of them adds to zero: its rounding is the square's), then at most one
# scalar edge element (a chunk has <= 3 head + 3 tail elements, one per thread) -> 65; the wave butterfly adds 6 levels, the pairwise sum of
# the four waves 2 -> 73.  The fold over chunks runs in double (2^-53 per step: nothing at this scale).  All terms are non-negative, so
# every relative error carries through the sum unamplified, and the root halves it: D u / 2 with u = 2^-24.  Outside the sum, the product
# g * pre_scale rounds once and enters the square twice (2 u there, u after the root), and the cast of the double root to float is a full u
# that the root does not halve: the strict worst case is (D + 4) u / 2.  The bound asserted is the one the issue sets, (D + 3) u / 2, half a
# u tighter; the worst case needs all 70-odd roundings of the longest path to fall the same way at full size.
D = 64 + 1 + 6 + 2
NORM_RTOL = (D + 3) * 2.0 ** -24 / 2


def _state(*vals):
    s = torch.zeros(8, device="cuda")
    for i, v in enumerate(vals):
        s[i] = v
    return s


def _carve(n, off, seed, scale=1.0):
    """n random floats starting `off` floats into a 16-byte aligned allocation; returns (allocation, view)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    buf = torch.randn(n + 16, device="cuda", generator=g) * scale
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:off + n]


def _norm(G, c, g, n, pre_scale, max_norm, state, base=None):
    """base: the allocation g was carved from -- torch reports a NULL data pointer for an empty view, and n = 0 still needs a real one."""
    p = G.ptr(g) if n else G.ptr(base)
    G.check(G.lib.eegldm_grad_norm(c.h, p, n, pre_scale, max_norm, G.ptr(state)))


def _coef32(max_norm, norm32):
    with np.errstate(all="ignore"):
        return np.minimum(np.float32(1.0), np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6)))


def _bits(x):
    return np.float32(x).view(np.int32)


SIZES = [0, 1, 3, 5, 1023, 1024, 1025, C - 1, C, C + 1, 3 * C + 7, 10 ** 6 + 3]


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_norm_against_float64_and_coefficient_bits(n, off):
    import gpu_util as G
    c = G.ctx()
    worst = 0.0
    for k, scale in enumerate((1e-6, 1.0, 1e4)):
        buf, g = _carve(n, off, seed=1000 * k + n % 997 + off, scale=scale)
        guard = buf.clone()
        g64 = g.double().cpu().numpy()
        for pre in (1.0, 2.0 ** -16, 3.0):
            st = _state()
            _norm(G, c, g, n, pre, float("inf"), st, base=buf[off:])
            s = st.cpu().numpy()
            want = float(np.sqrt(np.sum((g64 * pre) ** 2)))
            if n == 0:
                assert s[0] == 0.0 and s[1] == 1.0
            else:
                rel = abs(float(s[0]) - want) / want
                worst = max(worst, rel)
                assert rel <= NORM_RTOL, f"n={n} off={off} scale={scale} pre={pre}: norm {s[0]} vs {want} (rel {rel:.3e}, bound {NORM_RTOL:.3e})"
            assert s[1] == 1.0 and s[2] == 0.0 and s[3] == 0.0 and s[4] == 1.0 and s[5] == s[0] and s[6] == 0.0 and s[7] == 0.0
            norm32 = s[0]
            for mx in (1.0, 0.5 * float(norm32), 2.0 * float(norm32)):
                if not mx > 0.0:
                    continue               # (n = 0: the norm is 0 and max_norm must be positive)
                st2 = _state()
                _norm(G, c, g, n, pre, mx, st2, base=buf[off:])
                s2 = st2.cpu().numpy()
                assert _bits(s2[0]) == _bits(norm32)
                assert _bits(s2[1]) == _bits(_coef32(mx, norm32)), f"n={n} max_norm={mx}: coef {s2[1]!r} vs {_coef32(mx, norm32)!r}"
                assert s2[3] == (1.0 if s2[1] < 1.0 else 0.0)
        assert torch.equal(buf.view(torch.int32), guard.view(torch.int32))          # the gradient is only read
    print(f"n={n} off={off}: worst relative norm error {worst:.3e} (bound {NORM_RTOL:.3e})")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_nonfinite_flag_in_head_body_and_tail(off):
    """n = C + 9: two chunks; with off != 0 each has a scalar head, and the last elements of both are a scalar tail."""
    import gpu_util as G
    c = G.ctx()
    n = C + 9
    flag = torch.zeros(1, device="cuda")
    places = {"head": 0, "body": 100, "chunk0_tail": C - 1, "chunk1_body": C + 4, "tail": n - 1}
    cases = [(None, None)] + [(name, bad) for name in places for bad in (float("nan"), float("inf"), -float("inf"))]
    for name, bad in cases:
        gg = _carve(n, off, seed=5 + off)[1]
        if name is not None:
            gg[places[name]] = bad
        st = _state()
        _norm(G, c, gg, n, 1.0, 1.0, st)
        aligned = gg.clone()                    # eegldm_grad_check_finite asks for a 16-byte aligned buffer
        assert aligned.data_ptr() % 16 == 0
        G.check(G.lib.eegldm_grad_check_finite(c.h, G.ptr(aligned), n, G.ptr(flag)))
        s = st.cpu().numpy()
        assert s[2] == (0.0 if name is None else 1.0) == float(flag), (name, bad, s)
        if name is not None:                    # the norm propagates as torch's does: inf (coef 0) or NaN (coef NaN)
            t_norm = torch.linalg.vector_norm(gg.cpu())
            t_coef = torch.clamp(1.0 / (t_norm + 1e-6), max=1.0)
            assert (np.isnan(s[0]) and bool(torch.isnan(t_norm))) or s[0] == float(t_norm)
            assert (np.isnan(s[1]) and bool(torch.isnan(t_coef))) or s[1] == float(t_coef)


def test_counters_accumulate_and_refusals_leave_state_alone():
    import ctypes
    import gpu_util as G
    from eegldm._lib import lib
    c = G.ctx()
    n = 3 * C + 7
    _b, g = _carve(n, 1, seed=9)
    st = _state()
    norms = []
    for pre, mx in ((1.0, 1e9), (3.0, 1.0), (0.5, float("inf"))):      # only the second call clips
        _norm(G, c, g, n, pre, mx, st)
        norms.append(float(st[0]))
    s = st.cpu().numpy()
    assert (s[3], s[4]) == (1.0, 3.0) and s[5] == np.float32(max(norms)) and s[0] == np.float32(norms[-1]) and s[1] == 1.0
    before = st.clone()
    null = ctypes.c_void_p(None)
    bad_calls = [(c.h, null, n, 1.0, 1.0, G.ptr(st)), (c.h, G.ptr(g), n, 1.0, 1.0, null), (null, G.ptr(g), n, 1.0, 1.0, G.ptr(st)),
                 (c.h, G.ptr(g), -1, 1.0, 1.0, G.ptr(st)), (c.h, G.ptr(g), n, 1.0, 0.0, G.ptr(st)), (c.h, G.ptr(g), n, 1.0, -2.0, G.ptr(st)),
                 (c.h, G.ptr(g), n, 1.0, float("nan"), G.ptr(st))]
    for args in bad_calls:
        assert lib.eegldm_grad_norm(*args) != 0
    assert lib.eegldm_grad_scale_by(c.h, null, n, G.ptr(st)) != 0 and lib.eegldm_grad_scale_by(c.h, G.ptr(g), -1, G.ptr(st)) != 0
    torch.cuda.synchronize()
    assert torch.equal(st.view(torch.int32), before.view(torch.int32))


@pytest.mark.parametrize("n,off", [(1025, 1), (3 * C + 7, 3), (10 ** 6 + 3, 0)])
def test_norm_bits_repeat_and_ignore_deterministic_mode(n, off, env_switches):
    import gpu_util as G
    c = G.ctx()
    _b, g = _carve(n, off, seed=77)
    seen = set()
    for det in (None, "1", None):
        env_switches(EEGLDM_DETERMINISTIC=det)
        for _ in range(3):
            st = _state()
            _norm(G, c, g, n, 2.0 ** -16, 0.001, st)
            seen.add(tuple(st.view(torch.int32).tolist()))
    assert len(seen) == 1, seen


# ------------------------------------------------------------------------------------------------------------------ the update
def _views(n, offsets, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    bufs = []
    for k in range(5):
        b = torch.randn(n + 16, device="cuda", generator=g)
        bufs.append(b.abs() if k == 3 else b)
    return bufs, [b[o:o + n] for b, o in zip(bufs, offsets)]


OFFSETS = [(0,) * 5, (1,) * 5, (2,) * 5, (3,) * 5, (1, 2, 0, 3, 2)]


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("offsets", OFFSETS, ids=["aligned", "off4B", "off8B", "off12B", "mixed"])
@pytest.mark.parametrize("n", [1, 5, 1027, C + 9])
def test_clipped_update_is_the_old_export_with_the_product(n, offsets, with_ema):
    """state[1] = 1: the bytes of eegldm_adam_step / eegldm_adam_step_ema; state[1] = c: their bytes for the host float ginv * c."""
    import gpu_util as G
    c = G.ctx()
    step, ginv, omd = 7, 1.0 / 1024.0, float(np.float32(1.0 - 0.9993))
    for coef in (1.0, float(np.float32(0.37))):
        st = _state(123.0, coef)
        bufs_a, (p, g, m, v, e) = _views(n, offsets, seed=n + 3)
        bufs_b, (p2, g2, m2, v2, e2) = _views(n, offsets, seed=n + 3)
        before = [b.clone() for b in bufs_a]
        G.check(G.lib.eegldm_adam_step_clip(c.h, G.ptr(p), G.ptr(g), G.ptr(m), G.ptr(v), G.ptr(e) if with_ema else None, n, ADAM["lr"], ADAM["b1"],
                                            ADAM["b2"], ADAM["eps"], step, ginv, omd, G.ptr(st)))
        host = float(np.float32(ginv) * np.float32(coef))
        if with_ema:
            G.check(G.lib.eegldm_adam_step_ema(c.h, G.ptr(p2), G.ptr(g2), G.ptr(m2), G.ptr(v2), G.ptr(e2), n, ADAM["lr"], ADAM["b1"], ADAM["b2"],
                                               ADAM["eps"], step, host, omd))
        else:
            G.check(G.lib.eegldm_adam_step(c.h, G.ptr(p2), G.ptr(g2), G.ptr(m2), G.ptr(v2), n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], step, host))
        torch.cuda.synchronize()
        for name, a, b in zip("pgmve", bufs_a, bufs_b):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: clip != old export (n={n}, offsets={offsets}, coef={coef})"
        for name, a, b0, off in zip("pgmve", bufs_a, before, offsets):
            assert torch.equal(a[:off], b0[:off]) and torch.equal(a[off + n:], b0[off + n:]), f"{name}: written outside the range"
            changed = not torch.equal(a[off:off + n], b0[off:off + n])
            assert changed == (name in "pmv" or (name == "e" and with_ema)), f"{name}: changed={changed}"
        assert st.tolist() == [123.0, coef, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 5, 1027, C + 9])
def test_scale_by_and_composed_form(n, off):
    import gpu_util as G
    c = G.ctx()
    step, ginv = 3, 1.0 / 256.0
    bufs, (p, g, m, v, _e) = _views(n, (off,) * 5, seed=n + 11)
    p2, m2, v2, g0 = p.clone(), m.clone(), v.clone(), g.clone()
    st = _state()
    _norm(G, c, g, n, ginv, 0.01, st)                                   # clips: the norm of n unit normals / 256 is above 0.01 from n = 5 on
    coef = st[1].clone()
    G.check(G.lib.eegldm_adam_step_clip(c.h, G.ptr(p), G.ptr(g), G.ptr(m), G.ptr(v), None, n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], step,
                                        ginv, 0.0, G.ptr(st)))
    assert torch.equal(g.view(torch.int32), g0.view(torch.int32))       # the fused form leaves the gradient alone
    gbuf = bufs[1].clone(); gs = gbuf[off:off + n]
    G.check(G.lib.eegldm_grad_scale_by(c.h, G.ptr(gs), n, G.ptr(st)))
    assert torch.equal(gs.view(torch.int32), (g0 * coef).view(torch.int32))         # one fp32 product per element
    assert torch.equal(gbuf[:off], bufs[1][:off]) and torch.equal(gbuf[off + n:], bufs[1][off + n:])
    G.check(G.lib.eegldm_adam_step(c.h, G.ptr(p2), G.ptr(gs), G.ptr(m2), G.ptr(v2), n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], step, ginv))
    # composed and fused differ by one rounding of g * c * ginv: close, not bit-equal
    G.assert_close(p, p2, **ADAM_TOL, name="composed vs fused p")


def test_five_steps_against_torch_clip_and_adam_in_float64():
    import gpu_util as G
    c = G.ctx()
    n, max_norm = 4099, 1.0
    p0 = torch.from_numpy(normal((n,), seed=5))
    ref = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([ref], lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"])
    p = p0.clone().cuda(); m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    st = _state()
    clipped = []
    for step, scale in enumerate((0.001, 0.05, 0.002, 0.5, 0.01), start=1):       # norms 0.064, 3.2, 0.128, 32, 0.64 against max_norm 1
        g = torch.from_numpy(normal((n,), seed=20 + step)) * scale
        ref.grad = g.double().clone()
        want_norm = float(torch.nn.utils.clip_grad_norm_([ref], max_norm))
        opt.step()
        gd = g.cuda()
        _norm(G, c, gd, n, 1.0, max_norm, st)
        G.check(G.lib.eegldm_adam_step_clip(c.h, G.ptr(p), G.ptr(gd), G.ptr(m), G.ptr(v), None, n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"],
                                            step, 1.0, 0.0, G.ptr(st)))
        got = float(st[0])
        assert abs(got - want_norm) <= NORM_RTOL * want_norm, (step, got, want_norm)
        clipped.append(want_norm > max_norm)
    assert clipped == [False, True, False, True, False] and st.tolist()[3:5] == [2.0, 5.0]
    G.assert_close(p, ref.detach().float(), **ADAM_TOL, name="clipped adam vs torch float64")


# ------------------------------------------------------------------------------------------------------------------ Adam(max_grad_norm=) on a tiny UNet
def _tiny_unet(dtype="float32", seed=7):
    from eegldm.models import UNetModel
    cfg = dict(UNET_CASES["tiny_l64"][0])
    net = UNetModel(**cfg, dtype=dtype)
    net.load_state_dict({k: torch.from_numpy(gen_param(seed, k, tuple(v.shape))) for k, v in net.state_dict().items()})
    return net, cfg


def _sched(pred="epsilon"):
    from eegldm.schedulers import DDPMScheduler
    return DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195, prediction_type=pred)


def _batch(i, dev, B=4, L=64):
    return (torch.from_numpy(normal((B, 1, L), seed=100 + i)).to(dev), torch.from_numpy(normal((B, 1, L), seed=500 + i)).to(dev),
            torch.from_numpy(timesteps(B, seed=900 + i)).to(dev))


def _steps(net, opt, n_steps, first=0, scaler=None):
    from eegldm.training import ldm_train_step
    sched = _sched()
    for i in range(first, first + n_steps):
        lat, nz, t = _batch(i, net.device)
        net.train(); opt.zero_grad()
        ldm_train_step(net, sched, lat, nz, t, grad_scale=scaler.get_scale() if scaler else 1.0)
        if scaler:
            scaler.step(opt); scaler.update()
        else:
            opt.step()


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
def test_max_grad_norm_inf_reproduces_the_unclipped_optimizer(with_ema, env_switches):
    from eegldm.training import Adam, EMA
    env_switches(EEGLDM_DETERMINISTIC="1")          # two separate trainings are compared: the gradient sums must not race
    out = []
    for mg in (None, float("inf")):
        net, _ = _tiny_unet()
        ema = EMA(net, decay=0.9, warmup=False) if with_ema else None
        opt = Adam(net, lr=1e-3, ema=ema, max_grad_norm=mg)
        _steps(net, opt, 3)
        out.append((net.flat.clone(), opt.m.clone(), opt.v.clone(), ema.shadow.clone() if ema else None, opt))
    for a, b in zip(out[0][:4], out[1][:4]):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))
    st = out[1][4].clip_stats()
    assert st["clipped"] == 0 and st["steps"] == 3 and 0.0 < st["last_norm"] <= st["max_norm_seen"] < float("inf")
    assert out[1][4].step_count == 3 and float(out[1][4].grad_norm) == st["last_norm"]


def test_small_max_grad_norm_is_the_unclipped_update_fed_the_coefficient():
    from eegldm.training import Adam, ldm_train_step
    net, _ = _tiny_unet(); twin, _ = _tiny_unet()
    opt, opt_twin = Adam(net, lr=1e-3, max_grad_norm=1e-3), Adam(twin, lr=1e-3)
    lat, nz, t = _batch(0, net.device)
    net.train(); opt.zero_grad()
    ldm_train_step(net, _sched(), lat, nz, t)
    twin.flat_grad.copy_(net.flat_grad)
    g64 = net.flat_grad.double()
    opt.step()
    want = float(g64.norm())
    assert abs(float(opt.grad_norm) - want) <= NORM_RTOL * want
    coef = float(opt._clip[1])
    assert coef == float(_coef32(1e-3, np.float32(float(opt.grad_norm)))) and coef < 1.0
    opt_twin.step(grad_inv_scale=coef)
    for a, b in ((net.flat, twin.flat), (opt.m, opt_twin.m), (opt.v, opt_twin.v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert opt.clip_stats() == {"last_norm": float(opt.grad_norm), "max_norm_seen": float(opt.grad_norm), "clipped": 1, "steps": 1}
    opt.reset_clip_stats()
    st = opt.clip_stats()
    assert (st["clipped"], st["steps"], st["max_norm_seen"]) == (0, 0, 0.0)
    assert "max_grad_norm" not in str(opt.state_dict()["param_groups"]) and opt.state_dict().keys() == opt_twin.state_dict().keys()


def test_grad_scaler_with_a_clipping_optimizer():
    from eegldm.training import Adam, EMA, GradScaler, ldm_train_step
    net, _ = _tiny_unet()
    ema = EMA(net, decay=0.9, warmup=False)
    opt = Adam(net, lr=1e-3, ema=ema, max_grad_norm=1e-3)
    scaler = GradScaler(init_scale=1024.0)
    _steps(net, opt, 2, scaler=scaler)
    assert opt.step_count == 2 and ema.num_updates == 2
    stats = opt.clip_stats()
    assert stats["steps"] == 2 and stats["clipped"] == 2
    snap = [x.clone() for x in (net.flat, opt.m, opt.v, ema.shadow)]
    net.flat_grad[5] = float("inf")                                        # an injected overflow: the step is skipped, the scale halves
    assert scaler.step(opt) is None
    scaler.update()
    assert scaler.get_scale() == 512.0 and opt.step_count == 2 and ema.num_updates == 2
    for a, b in zip((net.flat, opt.m, opt.v, ema.shadow), snap):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    after = opt.clip_stats()
    assert (after["clipped"], after["steps"], after["max_norm_seen"]) == (stats["clipped"], stats["steps"], stats["max_norm_seen"])
    # a finite step un-scales and clips against the UN-scaled norm
    lat, nz, t = _batch(2, net.device)
    net.train(); opt.zero_grad()
    ldm_train_step(net, _sched(), lat, nz, t, grad_scale=scaler.get_scale())
    want = float(net.flat_grad.double().norm()) / 512.0
    twin_p, twin_m, twin_v, g = net.flat.clone(), opt.m.clone(), opt.v.clone(), net.flat_grad.clone()
    scaler.step(opt); scaler.update()
    assert opt.step_count == 3 and abs(float(opt.grad_norm) - want) <= NORM_RTOL * want
    coef = np.float32(float(opt._clip[1]))
    assert coef == _coef32(1e-3, np.float32(float(opt.grad_norm))) and opt.clip_stats()["steps"] == 3
    import gpu_util as G
    G.check(G.lib.eegldm_adam_step(net.ctx.h, G.ptr(twin_p), G.ptr(g), G.ptr(twin_m), G.ptr(twin_v), g.numel(), 1e-3, 0.9, 0.999, 1e-8, 3,
                                   float(np.float32(1.0 / 512.0) * coef)))
    assert torch.equal(twin_p.view(torch.int32), net.flat.view(torch.int32))


def test_clip_grad_norm_function():
    from eegldm.training import clip_grad_norm_, ldm_train_step
    net, _ = _tiny_unet()
    lat, nz, t = _batch(0, net.device)
    for frac in (0.25, 4.0):                       # clips / leaves alone
        net.train(); net.zero_grad()
        ldm_train_step(net, _sched(), lat, nz, t)
        before = float(net.flat_grad.double().norm())
        x = frac * before
        ret = clip_grad_norm_(net, x)
        assert ret.is_cuda and ret.numel() == 1 and abs(float(ret) - before) <= NORM_RTOL * before          # the norm before clipping
        # min(norm, x) with torch's epsilon: norm * min(1, x / (norm + 1e-6)).  The coefficient carries the norm's error plus the roundings
        # of its sum and quotient, the product one more per element
        after, want = float(net.flat_grad.double().norm()), before * min(1.0, x / (before + 1e-6))
        assert abs(after - want) <= (NORM_RTOL + 3 * 2.0 ** -24) * want, (after, want)
        assert (after < 0.3 * before) == (frac < 1.0)


# ------------------------------------------------------------------------------------------------------------------ accumulation
def _accum_case(step, dtype, env_switches):
    """Two calls on the halves of a B = 4 batch, grad_scale 0.5 each, no zero_grad in between, against one call on the whole batch."""
    env_switches(EEGLDM_DETERMINISTIC="1")
    net, cfg = _tiny_unet(dtype)
    sched = _sched()
    lat, nz, t = _batch(3, net.device)
    net.train(); net.zero_grad()
    whole = float(step(net, sched, lat, nz, t))
    g_whole = net.flat_grad.clone()
    net.zero_grad()
    halves = [float(step(net, sched, lat[i:i + 2], nz[i:i + 2], t[i:i + 2], grad_scale=0.5)) for i in (0, 2)]
    return net, cfg, (lat, nz, t), whole, g_whole, halves


@pytest.mark.parametrize("which", ["ldm", "dm"])
def test_two_micro_steps_accumulate_to_the_whole_batch_fp32(which, env_switches):
    import gpu_util as G
    from eegldm.training import dm_train_step, ldm_train_step
    step = ldm_train_step if which == "ldm" else dm_train_step
    net, _cfg, _b, whole, g_whole, halves = _accum_case(step, "float32", env_switches)
    G.assert_close(net.flat_grad, g_whole, **G.GTOL[G.F32], name=f"{which}: accumulated gradient")
    G.assert_close(torch.tensor([sum(halves) / 2]), torch.tensor([whole]), **G.TOL[G.F32], name=f"{which}: mean of the two losses")
    assert float(g_whole.abs().max()) > 0


def test_two_micro_steps_accumulate_bf16_within_the_storage_gap(env_switches):
    import gpu_util as G
    from eegldm.training import ldm_train_step
    from oracle import losses as Ls, unet as U
    from test_gpu_loss_weighting import _oracle_step
    net, cfg, (lat, nz, t), _whole, _g, _halves = _accum_case(ldm_train_step, "bfloat16", env_switches)
    sd = {k: torch.from_numpy(gen_param(7, k, s)) for k, s in U.unet_param_shapes(cfg).items()}
    acp = Ls.alphas_cumprod("scaled_linear_beta", 1000, 0.0015, 0.0195)
    ones = np.ones(1000)
    _l, _p, g32 = _oracle_step(sd, cfg, acp, lat.cpu(), nz.cpu(), t.cpu(), "epsilon", ones)
    _l, _p, gq = _oracle_step(sd, cfg, acp, lat.cpu(), nz.cpu(), t.cpu(), "epsilon", ones, quant=torch.bfloat16)
    print(G.assert_bf16_grads(net.grad_dict(), g32, gq, "accumulated bf16 step"))


def test_short_last_group_equals_a_plain_step(env_switches):
    """k = 1 of K = 2: the micro-batch ran with grad_scale 1 / K, the step multiplies grad_inv_scale by K / k."""
    import gpu_util as G
    from eegldm.entry.common import accum_factor
    from eegldm.training import Adam, GradScaler, ldm_train_step
    env_switches(EEGLDM_DETERMINISTIC="1")
    lat, nz, t = None, None, None
    out = []
    for K in (1, 2):
        net, _ = _tiny_unet()
        opt = Adam(net, lr=1e-3, max_grad_norm=float("inf"))
        scaler = GradScaler(enabled=False)
        lat, nz, t = _batch(4, net.device, B=2)
        net.train(); opt.zero_grad()
        ldm_train_step(net, _sched(), lat, nz, t, grad_scale=scaler.get_scale() / K)
        scaler.step(opt, accum_factor(K, 1)); scaler.update()
        out.append((net.flat.clone(), float(opt.grad_norm)))
    G.assert_close(out[1][0], out[0][0], **G.TOL[G.F32], name="weights after a short group")
    assert abs(out[1][1] - out[0][1]) <= 2 * NORM_RTOL * out[0][1]        # the factor reached the norm's pre_scale too


# ------------------------------------------------------------------------------------------------------------------ entry scripts
def _setup(tmp_path, n_epochs):
    from test_gpu_ema import _ldm_setup
    _out, train, _ = _ldm_setup(tmp_path, 1, 3000, n_epochs=n_epochs)
    return train


def test_entry_without_the_flags_is_pinned(tmp_path):
    """The same command on the same seed twice (deterministic mode): the same checkpoint keys, none of them new, and the same bytes."""
    from eegldm._lib import set_deterministic
    from eegldm.entry import train_ldm as TL
    from test_gpu_ema import CK_KEYS
    runs = []
    try:
        for name in ("a", "b"):
            (tmp_path / name).mkdir()
            train = _setup(tmp_path / name, n_epochs=2)
            runs.append(TL.main(TL.parse_args(train + ["--synthetic_windows", "16", "--max_steps", "3", "--deterministic"])))
            assert TL.LAST_RUN["steps"] == 3 and TL.LAST_RUN["opt_steps"] == 3 and TL.LAST_RUN["grad_norm_bits"] is None
    finally:
        set_deterministic(False)
    cks = [torch.load(os.path.join(r, "checkpoint.pth")) for r in runs]
    assert set(cks[0]) == set(cks[1]) == CK_KEYS
    fa, fb = (torch.load(os.path.join(r, "final_model.pth")) for r in runs)
    assert fa.keys() == fb.keys() and all(torch.equal(fa[k].view(torch.int32), fb[k].view(torch.int32)) for k in fa)


def test_entry_ldm_with_clipping_and_accumulation_and_resume(tmp_path, capsys):
    import yaml
    from eegldm.entry import train_ldm as TL
    train = _setup(tmp_path, n_epochs=2)            # 24 synthetic windows, batch 8: 3 micro-batches per epoch -> groups of 2 + 1
    flags = ["--synthetic_windows", "24", "--max_grad_norm", "0.5", "--grad_accum_steps", "2"]
    run = TL.main(TL.parse_args(train + flags))
    out = capsys.readouterr().out
    assert TL.LAST_RUN["steps"] == 6 and TL.LAST_RUN["opt_steps"] == 4            # per epoch: one full group and one short one
    lines = [ln for ln in out.splitlines() if ln.startswith("epoch ")]
    assert len(lines) == 2 and all("| grad norm " in ln and ", clipped " in ln and ln.rstrip().endswith("/2") for ln in lines), lines
    ck = torch.load(os.path.join(run, "checkpoint.pth"))
    assert ck["grad_clip"] == {"max_grad_norm": 0.5, "grad_accum_steps": 2} and int(ck["steps"]) == 6
    assert int(float(ck["optimizer"]["state"][0]["step"])) == 4
    # resume without the flags: they come back from the checkpoint; 4 more micro-batches = 2 full groups, cut by --max_steps
    l_yaml = train[train.index("--config_file") + 1]
    y = yaml.safe_load(open(l_yaml)); y["train"]["n_epochs"] = 4; yaml.safe_dump(y, open(l_yaml, "w"))
    assert TL.main(TL.parse_args(train + ["--synthetic_windows", "24", "--max_steps", "4"])) == run
    out = capsys.readouterr().out
    assert "| grad norm " in out and "overrides" not in out
    ck2 = torch.load(os.path.join(run, "checkpoint.pth"))
    assert ck2["grad_clip"] == ck["grad_clip"] and int(ck2["steps"]) == 10
    assert TL.LAST_RUN["opt_steps"] == 4 + 3                                       # epoch 3: groups 2 + 1; epoch 4: one micro-batch, cut
    assert int(float(ck2["optimizer"]["state"][0]["step"])) == 7
    # a different value on the command line wins and says so
    y["train"]["n_epochs"] = 5; yaml.safe_dump(y, open(l_yaml, "w"))
    TL.main(TL.parse_args(train + ["--synthetic_windows", "24", "--max_steps", "2", "--max_grad_norm", "2.0"]))
    out = capsys.readouterr().out
    assert out.count("overrides checkpoint.pth") == 1 and "max_grad_norm 0.5 -> 2.0" in out
    assert torch.load(os.path.join(run, "checkpoint.pth"))["grad_clip"] == {"max_grad_norm": 2.0, "grad_accum_steps": 2}


def test_entry_even_groups_step_count_is_half_the_micro_batches(tmp_path):
    from eegldm.entry import train_ldm as TL
    train = _setup(tmp_path, n_epochs=2)            # 16 windows, batch 8: 2 micro-batches per epoch
    TL.main(TL.parse_args(train + ["--synthetic_windows", "16", "--max_grad_norm", "0.5", "--grad_accum_steps", "2"]))
    assert TL.LAST_RUN["steps"] == 4 and TL.LAST_RUN["opt_steps"] == 2 and TL.LAST_RUN["grad_norm_bits"] is not None


def test_entry_dm_and_autoencoder_with_max_grad_norm(tmp_path, capsys):
    import yaml
    from eegldm.entry import train_autoencoderkl as TA, train_dm as TD
    from test_gpu_entry import AEKL_YAML, LDM_YAML
    out = str(tmp_path)
    d_yaml, a_yaml = os.path.join(out, "dm.yaml"), os.path.join(out, "aekl.yaml")
    d = dict(LDM_YAML); d["train"] = dict(d["train"], output_dir=out, run_dir="dm_eeg", batch_size=4, n_epochs=1)
    a = dict(AEKL_YAML); a["train"] = dict(a["train"], output_dir=out, n_epochs=1)
    yaml.safe_dump(d, open(d_yaml, "w")); yaml.safe_dump(a, open(a_yaml, "w"))
    run = TD.main(TD.parse_args(["--config_file", d_yaml, "--synthetic_windows", "12", "--max_grad_norm", "0.5", "--grad_accum_steps", "2"]))
    text = capsys.readouterr().out
    assert "| grad norm " in text and "clipped " in text and text.count("/2") >= 1          # 3 micro-batches: groups of 2 + 1
    ck = torch.load(os.path.join(run, "checkpoint.pth"))
    assert ck["grad_clip"] == {"max_grad_norm": 0.5, "grad_accum_steps": 2} and int(float(ck["optimizer"]["state"][0]["step"])) == 2
    run_a = TA.main(TA.parse_args(["--config_file", a_yaml, "--synthetic_windows", "16", "--latent_channels", "1", "--max_grad_norm", "1.0"]))
    text = capsys.readouterr().out
    assert text.count("| grad norm g ") == 1 and text.count("| grad norm d ") == 1          # each optimizer against its own model's norm
    assert torch.load(os.path.join(run_a, "checkpoint.pth"))["grad_clip"] == {"max_grad_norm": 1.0, "grad_accum_steps": 1}


def _two_rank_worker(rank, world, port, q, out):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      EEGLDM_DIST_BACKEND="gloo", EEGLDM_LOCAL_DEVICE="0")
    import torch.distributed as dist
    from eegldm.entry import train_ldm as TL
    TL.main(TL.parse_args(["--config_file", os.path.join(out, "ldm.yaml"), "--autoencoderkl_config_file_path", os.path.join(out, "aekl.yaml"),
                           "--synthetic_windows", "16", "--latent_channels", "1", "--max_steps", "3", "--max_grad_norm", "0.5",
                           "--grad_accum_steps", "2"]))
    r = dict(TL.LAST_RUN)
    q.put((rank, r["grad_norm_bits"], r["flat_sha1"], r["steps"], r["opt_steps"], r["sync_rounds"]))
    dist.destroy_process_group()


def test_entry_two_ranks_same_norm_bits_and_one_exchange_per_group(tmp_path):
    """Two ranks on one GPU over gloo, 3 micro-batches in groups of 2 (the second group cut short): the norm is taken after the all-reduce,
    so both ranks hold the same norm bits and end with the same weights, and a group starts ONE gradient exchange."""
    import yaml
    from test_gpu_distributed import _spawn2
    from test_gpu_entry import AEKL_YAML, LDM_YAML
    out = str(tmp_path)
    a = dict(AEKL_YAML); a["train"] = dict(a["train"], output_dir=out)
    l = dict(LDM_YAML); l["train"] = dict(l["train"], output_dir=out)
    yaml.safe_dump(a, open(os.path.join(out, "aekl.yaml"), "w")); yaml.safe_dump(l, open(os.path.join(out, "ldm.yaml"), "w"))
    r0, r1 = _spawn2(_two_rank_worker, extra=(out,))
    assert r0[1] == r1[1] and r0[1] is not None            # the same last_norm, bit for bit
    assert r0[2] == r1[2] and len(r0[2]) == 40             # identical replicas: the hash of every byte of the flat weights
    assert r0[3] == r1[3] == 3 and r0[4] == r1[4] == 2     # 3 micro-batches, 2 optimizer steps
    assert r0[5] == r1[5] == 2                             # one exchange per group, not one per micro-batch
