"""Repairing and extending real recordings (init and keep-mask on the canvas), host side, no GPU: the refusals (raised before anything
touches a model or a device), the torch reference composition (sample_long_hostloop with init / mask) against a per-window loop with the
blend written out here, the all-one / all-zero masks, the elementwise recursion with a zero network, mask erosion, the entry script's
planning arithmetic and the ctypes table."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from test_edit_cpu import _Boom, _fake_scheduler
from test_long_cpu import _TinyNet, _torch_step_scheduler


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("fn", ["sample_long", "sample_long_hostloop"])
def test_refusals_come_before_any_device_work(fn):
    from eegldm import sampling, schedulers as S
    run = getattr(sampling, fn)
    ae = types.SimpleNamespace(down=4, in_channels=1, out_channels=1)
    ae2 = types.SimpleNamespace(down=4, in_channels=2, out_channels=1)
    dpm = _fake_scheduler(S.DPMSolverMultistepScheduler)
    R, W = 2, 3
    lay = sampling.long_layout(W, 64, 4, 8)
    Lc = lay.canvas_len
    noise, init, cv, mask = torch.zeros(R, 1, Lc), torch.zeros(R, 1, 4 * Lc), torch.zeros(R, 1, Lc), torch.ones(R, 1, 4 * Lc)
    kw0 = dict(margin=4, ramp=8)
    bad = [
        dict(mask=mask),                                                 # mask without init / init_canvas
        dict(init=init, init_canvas=cv),                                 # both
        dict(init=init, strength=0.0), dict(init=init, strength=1.5), dict(init=init, strength=float("nan")), dict(init=init, strength=-0.1),
        dict(strength=0.5),                                              # strength without an input
        dict(init=init[:, :, :-1]), dict(init=init[:1]), dict(init=cv),  # init shapes (an LDM takes the recording at window resolution)
        dict(init_canvas=init), dict(init_canvas=cv[:, :, :-1]),
        dict(init=init, mask=mask[:, :, :-4]), dict(init=init, mask=torch.ones(R, 1, Lc)), dict(init=init, mask=torch.ones(R, 2, 4 * Lc)),
        dict(composite=True), dict(init=init, composite=True), dict(init_canvas=cv, mask=mask, composite=True),      # composite without mask and windows
        dict(init=init, mask=mask, mask_erode=-1), dict(mask_erode=-3),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            run(_Boom(), ae, dpm, noise, W, **kw0, **kw)
    # the expected shape is in the message
    with pytest.raises(ValueError, match=r"\(2, 1, %d\)" % (4 * Lc)):
        run(_Boom(), ae, dpm, noise, W, init=init[:, :, :-1], **kw0)
    with pytest.raises(ValueError, match=r"\(2, 1, %d\)" % Lc):
        run(_Boom(), ae, dpm, noise, W, init_canvas=init, **kw0)
    with pytest.raises(ValueError, match=r"\(2, 1, %d\)" % (4 * Lc)):
        run(_Boom(), ae, dpm, noise, W, init=init, mask=mask[:, :, 1:], **kw0)
    # in_channels != out_channels: no composite (explicit or by default); fine when it is switched off
    init2 = torch.zeros(R, 2, 4 * Lc)
    for kw in (dict(init=init2, mask=mask), dict(init=init2, mask=mask, composite=True)):
        with pytest.raises(ValueError, match="in_channels"):
            run(_Boom(), ae2, dpm, noise, W, **kw0, **kw)
    # pixel-space model: init and mask at the sampler's own resolution
    for kw in (dict(init=init), dict(init=cv, mask=mask), dict(mask=torch.ones(R, 1, Lc))):
        with pytest.raises(ValueError):
            run(_Boom(), None, dpm, noise, W, **kw0, **kw)
    # the arguments that are fine get as far as the UNet
    good = [(ae, dict(init=init, strength=0.5, mask=mask)), (ae, dict(init_canvas=cv, mask=mask, mask_erode=3)), (ae, dict(init=init)),
            (ae2, dict(init=init2, mask=mask, composite=False)), (None, dict(init=cv, mask=torch.ones(R, 1, Lc), composite=True))]
    for a, kw in good:
        with pytest.raises((AssertionError, TypeError), match="UNet"):
            run(_Boom(), a, dpm, noise, W, **kw0, **kw)


# ------------------------------------------------------------------ the torch reference composition, pixel space
def _f32(v):
    return v.to(torch.float32)


def _renoise(z0, nz, a):
    """k(a) with the library's roundings, written out: the product kb * nz in float32, then a fused multiply-add; a == 1 is z0"""
    a32 = np.float32(a)
    ka, kb = float(np.sqrt(a32)), float(np.sqrt(np.float32(1.0) - a32))
    if kb == 0.0:
        return _f32(z0.double() * ka)
    return _f32(ka * z0.double() + _f32(nz.double() * kb).double())


def _blend(m, k, p):
    """m == 0: p; m == 1: k; else fma(m, k, (1 - m) * p), 1 - m and the product rounded to float32"""
    mixed = _f32(m.double() * k.double() + _f32(_f32(1.0 - m.double()).double() * p.double()).double())
    return torch.where(m == 0, p, torch.where(m == 1, k, mixed))


def _x0(out, x, a_t, pred):
    a = np.float32(a_t)
    sa, sb = float(np.sqrt(a)), float(np.sqrt(np.float32(1.0) - a))
    if pred == "epsilon":
        return _f32(_f32(x.double() - sb * out.double()).double() / sa)
    if pred == "v_prediction":
        return _f32(sa * x.double() - _f32(sb * out.double()).double())
    return out


def _update(tab, i, x, x0, hist):
    inner = _f32(tab["c0"][i] * x0.double() + _f32(tab["c1"][i] * hist.double()).double()) if tab["c1"][i] != 0.0 else _f32(tab["c0"][i] * x0.double())
    return _f32(tab["cx"][i] * x.double() + inner.double())


def _per_window_loop(net, tab, rows_noise, rows_z0, rows_mask, pred):
    """The R * W windows as independent rows: the noised start, per step the model, x0, the update from the truncated tables, the blend"""
    x = _renoise(rows_z0, rows_noise, tab["a_t"][0])
    hist = torch.zeros_like(x)
    tt = torch.empty(x.shape[0], dtype=torch.int64)
    for i, t in enumerate(tab["timesteps"]):
        tt.fill_(t)
        x0 = _x0(net(x, timesteps=tt).float(), x, tab["a_t"][i], pred)
        x = _update(tab, i, x, x0, hist)
        hist = x0
        if rows_mask is not None:
            x = _blend(rows_mask, _renoise(rows_z0, rows_noise, tab["a_next"][i]), x)
    return x


def _mask(kind, R, n, seed=5):
    g = torch.Generator().manual_seed(seed)
    if kind == "zeros":
        return torch.zeros(R, 1, n)
    if kind == "ones":
        return torch.ones(R, 1, n)
    if kind == "binary":
        m = torch.ones(R, 1, n)
        m[:, :, n // 5:n // 2 + 3] = 0.0
        m[-1, :, -7:] = 0.0
        return m
    return torch.rand(R, 1, n, generator=g)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("order,N,strength", [(1, 4, 1.0), (2, 6, 1.0), (2, 6, 0.5)])
@pytest.mark.parametrize("R,W,Cc,kind", [(1, 1, 1, "binary"), (2, 3, 2, "binary"), (1, 5, 1, "fractional"), (2, 3, 1, None)])
def test_hostloop_without_overlap_is_the_per_window_loop_with_the_blend(R, W, Cc, kind, order, N, strength, pred):
    """m = r = 0, pixel-space call: sample_long_hostloop(init=, mask=) has to return, bit for bit, what the R * W windows give as independent
    rows of a loop written out here -- k(a_t[0]) as the start, the truncated tables of schedulers.edit_tables (first executed step first
    order), x <- blend(mask, k(a_next), x) after every step -- and the composite of the canvas with the input."""
    from eegldm.sampling import sample_long_hostloop
    from eegldm.schedulers import scheduler_edit_tables
    net, L = _TinyNet(Cc), 16
    sched = _torch_step_scheduler(N, order, pred)
    g = torch.Generator().manual_seed(21)
    noise, init = torch.randn(R, Cc, W * L, generator=g), torch.randn(R, Cc, W * L, generator=g) * 0.7
    mask = None if kind is None else _mask(kind, R, W * L)
    rec, canvas = sample_long_hostloop(net, None, sched, noise, W, margin=0, ramp=0, crop=2, init=init, strength=strength, mask=mask)
    tab = scheduler_edit_tables(sched, strength)
    assert tab["c1"][0] == 0.0 and len(tab["timesteps"]) == (N if strength == 1.0 else N // 2)
    rows = lambda v: v.reshape(R, v.shape[1], W, L).permute(0, 2, 1, 3).reshape(R * W, v.shape[1], L)
    m_rows = None if mask is None else rows(mask).expand(R * W, Cc, L)
    lat = _per_window_loop(net, tab, rows(noise), rows(init), m_rows, pred)
    want = lat.reshape(R, W, Cc, L).permute(0, 2, 1, 3).reshape(R, Cc, W * L)
    assert torch.isfinite(canvas).all() and torch.equal(canvas, want)
    full = want if mask is None else _blend(mask.expand(R, Cc, W * L), init, want)
    assert torch.equal(rec, full[:, :, 2:-2])
    if mask is not None:
        keep = (mask == 1).expand(R, Cc, W * L)
        assert torch.equal(canvas[keep], init[keep]), "the last step lands on a = 1: kept positions hold the input"
        _r, plain = sample_long_hostloop(net, None, sched, noise, W, margin=0, ramp=0, crop=2, init=init, strength=strength)
        assert not torch.equal(plain, canvas)


@pytest.mark.parametrize("m,r", [(0, 0), (1, 2), (2, 0)])
def test_all_one_mask_returns_init_and_all_zero_mask_is_init_only(m, r):
    from eegldm.sampling import long_layout, sample_long_hostloop
    R, W, Cc, L = 2, 3, 2, 16
    lay = long_layout(W, L, m, r)
    net, sched = _TinyNet(Cc), _torch_step_scheduler(6, 2, "v_prediction")
    g = torch.Generator().manual_seed(31)
    noise, init = torch.randn(R, Cc, lay.canvas_len, generator=g), torch.randn(R, Cc, lay.canvas_len, generator=g)
    kw = dict(margin=m, ramp=r, crop=0, init=init, strength=0.5)
    rec, cv = sample_long_hostloop(net, None, sched, noise, W, mask=torch.ones(R, 1, lay.canvas_len), **kw)
    assert torch.equal(cv, init) and torch.equal(rec, init)
    _rec0, cv0 = sample_long_hostloop(net, None, sched, noise, W, mask=torch.zeros(R, 1, lay.canvas_len), **kw)
    _reci, cvi = sample_long_hostloop(net, None, sched, noise, W, **kw)
    assert torch.equal(cv0, cvi) and torch.equal(_rec0, _reci) and not torch.equal(cvi, init)
    # init_canvas is the same input for a pixel-space model
    _recc, cvc = sample_long_hostloop(net, None, sched, noise, W, margin=m, ramp=r, crop=0, init_canvas=init, strength=0.5)
    assert torch.equal(cvc, cvi)


class _ZeroNet(_TinyNet):
    def forward(self, x, timesteps):
        return torch.zeros_like(x)


@pytest.mark.parametrize("kind", ["binary", "fractional", None])
def test_zero_network_follows_the_elementwise_recursion(kind):
    """A network that returns 0: x0 depends on the canvas value alone, so the windows of an overlap predict the same value and the canvas
    has to follow the plain recursion of step + blend element by element.  Outside the ramps: the bytes of the same call on ONE window as
    long as the canvas (nothing is fused there).  Everywhere: a float64 recursion written out here; the float32 run makes at most 12
    roundings per step (x0 2, the fuse 2, the update 3, k 2, the blend 3) of values no larger than the step's largest magnitude M, and a
    step passes an earlier error on times at most |cx| + |c0| / sqrt(a_t) + |c1| <= G; the bound is that recursion, E <- G E + 12 u M."""
    from eegldm.sampling import long_layout, sample_long_hostloop
    from eegldm.schedulers import scheduler_edit_tables
    R, W, L, m, r = 2, 3, 28, 4, 8
    lay = long_layout(W, L, m, r)
    Lc = lay.canvas_len
    net, sched = _ZeroNet(1), _torch_step_scheduler(6, 2, "epsilon")
    g = torch.Generator().manual_seed(41)
    noise, init = torch.randn(R, 1, Lc, generator=g), torch.randn(R, 1, Lc, generator=g)
    mask = None if kind is None else _mask(kind, R, Lc)
    kw = dict(crop=0, init=init, mask=mask, strength=0.7)
    _rec, cv = sample_long_hostloop(net, None, sched, noise, W, margin=m, ramp=r, **kw)
    _rec1, cv1 = sample_long_hostloop(net, None, sched, noise, 1, margin=0, ramp=0, **kw)
    ramp = torch.zeros(Lc, dtype=torch.bool)
    for a, b in lay.seams():
        ramp[a:b] = True
    assert torch.equal(cv[:, :, ~ramp], cv1[:, :, ~ramp])
    tab = scheduler_edit_tables(sched, 0.7)
    z0, nz = init.double(), noise.double()
    k64 = lambda a: (a ** 0.5) * z0 + ((1.0 - a) ** 0.5) * nz
    x, hist, E = k64(tab["a_t"][0]), torch.zeros_like(z0), 0.0
    for i in range(len(tab["timesteps"])):
        x0 = x / tab["a_t"][i] ** 0.5
        prev = tab["cx"][i] * x + tab["c0"][i] * x0 + tab["c1"][i] * hist
        M = max(float(v.abs().max()) for v in (x0, tab["cx"][i] * x, tab["c0"][i] * x0, tab["c1"][i] * hist, prev, z0, nz))
        G = abs(tab["cx"][i]) + abs(tab["c0"][i]) / tab["a_t"][i] ** 0.5 + abs(tab["c1"][i])
        E = G * E + 12 * 2.0 ** -24 * M
        hist, x = x0, prev
        if mask is not None:
            x = mask.double() * k64(tab["a_next"][i]) + (1.0 - mask.double()) * x
    err = float((cv.double() - x).abs().max())
    assert err <= E, (err, E)
    assert float(x.abs().max()) > 0.1 and E < 1e-3


# ------------------------------------------------------------------ erosion
def test_mask_erode_on_a_hand_written_mask():
    from eegldm.sampling import erode_mask
    m = torch.tensor([[[1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1.]]])
    assert torch.equal(erode_mask(m, 0), m)
    assert erode_mask(m, 1)[0, 0].tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1]
    assert erode_mask(m, 2)[0, 0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1]
    # the free ends of a recording are no regenerated span: an all-one mask stays; fractional values take the neighbourhood's minimum
    assert torch.equal(erode_mask(torch.ones(2, 1, 9), 3), torch.ones(2, 1, 9))
    f = torch.tensor([[[1, 0.5, 1, 1, 0.25, 1]]])
    assert erode_mask(f, 1)[0, 0].tolist() == [0.5, 0.5, 0.5, 0.25, 0.25, 0.25]
    with pytest.raises(ValueError):
        erode_mask(m, -1)


def test_erosion_reaches_the_latent_mask_and_not_the_composite():
    """pixel-space host loop with a binary mask: mask_erode = 2 regenerates two more positions on each side of the span, yet the composite
    returns the input wherever the mask AS GIVEN keeps it"""
    from eegldm.sampling import sample_long_hostloop
    R, W, L = 1, 2, 16
    net, sched = _TinyNet(1), _torch_step_scheduler(4, 1, "epsilon")
    g = torch.Generator().manual_seed(51)
    noise, init = torch.randn(R, 1, W * L, generator=g), torch.randn(R, 1, W * L, generator=g)
    mask = torch.ones(R, 1, W * L)
    mask[:, :, 10:14] = 0.0
    rec, cv = sample_long_hostloop(net, None, sched, noise, W, margin=0, ramp=0, crop=0, init=init, mask=mask, mask_erode=2)
    kept = torch.ones(W * L, dtype=torch.bool)
    kept[8:16] = False
    assert torch.equal(cv[:, :, kept], init[:, :, kept]) and (cv[:, :, ~kept] != init[:, :, ~kept]).all()
    given = mask[0, 0] == 1
    assert torch.equal(rec[:, :, given], init[:, :, given]) and torch.equal(rec[:, :, ~given], cv[:, :, ~given])


# ------------------------------------------------------------------ the entry script's planning arithmetic
def test_plan_window_count_and_left_out_samples():
    from eegldm.entry import edit_long as E
    # defaults: L = 768 latents, down 4, m 18, r 36: 2784 (W - 1) + 3000 <= n
    for n, W, left in ((3000, 1, 0), (3001, 1, 1), (5783, 1, 2783), (5784, 2, 0), (60000, 21, 1320)):
        p = E.plan_edit(n, 768, 4)
        assert (p["kept_windows"], p["left_out"], p["used"]) == (W, left, n - left), (n, p)
        assert p["layout"].n_windows == W and p["extension"] == 0 and (p["layout"].margin, p["layout"].ramp, p["layout"].stride) == (18, 36, 696)
        assert 4 * p["layout"].canvas_len - 72 == p["used"]
    with pytest.raises(ValueError):
        E.plan_edit(2999, 768, 4)
    # pixel space, no overlap: 3072-sample windows, the first gives 3000 samples
    p = E.plan_edit(7000, 3072, 1, margin=0, ramp=0)
    assert (p["kept_windows"], p["used"], p["left_out"]) == (2, 6072, 928)


def test_plan_extension_window_counts():
    from eegldm.entry import edit_long as E
    # five more minutes = 30000 samples at 2784 per window: 11 windows (30624 samples); one second: 1 window
    for minutes, extra in ((5.0, 11), (1.0 / 60.0, 1), (2784 / 6000.0, 1), (2785 / 6000.0, 2), (0.0, 0)):
        p = E.plan_edit(30000, 768, 4, extend_minutes=minutes)
        assert p["kept_windows"] == 10 and p["layout"].n_windows == 10 + extra and p["extension"] == 2784 * extra, (minutes, p)
        assert p["used"] == 2784 * 9 + 3000 and p["left_out"] == 30000 - p["used"]
    args = E.parse_args(["--output_dir", "o", "--diffusion_path", "d", "--input", "x.npy", "--pixel", "--config_file", "c", "--extend_minutes", "5",
                         "--mask_span", "10:20", "--mask_span", "100:200", "--mask_erode", "8", "--strength", "0.6", "--no_composite"])
    E.check_args(args)
    assert args.mask_span == ["10:20", "100:200"] and args.mask_erode == 8 and args.no_composite and args.seed == 0 and args.solver_order == 2
    base = ["--output_dir", "o", "--diffusion_path", "d", "--input", "x.npy", "--pixel", "--config_file", "c"]
    for bad in (["--strength", "0"], ["--strength", "1.1"], ["--mask_erode", "-1"], ["--extend_minutes", "-1"], ["--mask_span", "20:10"],
                ["--mask_span", "abc"], ["--hypnogram", "h.npy", "--class_label", "1"]):
        with pytest.raises(ValueError):
            E.check_args(E.parse_args(base + bad))
    with pytest.raises(ValueError):
        E.check_args(E.parse_args(base[:-3]))


def test_spans_to_mask_and_the_padded_inputs():
    from eegldm.entry import edit_long as E
    m = E.spans_to_mask(12, [(2, 4), (9, 12)])
    assert m.dtype == np.float32 and m.tolist() == [1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0]
    assert E.spans_to_mask(5, []).tolist() == [1] * 5 and E.parse_span("3:7") == (3, 7)
    with pytest.raises(ValueError):
        E.spans_to_mask(12, [(9, 13)])
    # the padded recording and mask: crop zeros, the used samples, the extension
    n = 3100
    x = np.arange(1, n + 1, dtype=np.float32)[None]
    plan = E.plan_edit(n, 768, 4)
    init, mk = E.build_inputs(x, None, plan, 4)
    assert mk is None and init.shape == (1, 1, 3072) and (init[0, 0, :36] == 0).all() and (init[0, 0, -36:] == 0).all()
    assert np.array_equal(init[0, 0, 36:-36], x[0, :3000])
    span = np.broadcast_to(E.spans_to_mask(n, [(100, 200)]), x.shape)
    init, mk = E.build_inputs(x, span, plan, 4)
    assert mk.shape == init.shape and (mk[0, 0, :36] == 1).all() and (mk[0, 0, -36:] == 1).all() and np.array_equal(mk[0, 0, 36:-36], span[0, :3000])
    plan = E.plan_edit(n, 768, 4, extend_minutes=0.2)
    init, mk = E.build_inputs(x, None, plan, 4)
    assert plan["layout"].n_windows == 2 and init.shape == (1, 1, 3072 + 2784)
    assert (mk[0, 0, :3036] == 1).all() and (mk[0, 0, 3036:] == 0).all() and (init[0, 0, 3036:] == 0).all() and np.array_equal(init[0, 0, 36:3036], x[0, :3000])


# ------------------------------------------------------------------ the ctypes table
def test_abi_table_and_argument_checks_without_a_device():
    from eegldm._lib import lib, SIGNATURES
    assert lib.eegldm_abi_version() == 8
    for name in ("eegldm_canvas_edit_step", "eegldm_sample_long_edit"):
        assert name in SIGNATURES and hasattr(lib, name)
    z = C.c_void_p(0)
    assert lib.eegldm_canvas_edit_step(z, z, 0.0, 0, z, z, 0.5, 0.6, 0, 0, 1.0, 1.0, 0.0, 1, 1, 2, 16, 4, 0, z, z, z, z, z, z, z) != 0
    assert b"null" in lib.eegldm_last_error()
    one, ts = (C.c_float * 1)(0.5), (C.c_int64 * 1)(999)
    assert lib.eegldm_sample_long_edit(z, z, z, z, z, ts, one, one, one, one, one, 1, 0, 0, 1.0, z, z, 1, 2, 16, 4, 0, 0, None, None, 1.0, 0) != 0
