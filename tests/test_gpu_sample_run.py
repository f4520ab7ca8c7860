"""GPU: eegldm_sample_run against the ten positional sampling exports, and the descriptor's own refusals.

Every positional export fills an eegldm_sample_desc from its argument list and runs it.  Case 1 pins that mapping: each export is called
with its argument list (ORDER: the header's order, by the descriptor's member names) and eegldm_sample_run with the same members written
into a descriptor, and the outputs must be the same bytes, eager and replayed.  Case 2 sends descriptors that break one rule each: every
one is refused, and the valid call on the same handles afterwards returns what it returned before.

Tiny fp32 UNet at L = 64, 4 executed steps (7 forwards in the two resampled forms: resamples 2, jump_length 1), B = 2 windows or one
canvas of W = 2 windows (m = 4, r = 8: Lc = 112), 3 classes with guidance 3 and null class 1, a context UNet with 2 context channels."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from param_gen import normal  # noqa: E402
from test_gpu_dpm_solver import _ae, _tiny  # noqa: E402

B, L, R, W, M, RAMP = 2, 64, 1, 2, 4, 8
LC = (W - 1) * (L - (2 * M + RAMP)) + L

_WINDOW = "latents_out windows_out B L use_graph graph_used labels guidance_scale null_class"
_CANVAS = "canvas_out recording_out R W L m r use_graph graph_used labels guidance_scale null_class"
_DDIM = "unet ae noise timesteps a_t a_prev beta_t n_steps ancestral pred_type clip_sample inv_scale_factor noise_seed latents_out windows_out B L use_graph graph_used"
_HEAD = "unet ae noise known mask timesteps a_t"
_SCALARS = "n_steps pred_type clip_sample inv_scale_factor"
_JUMPS = "jump_x jump_n noise_seed"
# the argument list of each export in the header's order, under the descriptor's member names
ORDER = {
    "eegldm_sample": _DDIM,
    "eegldm_sample_cond": f"{_DDIM} labels guidance_scale null_class",
    "eegldm_sample_multistep": f"unet ae noise timesteps a_t cx c0 c1 {_SCALARS} {_WINDOW}",
    "eegldm_sample_edit": f"{_HEAD} a_prev cx c0 c1 a_next {_SCALARS} {_WINDOW}",
    "eegldm_sample_long": f"unet ae noise timesteps a_t cx c0 c1 {_SCALARS} {_CANVAS}",
    "eegldm_sample_long_edit": f"{_HEAD} cx c0 c1 a_next {_SCALARS} {_CANVAS}",
    "eegldm_sample_edit_resample": f"{_HEAD} a_prev cx c0 c1 a_next {_SCALARS} {_JUMPS} {_WINDOW}",
    "eegldm_sample_long_edit_resample": f"{_HEAD} cx c0 c1 a_next {_SCALARS} {_JUMPS} {_CANVAS}",
    "eegldm_sample_edit_ctx": f"{_HEAD} a_prev cx c0 c1 a_next {_SCALARS} {_JUMPS} {_WINDOW} context context_rows",
    "eegldm_sample_long_edit_ctx": f"{_HEAD} cx c0 c1 a_next {_SCALARS} {_JUMPS} {_CANVAS} context context_rows",
}
_NUMBERS = set("B L R W m r n_steps ancestral pred_type clip_sample inv_scale_factor noise_seed guidance_scale null_class context_rows use_graph".split())


def _f32(v):
    return (C.c_float * len(v))(*v)


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _dev(a):
    return torch.as_tensor(a).to("cuda:0", torch.float32).contiguous()


def _span_mask(shape, first, stop):
    m = torch.ones(shape)
    m[..., first:stop] = 0.0
    return _dev(m)


@functools.lru_cache(maxsize=None)
def _forms():
    """name of the export -> (the descriptor's members without outputs and graph switch, {output member: shape}); the tensors the members
    point to live in the third entry of the returned tuple."""
    from eegldm._lib import PRED
    from eegldm.sampling import _multistep_tables, _step_tables, make_sampling_scheduler
    from eegldm.schedulers import RESAMPLE_KEY, scheduler_edit_tables, scheduler_resample_tables
    plain, cond, ctxn = _tiny(601)[2], _tiny(602, num_classes=3)[2], _tiny(603, in_channels=3, context_channels=2)[2]
    ae = _ae(604)
    down = ae.down
    t = dict(noise=_dev(normal((B, 1, L), seed=611)), known=_dev(normal((B, 1, L), seed=612) * 0.5), mask=_span_mask((B, 1, L), 20, 41),
             context=_dev(normal((B, 2, L), seed=613)),
             cnoise=_dev(normal((R, 1, LC), seed=614)), cknown=_dev(normal((R, 1, LC), seed=615) * 0.5), cmask=_span_mask((R, 1, LC), 50, 70),
             ccontext=_dev(normal((R, 2, LC), seed=616)))
    p = {k: v.data_ptr() for k, v in t.items()}
    ddim, dpm = make_sampling_scheduler(4), make_sampling_scheduler(4, sampler="dpmpp_2m")
    ts, a_t, a_prev, beta, _anc = _step_tables(ddim)
    sched_ddim = dict(n_steps=4, timesteps=_i64(ts), a_t=_f32(a_t), a_prev=_f32(a_prev), beta_t=_f32(beta), pred_type=PRED[ddim.prediction_type])
    ts, a_t, cx, c0, c1 = _multistep_tables(dpm)
    sched_ms = dict(n_steps=4, timesteps=_i64(ts), a_t=_f32(a_t), cx=_f32(cx), c0=_f32(c0), c1=_f32(c1), pred_type=PRED[dpm.prediction_type])
    e = scheduler_edit_tables(ddim, 1.0)
    edit_ddim = dict(n_steps=4, timesteps=_i64(e["timesteps"]), a_t=_f32(e["a_t"]), a_prev=_f32(e["a_prev"]), a_next=_f32(e["a_next"]),
                     pred_type=PRED[ddim.prediction_type])
    e = scheduler_edit_tables(dpm, 1.0)
    edit_ms = dict(n_steps=4, timesteps=_i64(e["timesteps"]), a_t=_f32(e["a_t"]), cx=_f32(e["cx"]), c0=_f32(e["c0"]), c1=_f32(e["c1"]),
                   a_next=_f32(e["a_next"]), pred_type=PRED[dpm.prediction_type])
    rt = scheduler_resample_tables(dpm, e, 2, 1)
    assert len(rt["timesteps"]) == 7 and any(rt["jump_n"])
    jumps = dict(n_steps=7, timesteps=_i64(rt["timesteps"]), a_t=_f32(rt["a_t"]), cx=_f32(rt["cx"]), c0=_f32(rt["c0"]), c1=_f32(rt["c1"]),
                 a_next=_f32(rt["a_next"]), jump_x=_f32(rt["jump_x"]), jump_n=_f32(rt["jump_n"]), noise_seed=RESAMPLE_KEY + 5,
                 pred_type=PRED[dpm.prediction_type])
    window = dict(B=B, L=L, noise=p["noise"])
    canvas = dict(R=R, W=W, L=L, m=M, r=RAMP, noise=p["cnoise"])
    classes = dict(labels=_i64([2, 0]), guidance_scale=3.0, null_class=1)
    pixel_w = {"latents_out": (B, 1, L), "windows_out": (B, 1, L)}
    ldm_w = {"latents_out": (B, 1, L), "windows_out": (B, 1, L * down)}
    pixel_c = {"canvas_out": (R, 1, LC), "recording_out": (R, 1, LC)}
    ldm_c = {"canvas_out": (R, 1, LC), "recording_out": (R, 1, LC * down)}
    forms = {
        "eegldm_sample": (dict(window, unet=plain.h, ae=ae.h, inv_scale_factor=0.7, **sched_ddim), ldm_w),
        "eegldm_sample_cond": (dict(window, unet=cond.h, inv_scale_factor=1.0, **sched_ddim, **classes), pixel_w),
        "eegldm_sample_multistep": (dict(window, unet=plain.h, ae=ae.h, inv_scale_factor=0.7, **sched_ms), ldm_w),
        "eegldm_sample_edit": (dict(window, unet=plain.h, inv_scale_factor=1.0, known=p["known"], mask=p["mask"], **edit_ddim), pixel_w),
        "eegldm_sample_long": (dict(canvas, unet=cond.h, ae=ae.h, inv_scale_factor=0.7, **sched_ms, **classes), ldm_c),
        "eegldm_sample_long_edit": (dict(canvas, unet=plain.h, inv_scale_factor=1.0, known=p["cknown"], mask=p["cmask"], **edit_ms), pixel_c),
        "eegldm_sample_edit_resample": (dict(window, unet=plain.h, inv_scale_factor=1.0, known=p["known"], mask=p["mask"], **jumps), pixel_w),
        "eegldm_sample_long_edit_resample": (dict(canvas, unet=plain.h, ae=ae.h, inv_scale_factor=0.7, known=p["cknown"], mask=p["cmask"], **jumps),
                                             ldm_c),
        "eegldm_sample_edit_ctx": (dict(window, unet=ctxn.h, inv_scale_factor=1.0, known=p["known"], mask=p["mask"], context=p["context"],
                                        context_rows=B, **jumps), pixel_w),
        "eegldm_sample_long_edit_ctx": (dict(canvas, unet=ctxn.h, inv_scale_factor=1.0, known=p["cknown"], mask=p["cmask"], context=p["ccontext"],
                                             context_rows=R, **edit_ms), pixel_c),
    }
    assert set(forms) == set(ORDER)
    return forms, (plain, cond, ctxn, ae, t)


def _outputs(shapes):
    return {k: torch.full(s, float("nan"), device="cuda:0") for k, s in shapes.items()}


def _run_desc(members, shapes, graph=0):
    """eegldm_sample_run on a descriptor holding `members` and fresh outputs -> (rc, outputs, graph_used)"""
    from eegldm._lib import SampleDesc, lib
    outs, used = _outputs(shapes), C.c_int(-1)
    d = SampleDesc(size=C.sizeof(SampleDesc), use_graph=graph, graph_used=C.pointer(used), **members, **{k: v.data_ptr() for k, v in outs.items()})
    rc = lib.eegldm_sample_run(C.byref(d))
    torch.cuda.synchronize()
    return rc, outs, used.value


def _run_export(name, members, shapes, graph=0):
    """the positional export `name` on the same members: an argument the form does not use is NULL / 0"""
    from eegldm._lib import lib
    outs, used = _outputs(shapes), C.c_int(-1)
    given = dict(members, use_graph=graph, graph_used=C.byref(used), **{k: v.data_ptr() for k, v in outs.items()})
    rc = getattr(lib, name)(*[given.get(k, 0 if k in _NUMBERS else None) for k in ORDER[name].split()])
    torch.cuda.synchronize()
    return rc, outs, used.value


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("name", sorted(ORDER))
def test_export_and_descriptor_return_the_same_bytes(name, graph):
    from eegldm._lib import lib
    members, shapes = _forms()[0][name]
    rc_a, a, used_a = _run_export(name, members, shapes, graph)
    assert rc_a == 0, lib.eegldm_last_error()
    rc_b, b, used_b = _run_desc(members, shapes, graph)
    assert rc_b == 0, lib.eegldm_last_error()
    for k in shapes:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), k
    assert used_a == used_b and used_a in (0, 1)


def _without(members, *names):
    return {k: v for k, v in members.items() if k not in names}


def _refusals():
    """(what is wrong, the valid form it is derived from, the broken members, the outputs it asks for)"""
    forms, (_plain, _cond, _ctxn, _ae_, t) = _forms()
    ms, shapes_w = forms["eegldm_sample_multistep"]
    ed, _ = forms["eegldm_sample_edit"]
    rs, _ = forms["eegldm_sample_edit_resample"]
    lg, shapes_c = forms["eegldm_sample_long"]
    bad_jump_n = _f32([0.5] + list(rs["jump_n"])[1:])
    bad_c1 = _f32([0.25] + list(ms["c1"])[1:])
    return [
        ("a mask without known", "eegldm_sample_multistep", dict(ms, mask=t["mask"].data_ptr()), shapes_w),
        ("jump_x without jump_n", "eegldm_sample_edit_resample", _without(rs, "jump_n"), shapes_w),
        ("jump_n[0] != 0", "eegldm_sample_edit_resample", dict(rs, jump_n=bad_jump_n), shapes_w),
        ("c1[0] != 0", "eegldm_sample_multistep", dict(ms, c1=bad_c1), shapes_w),
        ("the canvas form without cx", "eegldm_sample_long", dict(_without(lg, "cx"), a_prev=lg["a_t"]), shapes_c),
        ("L < 3 m + 2 r", "eegldm_sample_long", dict(lg, m=20, r=8), shapes_c),
        ("labels on an unconditional UNet", "eegldm_sample_multistep", dict(ms, labels=_i64([0, 0]), guidance_scale=1.0), shapes_w),
        ("a context on a plain UNet", "eegldm_sample_multistep", dict(ms, context=t["context"].data_ptr(), context_rows=B), shapes_w),
        ("ancestral with known", "eegldm_sample_edit", dict(ed, ancestral=1, beta_t=ed["a_t"]), shapes_w),
        ("no output pointer at all", "eegldm_sample_multistep", ms, {}),
    ]


@pytest.mark.parametrize("i", range(10))
def test_descriptor_refusals_leave_no_state(i):
    from eegldm._lib import lib
    what, name, broken, asked = _refusals()[i]
    members, shapes = _forms()[0][name]
    rc, want, _used = _run_desc(members, shapes)
    assert rc == 0, lib.eegldm_last_error()
    rc, _outs, _used = _run_desc(broken, asked)
    msg = lib.eegldm_last_error()
    print(f"{what}: rc {rc}, {msg!r}")
    assert rc != 0 and msg, what
    rc, got, _used = _run_desc(members, shapes)
    assert rc == 0, lib.eegldm_last_error()
    for k in shapes:
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], want[k]), (what, k)
