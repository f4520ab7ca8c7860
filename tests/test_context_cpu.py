"""CPU: context conditioning without a device -- the numpy restatement of the mask draw (tests/context_ref.py, which the GPU tests hold the
kernels to bit for bit), every refusal of the Python layer as a ValueError before the device is touched, and the scripts' flag,
checkpoint and resume logic with the recognition of a context checkpoint."""
import argparse
import types

import numpy as np
import pytest
import torch

import context_ref as R


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_philox_zero_vector_and_counter_sensitivity():
    """The one Random123 known-answer vector of Philox4x32-10 this generator can reach (its counter's upper two words are always zero):
    counter and key all zero.  Beyond it only that neighbouring counters give different 32-bit words; the values themselves are pinned to
    the device generator by the bit-equality tests of tests/test_gpu_context.py."""
    w = R.philox4x32(0, np.zeros(1, np.uint64))
    assert [int(v[0]) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    a = R.philox4x32(0xFFFFFFFFFFFFFFFF, np.array([0xFFFFFFFFFFFFFFFF], np.uint64))
    b = R.philox4x32(0xFFFFFFFFFFFFFFFF, np.array([0xFFFFFFFFFFFFFFFE], np.uint64))
    assert all(0 <= int(v[0]) < 2 ** 32 for v in a) and [int(v[0]) for v in a] != [int(v[0]) for v in b]


def test_the_three_kinds():
    B, L = 512, 96
    none = R.draw_mask(B, L, 1.0, 0.0, 3, 48, 1, 0)
    # (u0 == 1.0 -- a word that rounds to 2^32 -- would fall through to a span even at p_none = 1: not in these 512)
    assert (none == 0).all()
    kind, r0, r1 = R.draw_intervals(B, L, 0.0, 1.0, 3, 48, 2, 0)
    pre = R.draw_mask(B, L, 0.0, 1.0, 3, 48, 2, 0)
    assert (kind == R.PREFIX).all() and (r1 == L).all() and r0.min() >= 1 and r0.max() <= L - 1
    assert all((pre[b, :r0[b]] == 1).all() and (pre[b, r0[b]:] == 0).all() for b in range(B))
    assert len(set(r0.tolist())) > 40                                   # the split point moves
    kind, r0, r1 = R.draw_intervals(B, L, 0.0, 0.0, 3, 48, 3, 0)
    span = R.draw_mask(B, L, 0.0, 0.0, 3, 48, 3, 0)
    ln = r1 - r0
    assert (kind == R.SPAN).all() and ln.min() >= 3 and ln.max() <= 48 and r0.min() >= 0 and r1.max() <= L
    assert {3, 48} <= set(ln.tolist()) and 0 in r0.tolist()             # both ends of both ranges are reached
    assert ((span == 0).sum(1) == ln).all()
    # the offset is the sample index: row b of a draw at offset o is row 0 of a draw at offset o + b
    full = R.draw_mask(8, L, 0.1, 0.3, 3, 48, 4, 100)
    assert all(np.array_equal(R.draw_mask(1, L, 0.1, 0.3, 3, 48, 4, 100 + b)[0], full[b]) for b in range(8))
    assert np.array_equal(R.draw_mask(3, L, 0.1, 0.3, 3, 48, 4, 2 ** 64 - 1)[1], R.draw_mask(1, L, 0.1, 0.3, 3, 48, 4, 0)[0])      # the counter wraps


def test_edge_lengths():
    for pn, pp in ((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.3, 0.3)):
        assert (R.draw_mask(64, 1, pn, pp, 1, 1, 5, 0) == 0).all()       # L == 1: nothing can be kept (a prefix of L == 1 is all 0 too)
    m = R.draw_mask(64, 17, 0.0, 0.0, 17, 17, 6, 0)                      # span_min == span_max == L: the whole sample
    assert (m == 0).all()
    kind, r0, r1 = R.draw_intervals(64, 2, 0.0, 1.0, 1, 2, 7, 0)         # L == 2: the prefix keeps exactly one position
    assert (r0 == 1).all()


def test_shares_of_the_committed_seed():
    """The condition tests/test_gpu_context.py::test_mask_draw_kinds_and_shares asserts on the device, checked on the restatement first."""
    B, pn, pp = 4096, 0.1, 0.3
    kind, _r0, _r1 = R.draw_intervals(B, 96, pn, pp, 3, 48, 20240611, 0)
    for k, p in ((R.NONE, pn), (R.PREFIX, pp), (R.SPAN, 1.0 - pn - pp)):
        assert abs(int((kind == k).sum()) - B * p) <= 4 * (B * p * (1 - p)) ** 0.5


def test_restatement_refusals():
    for bad in ((0.1, 0.3, 0, 48), (0.1, 0.3, 5, 4), (0.1, 0.3, 3, 97), (-0.1, 0.3, 3, 48), (0.1, 1.5, 3, 48), (0.8, 0.3, 3, 48)):
        with pytest.raises(ValueError):
            R.draw_mask(2, 96, *bad, 1, 0)


# ------------------------------------------------------------------------------------------------------------------ refusals of the Python layer
class _Untouchable:
    """Stands where the scheduler / the device objects go: any use means the refusal came too late."""
    def __getattr__(self, name):
        raise AssertionError(f"touched ({name}) before the arguments were refused")


def _stub_unet(context_channels=0, num_classes=None):
    return types.SimpleNamespace(context_channels=context_channels, num_classes=num_classes, device="cpu", x_channels=1, in_channels=1 + context_channels)


def test_draw_arguments():
    from eegldm.training import context_draw_args
    assert context_draw_args({}, 96) == (0.1, 0.3, 3, 48)               # the defaults: L / 32 and L / 2
    assert context_draw_args({}, 8) == (0.1, 0.3, 1, 4) and context_draw_args({}, 1) == (0.1, 0.3, 1, 1)
    assert context_draw_args(dict(p_none=0.0, p_prefix=1.0, span_min=2, span_max=2), 64) == (0.0, 1.0, 2, 2)
    for bad in (dict(span_min=0), dict(span_min=5, span_max=4), dict(span_max=97), dict(p_none=-0.1), dict(p_prefix=1.5),
                dict(p_none=0.8, p_prefix=0.3), dict(spans=3)):
        with pytest.raises(ValueError):
            context_draw_args(bad, 96)


def test_train_step_refusals_come_before_the_device():
    from eegldm.training import add_noise_context, context_mask, context_window, dm_train_step, ldm_train_step
    B, L = 2, 64
    lat, mask = torch.zeros(B, 1, L), torch.ones(B, L)
    boom = _Untouchable()
    plain, ctx2, ctx3 = _stub_unet(0), _stub_unet(2), _stub_unet(3)
    for step in (ldm_train_step, dm_train_step):
        bad = [(plain, dict(context_mask=mask)), (plain, dict(context_mask={})), (plain, dict(context_latents=lat)), (plain, dict(mask_out=mask)),
               (ctx2, dict()),                                                               # a context model needs the mask
               (ctx3, dict(context_mask=mask)),                                              # the step forms C + 1 = 2 context channels
               (ctx2, dict(context_mask=mask[:, :-1])), (ctx2, dict(context_mask=torch.ones(B, 1, L))), (ctx2, dict(context_mask="span")),
               (ctx2, dict(context_mask=mask, context_latents=torch.zeros(B, 2, L))),
               (ctx2, dict(context_mask=dict(span_min=0))), (ctx2, dict(context_mask=dict(p_none=0.9, p_prefix=0.2))),
               (ctx2, dict(context_mask=dict(span_max=L + 1))), (ctx2, dict(context_mask=mask, mask_out=torch.zeros(B, L)))]      # mask_out on the host
        for unet, kw in bad:
            with pytest.raises(ValueError):
                step(unet, boom, lat, lat, torch.zeros(B, dtype=torch.int64), **kw)
    with pytest.raises(ValueError):
        add_noise_context(plain, boom, lat, lat, torch.zeros(B, dtype=torch.int64), mask)
    with pytest.raises(ValueError):
        context_mask(boom, B, L, dict(span_max=L + 1))
    with pytest.raises(ValueError):
        context_mask(boom, 0, L)
    for w, m, down in ((torch.zeros(B, 1, 4 * L), mask, 3), (torch.zeros(B, 1, 4 * L), mask[:1], 4), (torch.zeros(B, 1, 4 * L), mask, 0),
                       (torch.zeros(B, 4 * L), mask, 4)):
        with pytest.raises(ValueError):
            context_window(boom, w, m, down)


@pytest.mark.parametrize("fn", ["sample", "ddim_sample_hostloop"])
def test_sampler_refusals_come_before_the_device(fn):
    from test_edit_cpu import _fake_scheduler
    from eegldm import sampling, schedulers as S
    run = getattr(sampling, fn)
    B, L = 2, 64
    ae = types.SimpleNamespace(down=4, in_channels=1, out_channels=1)
    noise, init, mask = torch.zeros(B, 1, L), torch.zeros(B, 1, 4 * L), torch.ones(B, 1, 4 * L)
    ddim, dpm, ddpm = (_fake_scheduler(c) for c in (S.DDIMScheduler, S.DPMSolverMultistepScheduler, S.DDPMScheduler))
    plain, ctx = _stub_unet(0), _stub_unet(2)
    good = torch.zeros(B, 2, L)
    bad = [(plain, ddim, dict(context=good)), (plain, dpm, dict(init=init, mask=mask, blend=False)),            # a plain model has no context
           (ctx, ddim, dict(context=torch.zeros(B, 3, L))), (ctx, ddim, dict(context=torch.zeros(B, 2, L + 1))), (ctx, dpm, dict(context=torch.zeros(3, 2, L))),
           (ctx, ddim, dict(context=good.numpy())), (ctx, ddim, dict(context=good[:, :, None])),
           (ctx, dpm, dict(init=init, mask=mask, resamples=2, blend=False)),                                    # resampling needs the blend
           (ctx, ddpm, dict(init=init, mask=mask)), (ctx, ddpm, dict(context=good)),                            # the ancestral scheduler stays refused
           (ctx, ddim, dict(mask=mask, blend=False)), (ctx, ddim, dict(init=init, blend=False, composite=True))]
    for unet, sched, kw in bad:
        with pytest.raises(ValueError):
            run(unet, ae, sched, noise, **kw)


@pytest.mark.parametrize("fn", ["sample_long", "sample_long_hostloop"])
def test_long_sampler_refusals(fn):
    from test_edit_cpu import _fake_scheduler
    from eegldm import sampling, schedulers as S
    run = getattr(sampling, fn)
    dpm = _fake_scheduler(S.DPMSolverMultistepScheduler)
    R_, W, L, m, r = 2, 3, 64, 4, 8
    Lc = sampling.long_layout(W, L, m, r).canvas_len
    noise = torch.zeros(R_, 1, Lc)
    plain, ctx = _stub_unet(0), _stub_unet(2)
    for unet, kw in ((plain, dict(context=torch.zeros(R_, 2, Lc))), (plain, dict(blend=False)), (ctx, dict(context=torch.zeros(R_, 2, L))),
                     (ctx, dict(context=torch.zeros(1, 2, Lc))), (ctx, dict(context=torch.zeros(R_, 3, Lc))),
                     (ctx, dict(init_canvas=torch.zeros(R_, 1, Lc), mask=torch.ones(R_, 1, Lc), resamples=2, blend=False))):
        with pytest.raises(ValueError):
            run(unet, None, dpm, noise, W, margin=m, ramp=r, **kw)


# ------------------------------------------------------------------------------------------------------------------ scripts
def _args(**kw):
    base = dict(context=False, ctx_p_none=None, ctx_p_prefix=None, ctx_span_min=None, ctx_span_max=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_flags_and_checkpoint_entry():
    from eegldm.entry import train_dm, train_ldm
    from eegldm.entry.common import context_entry
    for mod, req in ((train_ldm, ["--config_file", "c.yaml", "--autoencoderkl_config_file_path", "a.yaml"]), (train_dm, ["--config_file", "c.yaml"])):
        a = mod.parse_args(req)
        assert a.context is False and a.ctx_p_none is None and a.ctx_span_max is None and context_entry(a, 1, 96) is None
        a = mod.parse_args(req + ["--context", "--ctx_p_none", "0.2", "--ctx_span_min", "5"])
        assert context_entry(a, 1, 96) == {"context_channels": 2, "p_none": 0.2, "p_prefix": 0.3, "span_min": 5, "span_max": 48}
    assert context_entry(_args(context=True), 3, 96) == {"context_channels": 4, "p_none": 0.1, "p_prefix": 0.3, "span_min": 3, "span_max": 48}
    assert context_entry(_args(context=True), 1, 3072)["span_min"] == 96 and context_entry(_args(context=True), 1, 3072)["span_max"] == 1536
    with pytest.raises(ValueError, match="--context"):
        context_entry(_args(ctx_p_none=0.2), 1, 96)                      # a draw flag without --context
    for bad in (dict(ctx_span_min=0), dict(ctx_span_max=200), dict(ctx_p_none=0.9, ctx_p_prefix=0.2), dict(ctx_span_min=50, ctx_span_max=49)):
        with pytest.raises(ValueError):
            context_entry(_args(context=True, **bad), 1, 96)


def test_resume_restores_and_refuses():
    from eegldm.entry.common import context_entry, context_resume
    saved = {"context_channels": 2, "p_none": 0.2, "p_prefix": 0.3, "span_min": 5, "span_max": 48}
    a = _args()
    context_resume(a, {"context": dict(saved)})                          # no flag: everything comes back
    assert a.context and context_entry(a, 1, 96) == saved
    a = _args(context=True, ctx_p_none=0.2)
    context_resume(a, {"context": dict(saved)})                          # an agreeing flag is fine
    assert context_entry(a, 1, 96) == saved
    for bad in (dict(ctx_p_none=0.1), dict(ctx_span_max=40), dict(ctx_span_min=6), dict(ctx_p_prefix=0.0)):
        with pytest.raises(ValueError, match="checkpoint"):
            context_resume(_args(context=True, **bad), {"context": dict(saved)})
    with pytest.raises(ValueError, match="without --context"):
        context_resume(_args(context=True), {"epoch": 1})
    a = _args()
    context_resume(a, {"epoch": 1})                                     # a plain checkpoint, no flag: nothing changes
    assert a.context is False and context_entry(a, 1, 96) is None


def test_recognition_of_a_context_checkpoint(tmp_path):
    from eegldm.entry.common import context_model_kwargs, context_of_checkpoint
    def sd(cin, out, prefix=""):
        return {prefix + "input_blocks.0.0.weight": torch.zeros(32, cin, 3), prefix + "out.2.weight": torch.zeros(out, 32, 3)}
    assert context_of_checkpoint(sd(3, 1)) == 2 and context_of_checkpoint(sd(7, 3)) == 4 and context_of_checkpoint(sd(3, 1, "module.")) == 2
    assert context_of_checkpoint(sd(1, 1)) == 0 and context_of_checkpoint(sd(3, 3)) == 0 and context_of_checkpoint(sd(4, 1)) == 0
    assert context_of_checkpoint({"diffusion": sd(3, 1), "epoch": 2}) == 2 and context_of_checkpoint({"diffusion": sd(1, 1), "epoch": 2}) == 0
    assert context_of_checkpoint({"diffusion": sd(1, 1), "context": {"context_channels": 2}}) == 2         # the entry decides
    assert context_of_checkpoint({}) == 0
    up = dict(in_channels=1, out_channels=1)
    assert context_model_kwargs(up, sd(1, 1)) == {} and up["in_channels"] == 1
    assert context_model_kwargs(up, sd(3, 1)) == {"context_channels": 2} and up["in_channels"] == 3
    # a run directory: checkpoint.pth decides, whatever weights file is sampled from
    torch.save({"diffusion": sd(3, 1), "context": {"context_channels": 2, "p_none": 0.1, "p_prefix": 0.3, "span_min": 3, "span_max": 48}},
               tmp_path / "checkpoint.pth")
    up = dict(in_channels=1, out_channels=1)
    assert context_model_kwargs(up, sd(3, 1), str(tmp_path)) == {"context_channels": 2} and up["in_channels"] == 3
    from eegldm.entry import edit_long, edit_trials
    base = ["--output_dir", "o", "--diffusion_path", "d", "--input", "x.npy"]
    assert edit_trials.parse_args(base).no_blend is False and edit_trials.parse_args(base + ["--no_blend"]).no_blend is True
    assert hasattr(edit_long.parse_args(base + ["--no_blend"]), "no_blend")
