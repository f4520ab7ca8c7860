"""Long recordings (overlapped windows on one canvas), host side, no GPU: the layout, the refusals (raised before anything touches a
model or a device), the hypnogram-to-window mapping, tools/seam_report.py, the ctypes table, and the torch reference composition
(sample_long_hostloop) against the per-window host loop when the windows do not overlap."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from test_dpm_solver_cpu import T, _acp
from test_edit_cpu import _Boom, _fake_scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(1, 16, 0, 0), (1, 28, 4, 8), (2, 16, 4, 0), (3, 64, 4, 8), (5, 64, 3, 5), (3, 28, 4, 8), (4, 12, 4, 0), (2, 7, 1, 2), (5, 16, 0, 0),
         (3, 768, 18, 36), (2, 64, 0, 7)]


@pytest.mark.parametrize("W,L,m,r", CASES)
def test_stride_canvas_length_and_partition_of_unity(W, L, m, r):
    from eegldm.sampling import long_layout
    lay = long_layout(W, L, m, r)
    S = L - (2 * m + r)
    assert lay.stride == S >= 1 and lay.canvas_len == (W - 1) * S + L and lay.starts == [k * S for k in range(W)]
    total = np.zeros(lay.canvas_len, np.float32)
    nonzero = np.zeros(lay.canvas_len, int)
    covered = np.zeros(lay.canvas_len, int)
    for k in range(W):
        w = lay.weights(k)
        assert w.dtype == np.float32 and w.shape == (L,) and (w >= 0).all() and (w <= 1).all()
        total[k * S:k * S + L] += w                    # float32 accumulation: at most two terms are non-zero anywhere
        nonzero[k * S:k * S + L] += w != 0
        covered[k * S:k * S + L] += 1
        # the issue's definition, position by position
        for j in range(L):
            want = 1.0
            if k > 0 and j < m + r:
                want = 0.0 if j < m else (j - m + 0.5) / r
            if k < W - 1 and j >= S + m:
                jn = j - S
                un = 0.0 if jn < m else ((jn - m + 0.5) / r if jn < m + r else 1.0)
                want = float(np.float32(1.0) - np.float32(un))
            assert w[j] == np.float32(want), (k, j, w[j], want)
    assert (total == np.float32(1.0)).all(), "the weights do not sum to exactly 1.0 in float32"
    assert ((nonzero == 1) | (nonzero == 2)).all() and (covered >= 1).all()
    assert (nonzero[:m + S] == 1).all() if W > 1 else (nonzero == 1).all()
    # every window-local position maps to exactly one canvas position, and each canvas position is hit by each covering window once
    hits = {}
    for k in range(W):
        for j in range(L):
            hits.setdefault((k, lay.starts[k] + j), []).append(j)
    assert all(len(v) == 1 for v in hits.values()) and len(hits) == W * L
    assert max(p for _k, p in hits) == lay.canvas_len - 1 and min(p for _k, p in hits) == 0
    # the owner table names a window of weight > 0, and its ramps are the seams
    k1, j = lay.owner()
    for p in range(lay.canvas_len):
        assert 0 <= j[p] < L and lay.weights(int(k1[p]))[j[p]] > 0
    assert lay.seams() == [(k * S + m, k * S + m + r) for k in range(1, W)]


def test_free_ends_keep_weight_one_and_m_r_zero_is_side_by_side():
    from eegldm.sampling import long_layout
    lay = long_layout(3, 64, 4, 8)
    assert (lay.weights(0)[:48 + 4] == 1).all() and (lay.weights(2)[12:] == 1).all() and (lay.weights(1)[:4] == 0).all() and (lay.weights(1)[-4:] == 0).all()
    assert lay.weights(1)[4] == np.float32(0.5 / 8) and lay.weights(0)[48 + 4] == np.float32(1.0) - np.float32(0.5 / 8)
    flat = long_layout(4, 16, 0, 0)
    assert flat.stride == 16 and flat.canvas_len == 64 and all((flat.weights(k) == 1).all() for k in range(4))
    with pytest.raises(IndexError):
        lay.weights(3)


@pytest.mark.parametrize("W,L,m,r", [(0, 16, 0, 0), (-1, 16, 0, 0), (2, 16, -1, 0), (2, 16, 0, -1), (2, 27, 4, 8), (2, 16, 4, 8), (2, 11, 4, 0),
                                      (1, 0, 0, 0), (2, 16, 3, 4)])
def test_layout_refusals(W, L, m, r):
    from eegldm.sampling import long_layout
    with pytest.raises(ValueError):
        long_layout(W, L, m, r)


@pytest.mark.parametrize("W,L,m,r", CASES)
@pytest.mark.parametrize("down", [1, 4])
def test_scaled_layout_is_consistent(W, L, m, r, down):
    from eegldm.sampling import long_layout
    lay = long_layout(W, L, m, r)
    big = lay.scaled(down)
    assert (big.n_windows, big.window_len, big.margin, big.ramp, big.stride) == (W, L * down, m * down, r * down, lay.stride * down)
    assert big.canvas_len == lay.canvas_len * down and big.starts == [s * down for s in lay.starts]
    assert big.seams() == [(a * down, b * down) for a, b in lay.seams()]
    # weight 0 / weight 1 / ramp regions of the scaled layout are the latent layout's, position by position
    for k in range(W):
        a, b = lay.weights(k), big.weights(k)
        kind = lambda w: np.where(w == 0, 0, np.where(w == 1, 2, 1))
        assert (np.repeat(kind(a), down) == kind(b)).all()


def test_hypnogram_to_window_mapping():
    from eegldm.sampling import long_layout, window_labels_from_hypnogram
    # latent layout of the 3072-sample window: S = 696 latents = 27.84 s, centres at 15.36 + 27.84 k seconds
    lay = long_layout(5, 768, 18, 36)
    assert lay.stride == 696
    stages = [0, 2, 2, 4, 1]                      # epochs [0, 30), [30, 60), ...
    # centres: 15.36, 43.20, 71.04, 98.88, 126.72 s -> epochs 0, 1, 2, 3, 4
    assert list(window_labels_from_hypnogram(stages, lay, down=4, sfreq=100.0)) == [0, 2, 2, 4, 1]
    # a longer run drifts against the epochs (27.84 s per window, 30 s per epoch): centres 15.36 + 27.84 k, so windows 7 and 8 (210.24 s
    # and 238.08 s) both fall into epoch 7 and every later window is one epoch behind its index
    lay = long_layout(14, 768, 18, 36)
    got = window_labels_from_hypnogram(np.arange(14), lay, down=4)
    assert list(got) == [0, 1, 2, 3, 4, 5, 6, 7, 7, 8, 9, 10, 11, 12]
    # pixel space, no overlap: 30.72-s windows centred at 15.36, 46.08, 76.8 s
    flat = long_layout(3, 3072, 0, 0)
    assert list(window_labels_from_hypnogram([3, 1, 0], flat, down=1)) == [3, 1, 0]
    with pytest.raises(ValueError):
        window_labels_from_hypnogram([0, 1], long_layout(3, 768, 18, 36), down=4)


def test_seam_report_flags_the_planted_step_only():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import seam_report as SR
    from eegldm.entry.sample_long import layout_json
    from eegldm.sampling import long_layout
    lay = long_layout(4, 192, 6, 12)
    lj = layout_json(lay, 4, crop=36)
    assert lj["S"] == 4 * lay.stride and lj["samples"] == 4 * lay.canvas_len - 72 and len(lj["seams"]) == 3
    rng = np.random.default_rng(5)
    n = lj["samples"]
    x = np.cumsum(rng.standard_normal(n)) * 0.05 + rng.standard_normal(n) * 0.1          # smooth-ish signal
    a, b = lj["seams"][1]
    x[(a + b) // 2:] += 5.0                            # a step in the middle of seam 2
    rep = SR.seam_report(x[None, None, :], lj)
    ratios = [s["ratio_diff_rms"] for s in rep["seams"]]
    assert ratios[1] > 3.0 and ratios[0] < 1.5 and ratios[2] < 1.5, ratios
    assert [s["span"] for s in rep["seams"]] == [list(s) for s in lj["seams"]]
    # a hard switch (ramp 0) is looked at over the samples around it
    hard = layout_json(long_layout(3, 64, 4, 0), 1, crop=0)
    y = rng.standard_normal(hard["samples"]) * 0.1
    y[hard["seams"][0][0]:] += 3.0
    rep = SR.seam_report(y, hard, halfwidth=4)
    assert rep["seams"][0]["ratio_diff_rms"] > 3.0 and rep["seams"][1]["ratio_diff_rms"] < 2.0


def test_refusals_come_before_any_device_work():
    from eegldm import sampling, schedulers as S
    ae = types.SimpleNamespace(down=4, in_channels=1, out_channels=1)
    ddim, dpm, ddpm = (_fake_scheduler(c) for c in (S.DDIMScheduler, S.DPMSolverMultistepScheduler, S.DDPMScheduler))
    lay = sampling.long_layout(3, 64, 4, 8)
    good = torch.zeros(2, 1, lay.canvas_len)
    for fn in (sampling.sample_long, sampling.sample_long_hostloop):
        bad = [
            (ddim, good, 3, dict(margin=4, ramp=8)), (ddpm, good, 3, dict(margin=4, ramp=8)),                   # not the multistep scheduler
            (dpm, good[:, :, :-1], 3, dict(margin=4, ramp=8)), (dpm, good[0], 3, dict(margin=4, ramp=8)),      # not (R, C, Lc)
            (dpm, good, 0, dict(margin=4, ramp=8)), (dpm, good, 3, dict(margin=-1, ramp=8)), (dpm, good, 3, dict(margin=4, ramp=-8)),
            (dpm, torch.zeros(2, 1, 2 * 4 + 16), 2, dict(margin=4, ramp=8)),                                  # L = 16 < 3 m + 2 r
            (dpm, good, 3, dict(margin=4, ramp=8, labels=[0, 1])), (dpm, good, 3, dict(margin=4, ramp=8, labels=[0] * 5)),      # not W or R W labels
        ]
        for sched, nz, W, kw in bad:
            with pytest.raises(ValueError):
                fn(_Boom(), None, sched, nz, W, **kw)
        # the defaults come from crop and the autoencoder: 18 and 36 latents for crop 36, down 4
        full = sampling.long_layout(2, 768, 18, 36)
        with pytest.raises((AssertionError, TypeError), match="UNet"):
            fn(_Boom(), ae, dpm, torch.zeros(1, 1, full.canvas_len), 2)
        with pytest.raises(ValueError):
            fn(_Boom(), ae, dpm, torch.zeros(1, 1, full.canvas_len + 1), 2)
        # arguments that are fine get as far as the UNet
        with pytest.raises((AssertionError, TypeError), match="UNet"):
            fn(_Boom(), None, dpm, good, 3, margin=4, ramp=8, labels=[0, 1, 2])


def test_abi_table_and_argument_checks_without_a_device():
    from eegldm._lib import lib, SIGNATURES
    assert lib.eegldm_abi_version() == 8
    for name in ("eegldm_canvas_gather", "eegldm_canvas_step", "eegldm_canvas_compose", "eegldm_sample_long"):
        assert name in SIGNATURES and hasattr(lib, name)
    z = C.c_void_p(0)
    assert lib.eegldm_canvas_gather(z, z, 1, 1, 2, 16, 8, z, z) != 0 and b"null" in lib.eegldm_last_error()
    assert lib.eegldm_canvas_step(z, z, 0.0, 0, z, z, 0.5, 0, 0, 1.0, 1.0, 0.0, 1, 1, 2, 16, 4, 0, z, z, z, z) != 0
    assert lib.eegldm_canvas_compose(z, z, 1, 1, 2, 16, 8, 4, 0, z) != 0
    one, ts = (C.c_float * 1)(0.5), (C.c_int64 * 1)(999)
    assert lib.eegldm_sample_long(z, z, z, ts, one, one, one, one, 1, 0, 0, 1.0, z, z, 1, 2, 16, 4, 0, 0, None, None, 1.0, 0) != 0


def test_entry_script_flags_and_plan():
    from eegldm.entry import sample_long as E
    base = ["--output_dir", "o", "--diffusion_path", "d"]
    ldm = base + ["--best_model_path", "b", "--autoencoderkl_config_file_path", "a", "--ldm_config_file_path", "l"]
    a = E.parse_args(ldm + ["--n_windows", "3"])
    E.check_args(a)
    assert a.margin is None and a.ramp is None and a.seed == 0 and a.solver_order == 2 and not a.pixel and not a.use_ema
    lay = E.plan_layout(a, 768, 4)
    assert (lay.n_windows, lay.margin, lay.ramp, lay.stride) == (3, 18, 36, 696)
    # ten minutes: 60000 samples + the crop; 21 windows give 4 * (20 * 696 + 768) - 72 = 58680 < 60000, 22 give 61464
    b = E.parse_args(ldm + ["--minutes", "10"])
    lay = E.plan_layout(b, 768, 4)
    assert lay.n_windows == 22 and 4 * lay.canvas_len - 72 >= 60000 > 4 * (lay.canvas_len - lay.stride) - 72
    c = E.parse_args(base + ["--pixel", "--config_file", "c", "--minutes", "0.4", "--margin", "0", "--ramp", "0"])
    E.check_args(c)
    assert E.plan_layout(c, 3072, 1).n_windows == 1
    for bad in (ldm, ldm + ["--n_windows", "2", "--minutes", "1"], ldm + ["--n_windows", "0"], base + ["--n_windows", "2"],
                base + ["--pixel", "--n_windows", "2"], ldm + ["--n_windows", "2", "--hypnogram", "h.npy", "--class_label", "1"]):
        with pytest.raises(ValueError):
            E.check_args(E.parse_args(bad))


class _TinyNet(torch.nn.Module):
    """Stands where the UNet goes in the torch-only loop: two convolutions and a timestep shift, enough to make windows depend on their
    neighbours' absence (zero padding) and on the step."""

    def __init__(self, ch):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a, self.b = torch.nn.Conv1d(ch, 8, 3, padding=1), torch.nn.Conv1d(8, ch, 3, padding=1)
        for p in self.parameters():
            p.data = torch.randn(p.shape, generator=g) * 0.3
        self.device, self.in_channels = torch.device("cpu"), ch

    def forward(self, x, timesteps):
        return self.b(torch.tanh(self.a(x) + (timesteps.float() / 1000.0).view(-1, 1, 1)))


def _torch_step_scheduler(N, order, pred):
    """The fake multistep scheduler of tests/test_edit_cpu.py with a `step` in torch: float64 restatement of eegldm_multistep_step with
    its float32 roundings (products feed fused multiply-adds), so that ddim_sample_hostloop runs without a device."""
    from eegldm import schedulers as S
    s = _fake_scheduler(S.DPMSolverMultistepScheduler, N)
    ts = [int(t) for t in s.timesteps]
    s.cx, s.c0, s.c1 = S.multistep_coefficients(s.alphas_cumprod, ts, 1.0, order, True)
    s.prediction_type, s.clip_sample, s.solver_order = pred, False, order
    f32 = lambda v: v.to(torch.float32)
    state = {}

    def step(out, t, x, first_order=False):
        i = ts.index(int(t))
        a = np.float32(float(s.alphas_cumprod[int(t)]))
        sa, sb = float(np.sqrt(a)), float(np.sqrt(np.float32(1.0) - a))
        o64, x64 = out.double(), x.double()
        if pred == "epsilon":
            x0 = f32(f32(x64 - sb * o64).double() / sa)
        elif pred == "v_prediction":
            x0 = f32(sa * x64 - f32(sb * o64).double())
        else:
            x0 = out
        inner = f32(s.c0[i] * x0.double() + f32(s.c1[i] * state["h"].double()).double()) if s.c1[i] != 0.0 else f32(s.c0[i] * x0.double())
        state["h"] = x0
        return f32(s.cx[i] * x64 + inner.double()), x0
    s.step = step
    return s


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("order,N", [(1, 4), (2, 6)])
@pytest.mark.parametrize("R,W,Cc", [(1, 1, 1), (2, 3, 2), (1, 5, 1)])
def test_hostloop_without_overlap_is_the_per_window_loop(R, W, Cc, order, N, pred):
    """m = r = 0: the canvas is W windows side by side, so sample_long_hostloop has to return what ddim_sample_hostloop returns for the
    R * W windows as a batch, bit for bit (torch on the CPU, pixel-space call)."""
    from eegldm.sampling import ddim_sample_hostloop, sample_long_hostloop
    net, L = _TinyNet(Cc), 16
    sched = _torch_step_scheduler(N, order, pred)
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(R, Cc, W * L, generator=g)
    rec, canvas = sample_long_hostloop(net, None, sched, noise, W, margin=0, ramp=0, crop=2)
    rows = noise.reshape(R, Cc, W, L).permute(0, 2, 1, 3).reshape(R * W, Cc, L)
    _win, lat = ddim_sample_hostloop(net, None, _torch_step_scheduler(N, order, pred), rows, crop=0)
    want = lat.reshape(R, W, Cc, L).permute(0, 2, 1, 3).reshape(R, Cc, W * L)
    assert torch.isfinite(canvas).all() and float(canvas.abs().max()) > 0
    assert torch.equal(canvas, want)
    assert rec.shape == (R, Cc, W * L - 4) and torch.equal(rec, canvas[:, :, 2:-2])
    # with an overlap the windows see each other: the result differs, and the canvas is the shorter one
    if W > 1:
        from eegldm.sampling import long_layout
        lay = long_layout(W, L, 1, 2)
        rec2, canvas2 = sample_long_hostloop(net, None, _torch_step_scheduler(N, order, pred), noise[:, :, :lay.canvas_len], W, margin=1, ramp=2, crop=0)
        assert canvas2.shape == (R, Cc, lay.canvas_len) and torch.equal(rec2, canvas2) and torch.isfinite(canvas2).all()
