"""Sampling from an input (SDEdit / masked sampling), host side, no GPU: the start index, the truncated tables of both samplers, the
refusals (raised before anything touches a device) and the ctypes table.  The float64 restatement of the multistep coefficients is the
one tests/test_dpm_solver_cpu.py holds (`reference_coefficients`)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from test_dpm_solver_cpu import T, _acp, reference_coefficients


@pytest.mark.parametrize("n,s,want", [
    (50, 1.0, (0, 50)), (50, 0.5, (25, 25)), (50, 0.2, (40, 10)), (20, 0.8, (4, 16)),
    (50, 1e-9, (49, 1)), (1, 0.01, (0, 1)), (1, 1.0, (0, 1)),          # a tiny strength still runs one step
    (5, 0.5, (2, 3)), (5, 0.3, (3, 2)), (5, 0.1, (4, 1)), (3, 0.5, (1, 2)),      # 2.5 -> 3, 1.5 -> 2, 0.5 -> 1: ties go away from zero
    (10, 0.96, (0, 10)), (10, 0.94, (1, 9)),
])
def test_start_index(n, s, want):
    from eegldm.schedulers import edit_start_index
    i0, n_run = edit_start_index(n, s)
    assert (i0, n_run) == want and i0 + n_run == n and 1 <= n_run <= n


@pytest.mark.parametrize("s", [0.0, -0.1, 1.0000001, 2.0, float("nan"), float("inf")])
def test_start_index_refuses_strength_outside_unit_interval(s):
    from eegldm.schedulers import edit_start_index
    with pytest.raises(ValueError):
        edit_start_index(50, s)


@pytest.mark.parametrize("spacing", ["linspace", "leading"])
@pytest.mark.parametrize("final_is_one", [True, False])
@pytest.mark.parametrize("N,strength", [(20, 0.5), (20, 0.2), (20, 1.0), (12, 0.75), (50, 0.3), (5, 0.5), (2, 0.5), (1, 1.0)])
def test_truncated_multistep_table(N, strength, final_is_one, spacing):
    """c1 == 0 on the first entry; every later entry IS the full grid's; the first entry against the independent float64 restatement of the
    first-order coefficients of that step, to 1 ulp of float32 (both sides are float64 evaluations rounded once, the standard of
    tests/test_dpm_solver_cpu.py); a_next is the next grid point's alphas_cumprod and final_alpha_cumprod after the last step."""
    from eegldm.schedulers import edit_start_index, edit_tables, multistep_coefficients, multistep_timesteps
    acp = _acp()
    final = 1.0 if final_is_one else float(acp[0])
    ts = multistep_timesteps(T, N, spacing)
    cx, c0, c1 = multistep_coefficients(acp, ts, final, 2, True)
    tab = edit_tables(acp, ts, strength, final, multistep=dict(cx=cx, c0=c0, c1=c1, lower_order_final=True))
    i0, n_run = edit_start_index(N, strength)
    assert tab["i0"] == i0 and tab["timesteps"] == ts[i0:] and len(tab["cx"]) == len(tab["c0"]) == len(tab["c1"]) == len(tab["a_next"]) == n_run
    assert tab["c1"][0] == 0.0
    for name, full in (("cx", cx), ("c0", c0), ("c1", c1)):
        assert tab[name][1:] == list(full[i0 + 1:]), name          # bit-equal: the same Python floats
    wx, w0, w1 = reference_coefficients(acp, ts, final, solver_order=1)
    assert w1[i0] == 0.0
    for name, g, w in (("cx", tab["cx"][0], wx[i0]), ("c0", tab["c0"][0], w0[i0])):
        w32 = np.float32(w)
        assert float(np.float32(g)) == g, f"{name} is not rounded to float32"
        assert abs(g - float(w32)) <= float(np.spacing(np.abs(w32))), (name, g, float(w))
    if strength == 1.0:
        assert (tab["cx"], tab["c0"], tab["c1"]) == (list(cx), list(c0), list(c1))          # the whole grid: nothing changes
    assert tab["a_t"] == [float(acp[t]) for t in ts[i0:]]
    assert tab["a_next"] == [float(acp[t]) for t in ts[i0 + 1:]] + [final]
    assert "a_prev" not in tab


@pytest.mark.parametrize("N,strength", [(50, 0.5), (10, 0.3), (200, 0.12), (5, 1.0)])
def test_truncated_first_order_is_ddim(N, strength):
    """solver_order = 1 on DDIM's grid, truncated: the entries are the full table's (nothing to lower), and they carry DDIM's identities
    cx sigma_i = sigma_{i+1}, cx alpha_i + c0 = alpha_{i+1} with (a_t, a_prev) of the truncated DDIM table, to the float32 rounding of the
    coefficients (the bounds of test_first_order_is_ddim: 2^-24 and 2 x 2^-24, all values <= 1)."""
    from eegldm.schedulers import edit_tables, multistep_coefficients, multistep_timesteps
    acp = _acp()
    ts = multistep_timesteps(T, N, "leading")
    for final in (1.0, float(acp[0])):
        cx, c0, c1 = multistep_coefficients(acp, ts, final, 1)
        tab = edit_tables(acp, ts, strength, final, multistep=dict(cx=cx, c0=c0, c1=c1))
        ddim = edit_tables(acp, ts, strength, final, ddim_ratio=T // N)
        i0 = tab["i0"]
        assert (tab["cx"], tab["c0"]) == (list(cx[i0:]), list(c0[i0:])) and not any(tab["c1"])
        assert ddim["timesteps"] == tab["timesteps"] and ddim["a_t"] == tab["a_t"] and ddim["a_next"] == ddim["a_prev"] == tab["a_next"]
        a, ap = np.asarray(ddim["a_t"], np.float64), np.asarray(ddim["a_prev"], np.float64)
        assert np.abs(np.asarray(tab["cx"]) * np.sqrt(1 - a) - np.sqrt(1 - ap)).max() <= 2.0 ** -24
        assert np.abs(np.asarray(tab["cx"]) * np.sqrt(a) + np.asarray(tab["c0"]) - np.sqrt(ap)).max() <= 2 * 2.0 ** -24


@pytest.mark.parametrize("final_is_one", [True, False])
def test_ddim_a_next_table(final_is_one):
    from eegldm.schedulers import edit_tables
    acp = _acp()
    final = 1.0 if final_is_one else float(acp[0])
    N = 50
    ts = [int(v) for v in (np.arange(N) * (T // N))[::-1]]
    tab = edit_tables(acp, ts, 0.5, final, ddim_ratio=T // N)
    assert tab["i0"] == 25 and tab["timesteps"] == ts[25:] and tab["timesteps"][0] == 480
    want = [float(acp[t - 20]) if t - 20 >= 0 else final for t in ts[25:]]
    assert tab["a_prev"] == want and tab["a_next"] == want and tab["a_next"][-1] == final
    assert tab["a_prev"][:-1] == tab["a_t"][1:]
    with pytest.raises(ValueError):
        edit_tables(acp, ts, 0.5, final)                      # neither sampler named
    with pytest.raises(ValueError):
        edit_tables(acp, ts, 0.5, final, ddim_ratio=20, multistep=dict(cx=[], c0=[], c1=[]))


def _fake_scheduler(cls, N=10):
    """A scheduler object without a device: the attributes the table helper reads (the constructors open a GPU context)."""
    from eegldm import schedulers as S
    acp = torch.from_numpy(_acp()).float()
    s = object.__new__(cls)
    s.alphas_cumprod, s.num_train_timesteps, s.num_inference_steps, s.final_alpha_cumprod = acp, T, N, 1.0
    if cls is S.DPMSolverMultistepScheduler:
        ts = S.multistep_timesteps(T, N)
        s.cx, s.c0, s.c1 = S.multistep_coefficients(acp, ts, 1.0, 2, True)
        s.lower_order_final = True
    else:
        ts = [int(v) for v in (np.arange(N) * (T // N))[::-1]]
    s.timesteps = torch.tensor(ts)
    return s


class _Boom:
    """Stands where the UNet goes: any attribute access means the refusal came too late."""
    def __getattr__(self, name):
        raise AssertionError(f"the UNet was touched ({name}) before the arguments were refused")


@pytest.mark.parametrize("fn", ["sample", "ddim_sample_hostloop"])
def test_refusals_come_before_any_device_work(fn):
    from eegldm import sampling, schedulers as S
    run = getattr(sampling, fn)
    B, L = 2, 64
    ae = types.SimpleNamespace(down=4, in_channels=1, out_channels=1)
    noise, init, lat, mask = torch.zeros(B, 1, L), torch.zeros(B, 1, 4 * L), torch.zeros(B, 1, L), torch.ones(B, 1, 4 * L)
    ddim, dpm, ddpm = (_fake_scheduler(c) for c in (S.DDIMScheduler, S.DPMSolverMultistepScheduler, S.DDPMScheduler))
    bad = [
        (ddpm, dict(init=init)), (ddpm, dict(init=init, mask=mask)), (ddpm, dict(init_latents=lat)),           # ancestral sampler
        (ddim, dict(mask=mask)), (dpm, dict(mask=mask)),                                                      # mask without init
        (ddim, dict(init=init, strength=0.0)), (dpm, dict(init=init, strength=1.5)), (ddim, dict(init=init, strength=-1.0)),
        (ddim, dict(init=init, strength=float("nan"))), (ddim, dict(strength=0.0)),
        (ddim, dict(strength=0.5)),                                                                           # strength without init
        (ddim, dict(init=init[:, :, :-4])), (ddim, dict(init=init[:1])), (dpm, dict(init=torch.zeros(B, 2, 4 * L))),      # shapes
        (ddim, dict(init=lat)), (ddim, dict(init_latents=init)), (ddim, dict(init=init, init_latents=lat)),
        (ddim, dict(init=init, mask=mask[:, :, :-1])), (dpm, dict(init=init, mask=torch.ones(B, 1, L))), (ddim, dict(init=init, mask=mask[:1])),
        (ddim, dict(init=init, composite=True)), (ddim, dict(init_latents=lat, mask=mask, composite=True)), (ddim, dict(composite=True)),
    ]
    for sched, kw in bad:
        with pytest.raises(ValueError):
            run(_Boom(), ae, sched, noise, **kw)
    # pixel-space model: init and mask at the sampler's own resolution
    for kw in (dict(init=init), dict(init=lat, mask=mask), dict(mask=torch.ones(B, 1, L))):
        with pytest.raises(ValueError):
            run(_Boom(), None, ddim, noise, **kw)
    # the arguments that are fine get as far as the UNet
    for sched, kw in ((ddim, dict(init=init, strength=0.5, mask=mask)), (dpm, dict(init_latents=lat, mask=mask))):
        with pytest.raises(AssertionError, match="the UNet was touched"):
            run(_Boom(), ae, sched, noise, **kw)


def test_scheduler_tables_from_scheduler_objects():
    from eegldm import schedulers as S
    dpm, ddim = _fake_scheduler(S.DPMSolverMultistepScheduler, 20), _fake_scheduler(S.DDIMScheduler, 50)
    t = S.scheduler_edit_tables(dpm, 0.5)
    assert t["i0"] == 10 and t["c1"][0] == 0.0 and t["c1"][1:] == list(dpm.c1[11:]) and dpm.c1[10] != 0.0 and t["a_next"][-1] == 1.0
    t = S.scheduler_edit_tables(ddim, 0.2)
    assert t["i0"] == 40 and t["timesteps"][0] == 180 and "cx" not in t
    with pytest.raises(ValueError, match="deterministic"):
        S.scheduler_edit_tables(_fake_scheduler(S.DDPMScheduler), 0.5)


def test_abi_table_and_argument_checks_without_a_device():
    from eegldm._lib import lib, SIGNATURES
    assert lib.eegldm_abi_version() == 8
    for name in ("eegldm_edit_step", "eegldm_edit_start", "eegldm_edit_window", "eegldm_sample_edit"):
        assert name in SIGNATURES and hasattr(lib, name)
    z = C.c_void_p(0)
    nul = C.POINTER(C.c_float)()
    assert lib.eegldm_edit_step(z, z, 0.0, 0, z, z, 0.5, 0.6, 0, 0, nul, z, z, z, z, z, z, 16) != 0
    assert b"null" in lib.eegldm_last_error()
    assert lib.eegldm_edit_start(z, z, 1.0, z, 0.5, z, z, 16) != 0
    assert lib.eegldm_edit_window(z, z, 1, 64, 4, 1, z, z, z, 1, z) != 0
    one, ts = (C.c_float * 1)(0.5), (C.c_int64 * 1)(999)
    assert lib.eegldm_sample_edit(z, z, z, z, z, ts, one, one, nul, nul, nul, nul, 1, 0, 0, 1.0, z, z, 1, 64, 0, None, None, 1.0, 0) != 0
    assert b"null" in lib.eegldm_last_error()


def test_entry_script_flags():
    from eegldm.entry import edit_trials as E
    base = ["--output_dir", "o", "--diffusion_path", "d", "--input", "w.npy"]
    ldm = base + ["--best_model_path", "b", "--autoencoderkl_config_file_path", "a", "--ldm_config_file_path", "l"]
    a = E.parse_args(ldm)
    assert a.strength == 1.0 and a.mask is None and a.mask_span is None and not a.no_composite and not a.pixel and a.sampler == "ddim" and a.seed == 0
    b = E.parse_args(ldm + ["--strength", "0.4", "--mask_span", "100:300", "--mask_span", "900:1000", "--no_composite", "--seed", "7",
                            "--sampler", "dpmpp_2m"])
    assert b.strength == 0.4 and b.mask_span == ["100:300", "900:1000"] and b.no_composite and b.seed == 7 and b.sampler == "dpmpp_2m"
    keep = E.build_mask(b, 2, 3072)
    assert keep.shape == (2, 1, 3072) and keep.dtype == np.float32
    assert (keep[:, 0, 100:300] == 0).all() and (keep[:, 0, 900:1000] == 0).all() and keep.sum() == 2 * (3072 - 300)
    assert E.build_mask(a, 2, 3072) is None
    for span in ("300:100", "-5:10", "0:4000", "abc", "5"):
        with pytest.raises(ValueError):
            E.build_mask(E.parse_args(ldm + [f"--mask_span={span}"]), 1, 3072)          # (= form: "-5:10" must not read as a flag)
    c = E.parse_args(base + ["--pixel", "--config_file", "c"])
    assert c.pixel
    with pytest.raises(ValueError):
        E.check_args(E.parse_args(base + ["--pixel"]))                          # the pixel-space model needs --config_file
    with pytest.raises(ValueError):
        E.check_args(E.parse_args(base))                                        # the LDM needs its three paths
    with pytest.raises(ValueError):
        E.check_args(E.parse_args(ldm + ["--strength", "0"]))
