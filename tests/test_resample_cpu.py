"""Resampled repair (RePaint), host side, no GPU: schedulers.resample_tables against an independent restatement of the walk, the jump
coefficients against float64, what stays bit-equal to the truncated tables, and the refusals (raised before anything touches a device)."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from test_dpm_solver_cpu import T, _acp
from test_edit_cpu import _Boom, _fake_scheduler

CASES = [(20, 2, 3), (20, 5, 5), (20, 1, 10), (10, 2, 3), (7, 3, 2), (5, 4, 4)]
COUNTS = {(20, 2, 3): 56, (20, 5, 5): 80, (20, 1, 10): 191, (10, 2, 3): 26}


def formula(n_run, j, r):
    return n_run + (r - 1) * j * len(range(0, n_run - j, j))


def walk(n_run, j, r):
    """RePaint's get_schedule_jump restated on levels (its `t`: the number of steps still to run, n_run at the start): the list of levels
    the walk visits, one level at a time in both directions, then read back as forwards: every move DOWN from level l is the forward of
    local step n_run - l.  -> (steps, jumped): the step of each forward, and whether the walk came UP right before it."""
    jumps = {t: r - 1 for t in range(0, n_run - j, j)}
    t, times = n_run, []
    while t >= 1:
        t -= 1
        times.append(t)
        if jumps.get(t, 0) > 0:
            jumps[t] -= 1
            for _ in range(j):
                t += 1
                times.append(t)
    # times[k] is the level (steps still to run) reached after transition k, starting from level n_run
    steps, jumped, level, came_up = [], [], n_run, False
    for nxt in times:
        if nxt < level:                     # one step down: the forward at local step n_run - level
            steps.append(n_run - level)
            jumped.append(came_up)
            came_up = False
        else:
            came_up = True                  # one level of a jump (j of them in a row make the ONE jump of the tables)
        level = nxt
    assert level == 0
    return steps, jumped


def _tables(kind, N, strength):
    """(tab, first_order, acp) of a DDIM "leading" grid or a 2M linspace grid"""
    from eegldm.schedulers import edit_tables, multistep_coefficients, multistep_timesteps
    acp = _acp()
    if kind == "ddim":
        ts = multistep_timesteps(T, N, "leading")
        return edit_tables(acp, ts, strength, 1.0, ddim_ratio=T // N), None
    ts = multistep_timesteps(T, N, "linspace")
    cx, c0, c1 = multistep_coefficients(acp, ts, 1.0, 2, True)
    tab = edit_tables(acp, ts, strength, 1.0, multistep=dict(cx=cx, c0=c0, c1=c1, lower_order_final=True))
    fx, f0, _ = multistep_coefficients(acp, ts, 1.0, 1, True)
    return tab, (list(fx[tab["i0"]:]), list(f0[tab["i0"]:]))


@pytest.mark.parametrize("n_run,j,r", CASES)
def test_step_sequence_and_forward_count(n_run, j, r):
    from eegldm.schedulers import resample_forwards, resample_tables
    tab, first = _tables("2m", n_run, 1.0)
    rt = resample_tables(tab, first, r, j)
    steps, jumped = walk(n_run, j, r)
    assert rt["step"] == steps
    assert [v != 0.0 for v in rt["jump_n"]] == jumped and [v != 0.0 for v in rt["jump_x"]] == jumped
    assert len(steps) == formula(n_run, j, r) == resample_forwards(n_run, r, j)
    if (n_run, j, r) in COUNTS:
        assert len(steps) == COUNTS[n_run, j, r]
    assert not jumped[0] and rt["jump_n"][0] == 0.0 and rt["jump_x"][0] == 0.0
    # every level's jump lands j steps back, r - 1 times per jump point
    ups = [(steps[i - 1] + 1, steps[i]) for i in range(len(steps)) if jumped[i]]
    assert all(a - b == j for a, b in ups) and len(ups) == (r - 1) * len(range(0, n_run - j, j))
    for k in rt:
        if isinstance(rt[k], list):
            assert len(rt[k]) == len(steps), k


@pytest.mark.parametrize("kind,N", [("ddim", 10), ("ddim", 20), ("2m", 12), ("2m", 20)])
@pytest.mark.parametrize("strength", [0.5, 1.0])
@pytest.mark.parametrize("j,r", [(2, 3), (3, 2), (1, 3)])
def test_coefficients_and_what_stays_bit_equal(kind, N, strength, j, r):
    from eegldm.schedulers import resample_tables
    tab, first = _tables(kind, N, strength)
    rt = resample_tables(tab, first, r, j)
    steps = rt["step"]
    assert rt["i0"] == tab["i0"] and len(steps) == formula(len(tab["timesteps"]), j, r)
    for i, s in enumerate(steps):
        jumped = rt["jump_n"][i] != 0.0
        for k in ("timesteps", "a_t", "a_next") + (("a_prev",) if kind == "ddim" else ()):
            assert rt[k][i] == tab[k][s], k
        if not jumped:
            assert rt["jump_x"][i] == 0.0
            if i > 0:
                assert rt["a_t"][i] == rt["a_next"][i - 1]          # a step continues from the level the one before landed on
            if kind == "2m":
                assert (rt["cx"][i], rt["c0"][i], rt["c1"][i]) == (tab["cx"][s], tab["c0"][s], tab["c1"][s])      # the same Python floats
            continue
        # the jump, against float64: rho = a_t / a_landed
        rho = np.float64(tab["a_t"][s]) / np.float64(rt["a_next"][i - 1])
        assert 0.0 < rho < 1.0
        for got, want in ((rt["jump_x"][i], math.sqrt(rho)), (rt["jump_n"][i], math.sqrt(1.0 - rho))):
            w32 = np.float32(want)
            assert float(np.float32(got)) == got, "not rounded to float32"
            assert abs(got - float(w32)) <= float(np.spacing(w32))
        # x^2 + n^2 == 1 to float32 rounding: each square carries 2 u relative (the rounded factor twice), both are <= 1
        assert abs(rt["jump_x"][i] ** 2 + rt["jump_n"][i] ** 2 - 1.0) <= 4 * 2.0 ** -24
        if kind == "2m":
            assert rt["c1"][i] == 0.0 and rt["cx"][i] == first[0][s] and rt["c0"][i] == first[1][s]
    assert any(v != 0.0 for v in rt["jump_n"])


@pytest.mark.parametrize("kind", ["ddim", "2m"])
def test_resamples_one_returns_the_tables(kind):
    from eegldm.schedulers import resample_tables
    tab, first = _tables(kind, 12, 0.5)
    for j in (1, 5, 100):                   # (no jump is taken: any jump_length >= 1 will do)
        rt = resample_tables(tab, first, 1, j)
        n = len(tab["timesteps"])
        for k, v in tab.items():
            assert rt[k] == v and (not isinstance(v, list) or rt[k] is v), k
        assert rt["step"] == list(range(n)) and rt["jump_x"] == [0.0] * n and rt["jump_n"] == [0.0] * n
    assert resample_tables(tab, None, 1, 1)["step"] == list(range(len(tab["timesteps"])))


def test_table_refusals():
    from eegldm.schedulers import resample_forwards, resample_tables
    tab, first = _tables("2m", 12, 0.5)         # n_run = 6
    for r, j in ((0, 1), (-1, 1), (2, 0), (2, -3), (1, 0), (2, 6), (2, 7), (5, 100)):
        with pytest.raises(ValueError):
            resample_tables(tab, first, r, j)
    assert len(resample_tables(tab, first, 2, 5)["step"]) == 6 + 5          # jump_length = n_run - 1 still has room for one jump point
    with pytest.raises(ValueError):
        resample_tables(tab, None, 2, 1)                                    # the multistep form needs its first-order coefficients
    with pytest.raises(ValueError):
        resample_forwards(6, 2, 6)
    assert resample_forwards(20, 3, 2) == 56


@pytest.mark.parametrize("fn", ["sample", "ddim_sample_hostloop", "sample_long", "sample_long_hostloop"])
def test_refusals_come_before_any_device_work(fn):
    from eegldm import sampling, schedulers as S
    run = getattr(sampling, fn)
    long = "long" in fn
    B, L = 2, 64
    ae = types.SimpleNamespace(down=4, in_channels=1, out_channels=1)
    noise, init, mask = torch.zeros(B, 1, L), torch.zeros(B, 1, 4 * L), torch.ones(B, 1, 4 * L)
    ddim, dpm, ddpm = (_fake_scheduler(c) for c in (S.DDIMScheduler, S.DPMSolverMultistepScheduler, S.DDPMScheduler))
    pos = (1,) if long else ()               # n_windows
    geo = dict(margin=0, ramp=0) if long else {}
    scheds = (dpm,) if long else (ddim, dpm)
    for sched in scheds:
        bad = [dict(init=init, mask=mask, resamples=0), dict(init=init, mask=mask, resamples=-2), dict(init=init, mask=mask, resamples=2, jump_length=0),
               dict(init=init, mask=mask, jump_length=0), dict(init=init, mask=mask, resamples=1.5),
               dict(init=init, mask=mask, resamples=2, jump_length=10), dict(init=init, mask=mask, resamples=2, jump_length=11),
               dict(init=init, mask=mask, strength=0.5, resamples=3, jump_length=5),                       # n_run = 5
               dict(resamples=2), dict(init=init, resamples=2), dict(init=init, strength=0.5, resamples=3, jump_length=2)]      # no init / no mask
        for kw in bad:
            with pytest.raises(ValueError):
                run(_Boom(), ae, sched, noise, *pos, **geo, **kw)
        # the arguments that are fine get as far as the UNet
        for kw in (dict(init=init, mask=mask, resamples=3, jump_length=2), dict(init=init, mask=mask, strength=0.5, resamples=2, jump_length=4),
                   dict(init=init, mask=mask, resamples=1, jump_length=50)):
            with pytest.raises((AssertionError, TypeError), match="the UNet was touched|must be a UNetModel"):
                run(_Boom(), ae, sched, noise, *pos, **geo, **kw)
    if not long:
        with pytest.raises(ValueError):                                      # the ancestral scheduler stays refused
            run(_Boom(), ae, ddpm, noise, init=init, mask=mask, resamples=2)


def test_scheduler_helper_and_key():
    from eegldm import schedulers as S
    dpm, ddim = _fake_scheduler(S.DPMSolverMultistepScheduler, 20), _fake_scheduler(S.DDIMScheduler, 10)
    tab = S.scheduler_edit_tables(dpm, 0.5)
    rt = S.scheduler_resample_tables(dpm, tab, 3, 2)
    fx, f0, _ = S.multistep_coefficients(dpm.alphas_cumprod, dpm.timesteps, 1.0, 1, True)
    assert len(rt["step"]) == formula(10, 2, 3)
    for i, s in enumerate(rt["step"]):
        if rt["jump_n"][i] != 0.0:
            assert (rt["cx"][i], rt["c0"][i], rt["c1"][i]) == (fx[10 + s], f0[10 + s], 0.0)
    rt = S.scheduler_resample_tables(ddim, S.scheduler_edit_tables(ddim, 1.0), 3, 2)
    assert len(rt["step"]) == 26 and "cx" not in rt and rt["a_prev"] == rt["a_next"]
    # the key of the jumps is a named constant apart from the small seeds callers use for their start noise
    assert isinstance(S.RESAMPLE_KEY, int) and S.RESAMPLE_KEY > 2 ** 24 and S.RESAMPLE_KEY + 2 ** 32 < 2 ** 64


def test_abi_table_and_argument_checks_without_a_device():
    from eegldm._lib import lib, SIGNATURES
    assert lib.eegldm_abi_version() == 8
    for name in ("eegldm_edit_jump", "eegldm_sample_edit_resample", "eegldm_sample_long_edit_resample"):
        assert name in SIGNATURES and hasattr(lib, name)
    z = C.c_void_p(0)
    nul = C.POINTER(C.c_float)()
    assert lib.eegldm_edit_jump(z, z, 0.5, 0.5, z, 1, 0, z, z, z, 0.5, z, z, 16) != 0
    assert b"null" in lib.eegldm_last_error()
    one, zero, ts = (C.c_float * 1)(0.5), (C.c_float * 1)(0.0), (C.c_int64 * 1)(999)
    assert lib.eegldm_sample_edit_resample(z, z, z, z, z, ts, one, one, nul, nul, nul, nul, 1, 0, 0, 1.0, zero, zero, 0, z, z, 1, 64, 0, None, None, 1.0,
                                           0) != 0
    assert lib.eegldm_sample_edit_resample(z, z, z, z, z, ts, one, one, nul, nul, nul, nul, 1, 0, 0, 1.0, zero, nul, 0, z, z, 1, 64, 0, None, None, 1.0,
                                           0) != 0
    assert lib.eegldm_sample_long_edit_resample(z, z, z, z, z, ts, one, one, one, zero, one, 1, 0, 0, 1.0, zero, zero, 0, z, z, 1, 1, 64, 0, 0, 0, None,
                                                None, 1.0, 0) != 0


def test_entry_script_flags():
    from eegldm.entry import edit_long as EL, edit_trials as ET
    base = ["--output_dir", "o", "--diffusion_path", "d", "--input", "w.npy", "--best_model_path", "b", "--autoencoderkl_config_file_path", "a",
            "--ldm_config_file_path", "l"]
    a = ET.parse_args(base)
    assert a.resamples == 1 and a.jump_length == 1
    b = ET.parse_args(base + ["--resamples", "3", "--jump_length", "2"])
    assert b.resamples == 3 and b.jump_length == 2
    with pytest.raises(ValueError):
        ET.check_args(ET.parse_args(base + ["--resamples", "0"]))
    with pytest.raises(ValueError):
        ET.check_args(ET.parse_args(base + ["--resamples", "3"]))            # resampling needs a mask
    c = EL.parse_args(base)
    assert c.resamples == 1 and c.jump_length == 1
