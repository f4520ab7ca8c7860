"""DPM-Solver++ (2M) host side, no GPU: timestep grids, the coefficient table against an independent float64 restatement, first order
== DDIM, and the solver driven over the closed-form Gaussian denoiser.  The float64 reference recursion of the solver lives here
(`reference_coefficients`, `run_solver`): it is written from the formulas, term by term, not from the table under test."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

T = 1000
GRID_N = [1, 2, 5, 14, 15, 50, 1000]


def _acp(beta_start=0.0015, beta_end=0.0205):
    """float64 view of the float32 alphas_cumprod the schedulers hold (scaled-linear betas)."""
    from eegldm.schedulers import _betas
    return torch.cumprod(1.0 - _betas("scaled_linear_beta", T, beta_start, beta_end), dim=0).double().numpy()


def reference_coefficients(acp, ts, final_acp, solver_order=2, lower_order_final=True):
    """Independent restatement in float64 numpy: lambda through log of the ratio of variances, the exponential through exp (not
    expm1) of the half-log-SNR difference.  -> float64 arrays (cx, c0, c1)."""
    N = len(ts)
    a = np.concatenate([np.asarray([acp[t] for t in ts], np.float64), [np.float64(final_acp)]])
    alpha, sigma = np.sqrt(a), np.sqrt(1.0 - a)
    cx, c0, c1 = np.zeros(N), np.zeros(N), np.zeros(N)
    for i in range(N):
        if sigma[i + 1] == 0.0:
            cx[i], k = 0.0, alpha[i + 1]
        else:
            cx[i] = sigma[i + 1] / sigma[i]
            # exp(-h) = (sigma_{i+1} / alpha_{i+1}) (alpha_i / sigma_i);  k = alpha_{i+1} (1 - exp(-h)) = alpha_{i+1} - sigma_{i+1} alpha_i / sigma_i
            k = alpha[i + 1] - sigma[i + 1] * alpha[i] / sigma[i]
        last = i == N - 1
        if solver_order == 1 or i == 0 or (last and sigma[i + 1] == 0.0) or (last and lower_order_final and N < 15):
            c0[i] = k
        else:
            lam = lambda j: 0.5 * (np.log(a[j]) - np.log1p(-a[j]))
            with np.errstate(divide="ignore"):          # h = 0 (a step onto its own grid point): r = inf, k = 0, the identity step
                r = (lam(i) - lam(i - 1)) / (lam(i + 1) - lam(i))
            c0[i], c1[i] = k + k / (2.0 * r), -k / (2.0 * r)
    return cx, c0, c1


def run_solver(cx, c0, c1, x, x0_fn, upto=None):
    """x_{i+1} = cx_i x_i + c0_i x0_i + c1_i x0_{i-1} in float64; x0_fn(i, x) is the data prediction at grid point i."""
    hist = np.zeros_like(x)
    for i in range(len(cx) if upto is None else upto):
        x0 = x0_fn(i, x)
        x = cx[i] * x + c0[i] * x0 + c1[i] * hist
        hist = x0
    return x


@pytest.mark.parametrize("spacing", ["linspace", "leading"])
@pytest.mark.parametrize("N", GRID_N)
def test_timestep_grids(spacing, N):
    from eegldm.schedulers import multistep_timesteps
    ts = multistep_timesteps(T, N, spacing)
    assert len(ts) == N and all(isinstance(t, int) for t in ts)
    assert all(a > b for a, b in zip(ts, ts[1:])), "not strictly decreasing"
    assert len(set(ts)) == N and 0 <= ts[-1] and ts[0] <= T - 1
    if spacing == "linspace":
        assert ts[0] == T - 1
        want = np.round(np.linspace(T - 1, 0, N + 1))[:-1]
        assert np.abs(np.asarray(ts) - want).max() <= (1 if N == T else 0)      # N = T: one rounding tie, the grid below it moves down by one
    else:
        assert ts == [int(v) for v in (np.arange(N) * (T // N))[::-1]]           # DDIMScheduler.set_timesteps
    with pytest.raises(ValueError):
        multistep_timesteps(T, T + 1, spacing)
    with pytest.raises(ValueError):
        multistep_timesteps(T, 0, spacing)


@pytest.mark.parametrize("spacing", ["linspace", "leading"])
@pytest.mark.parametrize("order,lof", [(1, True), (2, True), (2, False)])
@pytest.mark.parametrize("N", GRID_N)
def test_coefficient_table_vs_float64_restatement(spacing, order, lof, N):
    """Both sides are float64 evaluations rounded once to float32: they may differ by the rounding of a value that sits next to a
    float32 tie, so the bound is 1 ulp of float32 (np.spacing of the reference), not equality."""
    from eegldm.schedulers import multistep_coefficients, multistep_timesteps
    acp = _acp()
    ts = multistep_timesteps(T, N, spacing)
    for final in (1.0, float(acp[0])):
        got = multistep_coefficients(acp, ts, final, order, lof)
        want = reference_coefficients(acp, ts, final, order, lof)
        for name, g, w in zip(("cx", "c0", "c1"), got, want):
            g = np.asarray(g, np.float64); w32 = w.astype(np.float32)
            assert all(float(np.float32(v)) == v for v in g), f"{name} is not rounded to float32"
            assert (np.abs(g - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64)).all(), (name, N, np.abs(g - w).max())
        cx, c0, c1 = got
        assert c1[0] == 0.0
        if order == 1:
            assert not any(c1)
        elif N >= 3:
            assert all(v != 0.0 for v in c1[1:-1])
        if final == 1.0:
            assert cx[-1] == 0.0 and c1[-1] == 0.0 and c0[-1] == 1.0          # lands on x0
        elif order == 2 and N >= 2 and ts[-1] != 0:          # (ts[-1] == 0 with final = acp[0]: a zero-length last step, the identity)
            assert (c1[-1] == 0.0) == (lof and N < 15)


def test_bad_arguments():
    from eegldm.schedulers import multistep_coefficients
    acp = _acp()
    with pytest.raises(ValueError):
        multistep_coefficients(acp, [999, 500], 1.0, 3)
    with pytest.raises(ValueError):
        multistep_coefficients(acp, [999, 500], 0.0, 2)
    with pytest.raises(ValueError):
        multistep_coefficients(np.array([0.5, 1.0]), [1, 0], 1.0, 2)


@pytest.mark.parametrize("N", [1, 2, 5, 10, 50, 200, 1000])
def test_first_order_is_ddim(N):
    """On DDIM's grid and final alpha the first-order step is DDIM's: x_{i+1} = alpha_{i+1} x0 + sigma_{i+1} eps with
    eps = (x - alpha_i x0) / sigma_i, i.e. cx sigma_i = sigma_{i+1} and cx alpha_i + k = alpha_{i+1}.

    Bound, from the operation count on the UNROUNDED float64 coefficients (the table's float32 rounding is test 2's subject): with
    u = 2^-53, cx = sigma_{i+1} / sigma_i is one rounded division of two rounded square roots, and cx * sigma_i one more product: the
    first identity holds to 2 u relative (the sqrt errors cancel between cx and the sigmas it is checked against) -- 4 u allowed.  k
    goes through log, expm1 and a product (library functions to 1 ulp each, but lambda's ABSOLUTE error of ~2 u (|lambda| + 1), |lambda| <=
    ~5 on this schedule, passes through exp(-h) unamplified relative to exp(-h) <= 1): |dk| <= ~16 u alpha_{i+1} (1 + exp(-h)) <= 32 u;
    the sum cx alpha_i + k adds 2 roundings of numbers <= 1.  64 u absolute is allowed."""
    from eegldm.schedulers import multistep_coefficients, multistep_timesteps
    acp = _acp()
    u = 2.0 ** -53
    for final in (1.0, float(acp[0])):          # DDIMScheduler.final_alpha_cumprod: set_alpha_to_one True / False
        ts = multistep_timesteps(T, N, "leading")
        a = np.asarray([acp[t] for t in ts] + [final], np.float64)
        alpha, sigma = np.sqrt(a), np.sqrt(1.0 - a)
        cx, k, c1 = multistep_coefficients(acp, ts, final, solver_order=1, as_float32=False)
        assert not any(c1)
        for i in range(N):
            assert abs(cx[i] * sigma[i] - sigma[i + 1]) <= 4 * u * sigma[i + 1], (i, cx[i] * sigma[i] - sigma[i + 1])
            assert abs(cx[i] * alpha[i] + k[i] - alpha[i + 1]) <= 64 * u, (i, (cx[i] * alpha[i] + k[i] - alpha[i + 1]) / u)
    # and the table itself (float32) carries those values: its first-order rows against DDIM's coefficients to float32 rounding
    ts = multistep_timesteps(T, N, "leading")
    cx32, c032, c132 = multistep_coefficients(acp, ts, 1.0, solver_order=1)
    a = np.asarray([acp[t] for t in ts] + [1.0], np.float64)
    alpha, sigma = np.sqrt(a), np.sqrt(1.0 - a)
    assert not any(c132)
    assert np.abs(np.asarray(cx32) * sigma[:-1] - sigma[1:]).max() <= 2.0 ** -24
    assert np.abs(np.asarray(cx32) * alpha[:-1] + np.asarray(c032) - alpha[1:]).max() <= 2 * 2.0 ** -24


def _gaussian_errors(s, N, state_dtype=np.float64):
    """(first-order error, second-order error) of the table driven over the optimal denoiser of N(0, s^2) data on the linspace grid, at
    the last grid point before the final step, relative to max |exact|."""
    from eegldm.schedulers import multistep_coefficients, multistep_timesteps
    acp = _acp()
    ts = multistep_timesteps(T, N, "linspace")
    a = np.asarray([acp[t] for t in ts], np.float64)
    xT = np.random.default_rng(5).standard_normal(512) * math.sqrt(a[0] * s * s + 1.0 - a[0])

    def x0_fn(i, x):      # eps = sigma x / (acp s^2 + 1 - acp);  x0 = (x - sigma eps) / alpha
        eps = math.sqrt(1.0 - a[i]) * x / (a[i] * s * s + 1.0 - a[i])
        return (x - math.sqrt(1.0 - a[i]) * eps) / math.sqrt(a[i])

    exact = xT * math.sqrt((a[-1] * s * s + 1.0 - a[-1]) / (a[0] * s * s + 1.0 - a[0]))
    errs = []
    for order in (1, 2):
        cx, c0, c1 = (np.asarray(v, state_dtype) for v in multistep_coefficients(acp, ts, 1.0, order))
        x = run_solver(cx, c0, c1, xT.astype(state_dtype), x0_fn, upto=N - 1)
        errs.append(float(np.abs(x - exact).max() / np.abs(exact).max()))
    return errs


@pytest.mark.parametrize("s", [1.0, 2.0])
@pytest.mark.parametrize("N", [10, 20, 40])
def test_gaussian_closed_form_second_order_beats_first(s, N):
    """The probability-flow ODE of N(0, s^2) data has the exact solution x_t = x_T sqrt((acp_t s^2 + 1 - acp_t) / (acp_T s^2 + 1 - acp_T)).
    Second order must be at least five times closer to it than first order on the same grid (measured ratios: 9.7-13.8 at s = 1,
    24-40 at s = 2).  s = 0.5 is not asserted: the ratio there is not monotone in N."""
    e1, e2 = _gaussian_errors(s, N)
    print(f"s={s} N={N}: first order {e1:.3e}, second order {e2:.3e}, ratio {e1 / e2:.1f}")
    assert e2 <= e1 / 5.0, (e1, e2)
    f1, f2 = _gaussian_errors(s, N, np.float32)          # the state carried in float32, as on the device
    # per step: three products and two sums in float32, |cx| + |c0| + |c1| <= ~3 on this grid -> 16 x 2^-24 of max |x| a step
    assert abs(f2 - e2) <= 16 * N * 2.0 ** -24 and abs(f1 - e1) <= 16 * N * 2.0 ** -24


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("N", [1, 10, 20])
def test_final_step_lands_on_x0(order, N):
    from eegldm.schedulers import multistep_coefficients, multistep_timesteps
    acp = _acp()
    ts = multistep_timesteps(T, N, "linspace")
    cx, c0, c1 = multistep_coefficients(acp, ts, 1.0, order)
    seen = []

    def x0_fn(i, x):
        seen.append(np.tanh(x) + 0.1 * i)
        return seen[-1]
    out = run_solver(np.asarray(cx), np.asarray(c0), np.asarray(c1), np.random.default_rng(6).standard_normal(64), x0_fn)
    assert np.array_equal(out, seen[-1])


def test_entry_points_reject_bad_arguments_without_a_device():
    """Argument checks run before anything touches the GPU: a NULL context / buffer, step 0 with c1 != 0."""
    from eegldm._lib import lib, SIGNATURES
    assert lib.eegldm_abi_version() == 8
    assert "eegldm_multistep_step" in SIGNATURES and "eegldm_sample_multistep" in SIGNATURES
    z = C.c_void_p(0)
    assert lib.eegldm_multistep_step(z, z, 0.0, 0, z, z, 0.5, 0, 0, 1.0, 1.0, 0.0, z, z, z, 16) != 0
    one = (C.c_float * 1)(0.5)
    ts = (C.c_int64 * 1)(999)
    assert lib.eegldm_sample_multistep(z, z, z, ts, one, one, one, one, 1, 0, 0, 1.0, z, z, 1, 64, 0, None, None, 1.0, 0) != 0
    assert b"null" in lib.eegldm_last_error()


def test_entry_scripts_take_the_sampler_flags_and_default_to_ddim():
    from eegldm.entry import sample_trials as ST, sample_trials_dm as SD
    a = ST.parse_args(["--output_dir", "o", "--best_model_path", "b", "--diffusion_path", "d", "--autoencoderkl_config_file_path", "a",
                       "--ldm_config_file_path", "l"])
    assert a.sampler == "ddim" and a.solver_order == 2
    b = SD.parse_args(["--output_dir", "o", "--config_file", "c", "--diffusion_path", "d", "--sampler", "dpmpp_2m", "--solver_order", "1"])
    assert b.sampler == "dpmpp_2m" and b.solver_order == 1
    with pytest.raises(SystemExit):
        SD.parse_args(["--output_dir", "o", "--config_file", "c", "--diffusion_path", "d", "--sampler", "euler"])
    from eegldm import sampling
    assert sampling.sample is sampling.ddim_sample
