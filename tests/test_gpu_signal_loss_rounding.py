"""-m gpu: the kernels that turn windows into loss values, loss gradients and reported quality numbers -- eegldm_spectral_loss
(csrc/spectral.hip), eegldm_l1_loss and eegldm_lsgan_loss (csrc/losses.hip), eegldm_ms_ssim_1d and eegldm_psd_multitaper (csrc/metrics.hip)
-- called through the C ABI and held to the float64 references and derived bounds of tests/signal_loss_reference.py (the derivations and the
chain lengths are in that module's docstrings; tests/test_signal_loss_numerics_cpu.py shows on the CPU that fp32 models of the kernels pass
these bounds on these very cases and that planted defects do not).  Every kernel here is one workgroup per window (the two element-wise
losses: a grid-stride loop), so B = 3 windows are enough.

Check A: the hard bound, on the loss and on every gradient / output element.
Check B (spectral gradient): the rel-L2 error against float64 is at most 4 x that of the CPU yardstick -- the same four-step transform in
numpy float32, one transform per window, same chain lengths, sums in another order (the margin tests/test_gpu_usleep_train.py::
test_adam_follows_golden_losses uses for that situation).  It is check B that is sharp where recon << target: the hard bound is a worst
case over every rounding and lies a factor 10^3 above what either evaluation does.  The case `identical` has a reference gradient of
exactly 0 and a yardstick error of exactly 0 (both spectra come out of the same arithmetic), so check A alone judges it.
Condition on the inputs, asserted: every bin's float64 A_k^2 is a factor 16 away from the gate threshold (above it in every case but
`bandlimited`), so no comparison depends on which side of the gate a rounding falls.

Each case prints one [numerics] line: case, element count, worst error in units of its bound, and for check B the two rel-L2 values
(profiles/signal_loss_numerics.txt is one run's output)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import signal_loss_reference as S  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
GW = 2.5


def _lib():
    import eegldm
    from eegldm._lib import lib, check, ptr
    return lib, check, ptr, eegldm.default_context(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- spectral loss
spectral_cases = functools.lru_cache(maxsize=None)(S.spectral_cases)


@functools.lru_cache(maxsize=None)
def spectral_ref(L, name):
    recon, target = spectral_cases(L)[name]
    return S.spectral_reference(recon, target, None, GW)


def run_spectral(recon, target, acc=None, gw=GW, grad=True):
    """-> (loss as float64, gradient buffer (B, L) fp32 or None)"""
    lib, check, ptr, ctx = _lib()
    B, L = recon.shape
    rd, td = dev(recon), dev(target)
    loss = torch.full((1,), 123.0, device=DEV)                 # (the entry point zeroes it)
    d = (dev(acc) if acc is not None else torch.zeros(B, L, device=DEV)) if grad else None
    check(lib.eegldm_spectral_loss(ctx.h, ptr(rd), ptr(td), ptr(loss), ptr(d), B, 1, L, gw))
    return float(loss.cpu().double()[0]), (d.cpu().numpy() if grad else None)


def judge_spectral(tag, recon, target, ref, loss, out, check_b):
    rl, rg = S.worst_ratio(loss, ref["loss"], ref["e_loss"]), S.worst_ratio(out, ref["out"], ref["e_out"])
    extra = ""
    if check_b:
        acc = ref["out"] - GW * ref["grad"]
        _ly, outy = S.spectral_model(recon, target, acc.astype(f32), GW)
        e_dev, e_yard = S.l2_err(out, ref["out"]) / ref["gnorm"], S.l2_err(outy, ref["out"]) / ref["gnorm"]
        extra = f" relL2 device {e_dev:.2e} yardstick {e_yard:.2e}"
    S.report(tag, out.size, max(rl, rg), f" (loss {rl:.2e}){extra}")
    assert rl <= 1, f"{tag}: loss {loss!r} against {ref['loss']!r}, {rl:.3g} x its bound {ref['e_loss']:.3g}"
    assert rg <= 1, f"{tag}: gradient {rg:.3g} x its bound"
    if check_b:
        assert e_dev <= 4 * e_yard, f"{tag}: gradient rel-L2 error {e_dev:.3e} against float64, yardstick {e_yard:.3e}"


@pytest.mark.parametrize("name", list(S.spectral_cases(96)))
@pytest.mark.parametrize("L", sorted(S.FFT_SPLIT))
def test_spectral_cases(L, name):
    recon, target = spectral_cases(L)[name]
    ref = spectral_ref(L, name)
    assert ref["margin"] >= S.GATE_MARGIN, ref["margin"]
    assert bool(ref["open"].all()) == (name in S.SPECTRAL_UNGATED)
    loss, out = run_spectral(recon, target)
    judge_spectral(f"spectral L={L} {name}", recon, target, ref, loss, out, name in S.SPECTRAL_CHECK_B)
    if name == "bandlimited":                                  # the all-zero window: every bin gated, the gradient exactly 0
        assert not bits(out[1]).any() and not ref["open"][1].any() and ref["open"][0].sum() == ref["open"][2].sum() > 0


@pytest.mark.parametrize("L", sorted(S.FFT_SPLIT))
def test_spectral_accumulates_and_windows_are_independent(L):
    recon, target = spectral_cases(L)["small_1e-02"]
    acc = np.random.default_rng(L).standard_normal(recon.shape).astype(f32)
    ref = S.spectral_reference(recon, target, acc, GW)
    loss, out = run_spectral(recon, target, acc)
    judge_spectral(f"spectral L={L} small_1e-02 onto a preloaded accumulator", recon, target, ref, loss, out, True)
    loss0, none = run_spectral(recon, target, grad=False)     # d_recon_accum = NULL: the same loss (the B partials may add in another order)
    assert none is None and abs(loss0 - loss) <= 2 * S.U * 3 * abs(loss)
    assert S.worst_ratio(loss0, ref["loss"], ref["e_loss"]) <= 1
    perm = [2, 0, 1]                                           # permuting the windows permutes the gradients bit for bit
    _lp, outp = run_spectral(recon[perm], target[perm], acc[perm])
    assert np.array_equal(bits(outp), bits(out[perm]))


@pytest.mark.parametrize("L", sorted(S.FFT_SPLIT))
def test_spectral_deterministic_mode(L, env_switches):
    env_switches(EEGLDM_DETERMINISTIC="1")
    recon, target = spectral_cases(L)["matched"]
    ref = spectral_ref(L, "matched")
    loss, out = run_spectral(recon, target)
    judge_spectral(f"spectral L={L} matched EEGLDM_DETERMINISTIC=1", recon, target, ref, loss, out, True)
    loss2, out2 = run_spectral(recon, target)
    loss0, _none = run_spectral(recon, target, grad=False)
    assert np.array_equal(bits(out), bits(out2)) and bits(f32(loss))[()] == bits(f32(loss2))[()] == bits(f32(loss0))[()]


@pytest.mark.parametrize("L", sorted(S.FFT_SPLIT))
def test_spectral_non_finite_values_stay_in_their_window(L):
    recon, target = spectral_cases(L)["matched"]
    _loss, clean = run_spectral(recon, target)
    for which in ("recon", "target"):
        for val in (np.nan, np.inf):
            r, t = recon.copy(), target.copy()
            (r if which == "recon" else t)[1, 5] = val
            loss, out = run_spectral(r, t)
            assert np.isnan(loss), (which, val, loss)
            assert np.isnan(out[1]).all(), (which, val, int(np.isnan(out[1]).sum()))
            assert np.array_equal(bits(out[[0, 2]]), bits(clean[[0, 2]])), (which, val)


# ---------------------------------------------------------------------------------------------------- L1 and least-squares GAN
def run_l1(a, b, da0, gw):
    lib, check, ptr, ctx = _lib()
    loss = torch.full((1,), 123.0, device=DEV)
    d = dev(da0) if da0 is not None else None
    ad, bd = dev(a), dev(b)                                    # (named: a temporary's memory would be handed to the next one)
    check(lib.eegldm_l1_loss(ctx.h, ptr(ad), ptr(bd), ptr(loss), ptr(d), a.size, gw))
    return float(loss.cpu().double()[0]), (d.cpu().numpy() if d is not None else None)


def run_lsgan(x, real, gw, grad=True):
    lib, check, ptr, ctx = _lib()
    loss = torch.full((1,), 123.0, device=DEV)
    d = torch.full((x.size,), 77.0, device=DEV) if grad else None          # dlogits is written, not accumulated
    xd = dev(x)
    check(lib.eegldm_lsgan_loss(ctx.h, ptr(xd), int(real), ptr(loss), ptr(d), x.size, gw))
    return float(loss.cpu().double()[0]), (d.cpu().numpy() if grad else None)


@pytest.mark.parametrize("n", S.LOSS_N)
def test_l1_and_lsgan(n, env_switches):
    """sizes 1, one below and one above a block, and 3 x 3072 + 1; elements with a == b (+0 against -0 among them: sign(0) = 0), logits of
    exactly +0 and -0 (slope 0.05) against both targets; L1 accumulates onto a preloaded buffer or only returns the loss (da = NULL), the
    LSGAN gradient overwrites; then the same under EEGLDM_DETERMINISTIC=1, twice, bit for bit.  (eegldm_l1_loss's overwrite path is a
    switch of the fused AutoencoderKL step with no C ABI of its own; tests/test_gpu_aekl.py covers it.)"""
    a, b, x = S.loss_case(n)
    da0 = np.random.default_rng(n).standard_normal(n).astype(f32)
    for det in (False, True):
        if det:
            env_switches(EEGLDM_DETERMINISTIC="1")
        tag = " EEGLDM_DETERMINISTIC=1" if det else ""
        rl, e_l, rout, e_out = S.l1_reference(a, b, da0, 0.7)
        loss, out = run_l1(a, b, da0, 0.7)
        w = max(S.worst_ratio(loss, rl, e_l), S.worst_ratio(out, rout, e_out))
        S.report(f"l1 n={n}{tag}", n, w)
        assert w <= 1, (loss, rl, e_l)
        assert out[0] == da0[0] and (out[::5] == da0[::5]).all()              # a == b: the accumulator keeps its bits
        loss0, _none = run_l1(a, b, None, 0.7)
        assert S.worst_ratio(loss0, rl, e_l) <= 1
        runs = [(loss, out)]
        for real in (True, False):
            rl, e_l, rdl, e_dl = S.lsgan_reference(x, real, 1.3)
            loss, dl = run_lsgan(x, real, 1.3)
            w = max(S.worst_ratio(loss, rl, e_l), S.worst_ratio(dl, rdl, e_dl))
            S.report(f"lsgan n={n} target {'real' if real else 'fake'}{tag}", n, w)
            assert w <= 1, (loss, rl, e_l)
            loss0, _none = run_lsgan(x, real, 1.3, grad=False)
            assert S.worst_ratio(loss0, rl, e_l) <= 1
            runs.append((loss, dl))
        if det:
            again = [run_l1(a, b, da0, 0.7), run_lsgan(x, True, 1.3), run_lsgan(x, False, 1.3)]
            for (l1_, g1), (l2_, g2) in zip(runs, again):
                assert bits(f32(l1_))[()] == bits(f32(l2_))[()] and np.array_equal(bits(g1), bits(g2))


@pytest.mark.parametrize("n", S.LOSS_N)
def test_l1_and_lsgan_nan_stays_in_its_element(n):
    a, b, x = S.loss_case(n)
    i = n // 2
    da0 = np.zeros(n, f32)
    _l, clean = run_l1(a, b, da0, 0.7)
    a2 = a.copy(); a2[i] = np.nan
    loss, out = run_l1(a2, b, da0, 0.7)
    keep = np.arange(n) != i
    assert np.isnan(loss) and np.isnan(out[i]) and np.array_equal(bits(out[keep]), bits(clean[keep]))
    for real in (True, False):
        _l, clean = run_lsgan(x, real, 1.3)
        x2 = x.copy(); x2[i] = np.nan
        loss, dl = run_lsgan(x2, real, 1.3)
        assert np.isnan(loss) and np.isnan(dl[i]) and np.array_equal(bits(dl[keep]), bits(clean[keep]))


# ---------------------------------------------------------------------------------------------------- multi-scale SSIM
def run_ssim(x, y, kernel, weights, data_range=1.0, k1=0.01, k2=0.03, sentinel=-7.0):
    """-> (return code, out (B,) fp32)"""
    lib, _check, ptr, ctx = _lib()
    B, Cc, L = x.shape
    out = torch.full((B,), sentinel, device=DEV)
    kernel, weights = np.asarray(kernel, f32), np.asarray(weights, f32)
    xd, yd = dev(x), dev(y)
    rc = lib.eegldm_ms_ssim_1d(ctx.h, ptr(xd), ptr(yd), ptr(out), B, Cc, L, (C.c_float * len(kernel))(*kernel.tolist()), len(kernel),
                               (C.c_float * len(weights))(*weights.tolist()), len(weights), data_range, k1, k2)
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("ks,L,C_", S.SSIM_CASES)
def test_ms_ssim(ks, L, C_):
    """[0, 1] windows; 375 drops a trailing sample at two scales, 4096 fills the 8-per-thread pooling registers, 17 taps is MAX_TAPS.  Pair 0
    identical: exactly 1; pair 1 anti-correlated: exactly 0 (the bound there is 0); pair 2 offset by 10 data ranges: within a bound that
    the one-pass cancellation widens."""
    x, y = S.ssim_case(ks, L, C_)
    k = S.gaussian_1d(ks)
    val, bound = S.ms_ssim_reference(x, y, k, S.SSIM_WEIGHTS)
    rc, got = run_ssim(x, y, k, S.SSIM_WEIGHTS)
    assert rc == 0 and np.isfinite(bound).all()
    S.report(f"ms-ssim ks={ks} L={L} C={C_}", len(val), S.worst_ratio(got, val, bound), f" (offset pair {abs(got[2] - val[2]) / bound[2]:.2e})")
    assert np.all(np.abs(got.astype(np.float64) - val) <= bound), (got, val, bound)
    assert got[0] == 1.0 and got[1] == 0.0 and bound[1] == 0.0 and bound[2] > 10 * bound[3]
    rc, sym = run_ssim(y, x, k, S.SSIM_WEIGHTS)
    assert rc == 0 and np.all(np.abs(sym.astype(np.float64) - val) <= bound)


def test_ms_ssim_three_scales():
    x, y = S.ssim_case(3, 48, 1)
    k = S.gaussian_1d(3)
    w = (0.2, 0.3, 0.5)
    val, bound = S.ms_ssim_reference(x, y, k, w)
    rc, got = run_ssim(x, y, k, w)
    S.report("ms-ssim ks=3 L=48 C=1 three scales", len(val), S.worst_ratio(got, val, bound))
    assert np.isfinite(bound).all()
    assert rc == 0 and np.all(np.abs(got.astype(np.float64) - val) <= bound), (got, val, bound)


@pytest.mark.parametrize("L,ks,n_scales", [(300, 11, 6), (352, 11, 6), (80, 11, 4), (160, 11, 5), (176, 11, 5)])
def test_ms_ssim_refuses_a_scale_shorter_than_the_kernel(L, ks, n_scales):
    """The reference's guard, L / (n_scales - 1)^2 > ks - 1, lets 300 samples through for 6 scales and 11 taps: the last scale has 9 samples, a
    negative count of valid positions.  The entry point refuses whenever any scale is shorter than the kernel (and whenever the reference
    does), and leaves `out` untouched; one step further (352 -> 11 samples; 176 -> 11) it computes."""
    rng = np.random.default_rng(L)
    x = rng.uniform(0, 1, (3, 1, L)).astype(f32); y = np.clip(x + 0.03 * rng.standard_normal(x.shape), 0, 1).astype(f32)
    w = np.full(n_scales, 1.0 / n_scales, f32)
    k = S.gaussian_1d(ks)
    rc, out = run_ssim(x, y, k, w)
    if S.ssim_refused(L, ks, n_scales):
        assert (L >> (n_scales - 1)) < ks or L // max(1, n_scales - 1) ** 2 <= ks - 1
        assert rc != 0 and (out == f32(-7.0)).all(), (rc, out)
    else:
        val, bound = S.ms_ssim_reference(x, y, k, w)
        assert np.isfinite(bound).all() and np.all(bound < 1e-2), bound
        assert rc == 0 and np.all(np.abs(out.astype(np.float64) - val) <= bound), (out, val, bound)
    assert S.ssim_refused(300, 11, 6) and S.ssim_refused(80, 11, 4) and S.ssim_refused(160, 11, 5) and not S.ssim_refused(352, 11, 6)


# ---------------------------------------------------------------------------------------------------- multitaper PSD
def run_psd(x, tapers, weights, sfreq, n_bins, sentinel=-7.0):
    lib, _check, ptr, ctx = _lib()
    B, L = x.shape
    psd = torch.full((B, max(n_bins, 1)), sentinel, device=DEV)
    weights = np.asarray(weights, f32)
    xd, td = dev(x), dev(tapers)
    rc = lib.eegldm_psd_multitaper(ctx.h, ptr(xd), ptr(td), (C.c_float * len(weights))(*weights.tolist()), len(weights), sfreq,
                                   n_bins, ptr(psd), B, L)
    return rc, psd.cpu().numpy()


@pytest.mark.parametrize("L,K", S.PSD_CASES)
def test_psd_multitaper(L, K):
    """The whole one-sided spectrum: the Nyquist bin of an even L (not doubled), the last bin of an odd L (doubled).  Window 1 has a mean of
    100 sigma; window 2 is a pure sinusoid, whose bins far from the line are held by the absolute bound -- a share of the window's sum
    |v|, no relative tolerance."""
    x, tp, w, nb = S.psd_case(L, K)
    psd, bound = S.psd_reference(x, tp, w, 100.0, nb)
    rc, got = run_psd(x, tp, w, 100.0, nb)
    assert rc == 0 and got.shape == psd.shape
    ratio = [S.worst_ratio(got[b], psd[b], bound[b]) for b in range(3)]
    S.report(f"psd L={L} K={K}", psd.size, max(ratio), f" (noise {ratio[0]:.2e}, mean 100 sigma {ratio[1]:.2e}, sinusoid {ratio[2]:.2e})")
    assert np.all(np.abs(got.astype(np.float64) - psd) <= bound)


def test_psd_multitaper_refusals_leave_the_output_untouched():
    x, tp, w, nb = S.psd_case(256, 16)
    rc, got = run_psd(x, tp, w, 100.0, nb + 1)                 # n_bins > L / 2 + 1
    assert rc != 0 and (got == f32(-7.0)).all()
    tp17, w17 = np.concatenate([tp, tp[:1]]), np.concatenate([w, w[:1]])
    rc, got = run_psd(x, tp17, w17, 100.0, nb)                 # K > 16
    assert rc != 0 and (got == f32(-7.0)).all()
    x, tp, w, nb = S.psd_case(255, 3)
    rc, got = run_psd(x, tp, w, 100.0, nb + 1)                 # odd L: L / 2 + 1 = 128 bins, 129 refused
    assert rc != 0 and (got == f32(-7.0)).all()
