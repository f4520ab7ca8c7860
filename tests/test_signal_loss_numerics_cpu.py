"""CPU: the float64 references and bounds of tests/signal_loss_reference.py against fp32 models of the kernels' arithmetic -- every case of
tests/test_gpu_signal_loss_rounding.py must pass its bound with the model, and each planted defect must fail on the smallest case that can
show it.  The spectral models also settle, before a GPU is involved, what the repair of spectral_kernel is measured by: the kernel as it
was (recon + i target in one packed transform, gate on the combined power) misses check B of the GPU test -- a gradient error within 4 x
that of a plain fp32 evaluation with one transform per window -- on the recon << target cases, by factors of 50 to 10^6."""
import numpy as np
import pytest
import torch

import signal_loss_reference as S

f32 = np.float32


# ---------------------------------------------------------------------------------------------------- spectral loss
def _spectral_judge(L, name, variant="decoupled", defect=None, acc_seed=None):
    """-> (worst loss ratio, worst gradient ratio, model rel-L2, yardstick rel-L2, reference)"""
    recon, target = S.spectral_cases(L)[name]
    acc = None if acc_seed is None else np.random.default_rng(acc_seed).standard_normal(recon.shape).astype(f32)
    gw = 2.5
    ref = S.spectral_reference(recon, target, acc, gw)
    loss, out = S.spectral_model(recon, target, acc, gw, variant, defect)
    _ly, outy = S.spectral_model(recon, target, acc, gw, "decoupled")
    rl = S.worst_ratio(loss, ref["loss"], ref["e_loss"])
    rg = S.worst_ratio(out, ref["out"], ref["e_out"])
    den = ref["gnorm"] if ref["gnorm"] > 0 else 1.0
    return rl, rg, S.l2_err(out, ref["out"]) / den, S.l2_err(outy, ref["out"]) / den, ref


@pytest.mark.parametrize("L", sorted(S.FFT_SPLIT))
def test_spectral_model_within_bound_and_inputs_clear_of_the_gate(L):
    for name in S.spectral_cases(L):
        rl, rg, em, ey, ref = _spectral_judge(L, name, acc_seed=5 if name == "matched" else None)
        S.report(f"cpu spectral L={L} {name}", 3 * L, max(rl, rg), f" relL2 model {em:.2e} yardstick {ey:.2e}")
        assert ref["margin"] >= S.GATE_MARGIN, (name, ref["margin"])
        assert bool(ref["open"].all()) == (name in S.SPECTRAL_UNGATED), name
        assert rl <= 1 and rg <= 1, (name, rl, rg)
        if name == "bandlimited":
            out = S.spectral_model(*S.spectral_cases(L)[name], None, 2.5)[1]
            assert not out[1].any() and not ref["out"][1].any()


@pytest.mark.parametrize("L", sorted(S.FFT_SPLIT))
@pytest.mark.parametrize("name", ["small_1e-02", "small_1e-03", "small_1e-05"])
def test_unscaled_packing_and_combined_gate_fail(L, name):
    """the kernel before the repair: its error follows the target's scale.  Check B catches it from 1e-2 on; at 1e-5 the combined gate
    closes every bin and check A fails as well."""
    rl, rg, em, ey, _ref = _spectral_judge(L, name, variant="packed")
    S.report(f"cpu spectral L={L} {name} (unscaled packing)", 3 * L, max(rl, rg), f" relL2 model {em:.2e} yardstick {ey:.2e}")
    assert em > 4 * ey, (em, ey)
    if name == "small_1e-05":
        assert rg > 1 and em > 0.5


@pytest.mark.parametrize("defect,name,variant", [("sign", "matched", "decoupled"), ("twiddle", "matched", "decoupled"),
                                                 ("noscale", "matched", "decoupled"), ("overwrite", "matched", "decoupled"),
                                                 ("herm0", "offset", "packed")])
def test_spectral_defects_fail(defect, name, variant):
    """herm0 is planted in the packed arithmetic, the only one with a Hermitian separation, on the matched-scale case with an offset, where
    that arithmetic is sound without the defect (the repaired kernel transforms each window alone and has no partner index to get wrong)"""
    L = 96
    rl, rg, em, ey, _ref = _spectral_judge(L, name, variant=variant, defect=defect, acc_seed=5)
    assert rg > 1 or em > 4 * ey, (defect, rl, rg, em, ey)          # check A or check B of the GPU test
    assert em > 100 * ey, (defect, em, ey)
    rl0, rg0, em0, ey0, _r = _spectral_judge(L, name, variant=variant, acc_seed=5)
    assert rl0 <= 1 and rg0 <= 1 and em0 <= 4 * ey0


# ---------------------------------------------------------------------------------------------------- L1, LSGAN
def _l1_judge(n, defect=None, acc=True):
    a, b, _x = S.loss_case(n)
    da0 = np.random.default_rng(n).standard_normal(n).astype(f32) if acc else None
    loss, e_loss, out, e_out = S.l1_reference(a, b, da0, 0.7)
    lm, om = S.l1_model(a, b, da0, 0.7, defect)
    return S.worst_ratio(lm, loss, e_loss), S.worst_ratio(om, out, e_out)


def _lsgan_judge(n, real, defect=None):
    _a, _b, x = S.loss_case(n)
    loss, e_loss, dl, e_dl = S.lsgan_reference(x, real, 1.3)
    lm, dm = S.lsgan_model(x, real, 1.3, defect)
    return S.worst_ratio(lm, loss, e_loss), S.worst_ratio(dm, dl, e_dl)


@pytest.mark.parametrize("n", S.LOSS_N)
def test_l1_lsgan_models_within_bound(n):
    for acc in (True, False):
        rl, rg = _l1_judge(n, acc=acc)
        assert rl <= 1 and rg <= 1, (n, acc, rl, rg)
    for real in (True, False):
        rl, rg = _lsgan_judge(n, real)
        assert rl <= 1 and rg <= 1, (n, real, rl, rg)


def test_l1_lsgan_defects_fail():
    assert _l1_judge(1, "sign0")[1] > 1                      # the single element is +0 against -0
    assert _lsgan_judge(1, True, "slope0")[1] > 1            # target real: d = -1 (target fake: d = 0 hides any slope, see below)
    for n in (255, 3 * 3072 + 1):                            # 1 / (n + 1): n = 1 would show it too, the large n is where it hides
        rl, rg = _l1_judge(n, "inv_n")
        assert rl > 1 and rg > 1, (n, rl, rg)
        rl, rg = _lsgan_judge(n, True, "inv_n")
        assert rl > 1 and rg > 1, (n, rl, rg)


def test_slope0_needs_the_real_target():
    """why the GPU test runs logits of 0 against both targets: with target fake a logit of 0 has d = 0 and any slope gives 0"""
    _a, _b, x = S.loss_case(1)
    assert S.lsgan_model(x, False, 1.3, "slope0")[1][0] == S.lsgan_model(x, False, 1.3)[1][0] == 0.0


# ---------------------------------------------------------------------------------------------------- MS-SSIM
def _ssim_judge(ks, L, C, defect=None, weights=S.SSIM_WEIGHTS):
    x, y = S.ssim_case(ks, L, C)
    k = S.gaussian_1d(ks)
    val, bound = S.ms_ssim_reference(x, y, k, weights)
    got = S.ms_ssim_model(x, y, k, weights, defect=defect)
    return got, val, bound


@pytest.mark.parametrize("ks,L,C", S.SSIM_CASES)
def test_ms_ssim_reference_follows_the_definition_and_model_within_bound(ks, L, C):
    from oracle.metrics import ms_ssim_1d
    got, val, bound = _ssim_judge(ks, L, C)
    x, y = S.ssim_case(ks, L, C)
    want = ms_ssim_1d(torch.from_numpy(x), torch.from_numpy(y), kernel_size=ks).numpy()[:, 0]
    plain = [0, 1, 3, 4]                                       # (the pair offset by 10 data ranges is beyond an fp32 evaluation's reach)
    assert np.allclose(val[plain], want[plain], rtol=2e-4, atol=2e-5), (val, want)
    S.report(f"cpu ms-ssim ks={ks} L={L} C={C}", len(val), S.worst_ratio(got, val, bound))
    assert np.all(np.abs(got - val) <= bound), (got, val, bound)
    assert val[0] == 1.0 and got[0] == 1.0 and val[1] == 0.0 and bound[1] == 0.0 and got[1] == 0.0
    assert bound[2] > 10 * bound[3] and np.isfinite(bound).all()          # the bound widens with the cancellation, and stays a bound
    assert np.all(bound[[3, 4]] < 1e-3)


def test_ms_ssim_three_scales_and_refusal_rule():
    x, y = S.ssim_case(3, 48, 1)
    k = S.gaussian_1d(3)
    val, bound = S.ms_ssim_reference(x, y, k, (0.2, 0.3, 0.5))
    got = S.ms_ssim_model(x, y, k, (0.2, 0.3, 0.5))
    assert np.all(np.abs(got - val) <= bound)
    assert S.ssim_refused(300, 11, 6) and not S.ssim_refused(3000, 11, 5) and S.ssim_refused(160, 11, 5) and not S.ssim_refused(176, 11, 5)


@pytest.mark.parametrize("defect", ["odd", "ssim", "nochan", "c1c2"])
def test_ms_ssim_defects_fail(defect):
    ks, L, C = 7, 375, 2                                       # the smallest case with a dropped sample and two channels
    got, val, bound = _ssim_judge(ks, L, C, defect)
    assert abs(got[4] - val[4]) > bound[4], (defect, got, val, bound)


# ---------------------------------------------------------------------------------------------------- multitaper PSD
@pytest.mark.parametrize("L,K", S.PSD_CASES)
def test_psd_model_within_bound(L, K):
    x, tp, w, nb = S.psd_case(L, K)
    psd, bound = S.psd_reference(x, tp, w, 100.0, nb)
    got = S.psd_model(x, tp, w, 100.0, nb)
    S.report(f"cpu psd L={L} K={K}", psd.size, S.worst_ratio(got, psd, bound))
    assert np.all(np.abs(got - psd) <= bound)
    if K == 7:
        # the sinusoid under DPSS tapers: far from the line the spectrum is 1e-5 of the peak and below; the bound there is absolute,
        # 2 |S| e_S + e_S^2 with e_S a share gamma(L) of the window's sum |v|: a few 1e-6 of the peak, whatever the bin holds
        far = np.abs(np.arange(nb) - L // 5) > 40
        assert psd[2][far].max() < 1e-4 * psd[2].max() and bound[2][far].max() < 1e-5 * psd[2].max()
        assert (bound[2][far] > psd[2][far]).any()
        from oracle.metrics import psd_multitaper
        want, _f = psd_multitaper(x.astype(np.float64), 100.0, 1e9)
        assert np.allclose(psd, want, rtol=1e-5, atol=1e-9 * want.max())          # (the oracle's tapers are float64, these fp32)


@pytest.mark.parametrize("defect,L,K", [("nyq", 2, 1), ("last", 255, 3), ("mean", 2, 1), ("w", 255, 3)])
def test_psd_defects_fail(defect, L, K):
    x, tp, w, nb = S.psd_case(L, K)
    psd, bound = S.psd_reference(x, tp, w, 100.0, nb)
    got = S.psd_model(x, tp, w, 100.0, nb, defect)
    assert np.any(np.abs(got - psd) > bound), defect
