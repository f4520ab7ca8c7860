"""CPU: the checks of tests/usleep_reference.py are sharp at the shapes tests/test_gpu_usleep_fwd.py runs on the U-Sleep forward kernels
(csrc/usleep.hip, csrc/usleep_train.hip).  On six of the sweep's cases the bound functions accept the float64 reference rounded once to fp32
and a plain torch-fp32 evaluation of the layer, in all three modes; and they reject what a subtly wrong kernel would store -- sixteen defect
models built here from the reference, never in a kernel."""
import pytest
import torch
import torch.nn.functional as F

import usleep_reference as R

CASES = {
    "preskip": ("ups", dict(rows=65, Cout=17, Cin=33, K=2), 11),           # nearest x2 at odd L through the K = 2 conv, no zero on the left
    "skip_even": ("ups_skip", dict(rows=130, Cout=17, Cin=33, K=7), 12),   # Lb = L + 1: the skip is the cropped one
    "skip_odd": ("ups_skip", dict(rows=65, Cout=17, Cin=33, K=7), 13),     # row tile ending inside a sample, Cout = 16 + 1, Cin = 32 + 1
    "plain": ("plain", dict(rows=65, Cout=17, Cin=33, K=7), 14),
    "generic_k": ("plain", dict(rows=64, Cout=16, Cin=32, K=13), 15),
    "one": ("plain", dict(rows=63, Cout=1, Cin=1, K=1), 16),
}


def case(name):
    form, sw, seed = CASES[name]
    return R.layer_case(form, seed=seed, **sw)


def f32(t):
    return t.float()


def ideal_out(c, mode, z=None, pooled=True):
    """The float64 reference rounded once to fp32 at every stored quantity (z, then everything else from the stored z)."""
    if z is None:
        _s, z, _d = R.conv_elu_ref(c)
    z = f32(z)
    if mode == 0:
        y, _ = R.bn_eval_ref(z.double(), 0.0, c["gamma"], c["beta"], c["rm"], c["rv"])
        out = dict(y=f32(y), rm=c["rm"].clone(), rv=c["rv"].clone(), nbt=c["nbt"].clone())
    else:
        r = R.bn_train_ref(z, c["gamma"], c["beta"], c["rm"], c["rv"], c["nbt"], mode)
        out = dict(z=z, y=f32(r["y"][0]), rm=f32(r["rm"][0]), rv=f32(r["rv"][0]), nbt=f32(r["nbt"][0]))
        if mode == 2:
            out["stat"] = torch.cat([f32(r["mean"][0]), f32(r["rstd"][0])])
    if pooled:
        out["pooled"] = R.maxpool_fwd_ref(out["y"])
    return out


def torch32_out(c, mode):
    """conv -> ELU -> BatchNorm -> pad + MaxPool as torch evaluates them in fp32."""
    v = R.virtual_input(c["a"], c["b2"], c["ups"], c["L"])
    z = F.elu(R.conv_same(v, c["w"], c["bias"], c["left"]))
    rm, rv = c["rm"].clone(), c["rv"].clone()
    y = F.batch_norm(z, rm, rv, c["gamma"], c["beta"], training=mode != 0, momentum=0.1, eps=1e-5)
    out = dict(y=y, rm=rm, rv=rv, nbt=c["nbt"] + (1.0 if mode else 0.0), pooled=R.maxpool_fwd_ref(y))
    if mode:
        out["z"] = z
    return out


def rejected(name, c, mode, out, match="bound|exact"):
    with pytest.raises(AssertionError, match=match):
        R.judge_layer(name, c, mode, out)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reference_and_torch_fp32_are_accepted(name, mode):
    c = case(name)
    wi = R.judge_layer(f"{name} RNE(ref)", c, mode, ideal_out(c, mode))
    wt = R.judge_layer(f"{name} torch fp32", c, mode, torch32_out(c, mode))
    print(f"[numerics] model {name} mode {mode}: worst error / bound, RNE(ref) {max(v for k, v in wi.items() if k != 'expm1 ulps'):.3f}, "
          f"torch fp32 {max(v for k, v in wt.items() if k != 'expm1 ulps'):.3f}")
    assert max(v for k, v in wi.items() if k != "expm1 ulps") <= 0.5          # one rounding of each stored quantity is far inside


def z_defect(c, build):
    """Outputs of every mode from a wrong ELU output `build(c) -> z (float64)`: the stored z is the wrong one, everything after it is right."""
    z = build(c)
    for mode in (0, 1, 2):
        rejected("defect", c, mode, ideal_out(c, mode, z=z))


def _conv(c, v=None, w=None, bias=None, left=None):
    v = R.virtual_input(R.f64(c["a"]), R.f64(c["b2"]), c["ups"], c["L"]) if v is None else v
    return R.conv_same(v, R.f64(c["w"]) if w is None else w, R.f64(c["bias"]) if bias is None else bias, c["left"] if left is None else left)


def test_k2_zero_pad_on_the_left():
    c = case("preskip")
    assert c["K"] == 2 and c["left"] == 0
    z_defect(c, lambda c: R.elu64(_conv(c, left=1)))


def test_nearest_x2_read_at_p_plus_1_halved():
    c = case("preskip")

    def build(c):
        a = R.f64(c["a"])
        idx = ((torch.arange(c["L"]) + 1) >> 1).clamp_max(c["La"] - 1)
        return R.elu64(_conv(c, v=a[..., idx]))
    z_defect(c, build)


def test_skip_read_with_the_cropped_stride():
    c = case("skip_even")
    assert c["Lb"] == c["L"] + 1

    def build(c):
        B, Cb, L = c["B"], c["Cb"], c["L"]
        flat = R.f64(c["b2"]).reshape(-1)
        skip = flat[:B * Cb * L].reshape(B, Cb, L)              # row (b, ci) starts at (b Cb + ci) L instead of (b Cb + ci) Lb
        up = R.virtual_input(R.f64(c["a"]), None, 1, L)
        return R.elu64(_conv(c, v=torch.cat([up, skip], 1)))
    z_defect(c, build)


def test_input_channel_32_dropped_at_cin_33():
    c = case("skip_odd")

    def build(c):
        w = R.f64(c["w"]).clone(); w[:, 32] = 0
        return R.elu64(_conv(c, w=w))
    z_defect(c, build)


def test_bias_omitted_for_channel_16_at_cout_17():
    for name in ("skip_odd", "plain"):
        c = case(name)

        def build(c):
            b = R.f64(c["bias"]).clone(); b[16] = 0
            return R.elu64(_conv(c, bias=b))
        z_defect(c, build)


def test_row_64_of_65_computed_with_row_63s_position():
    c = case("plain")
    assert (c["B"], c["L"]) == (5, 13)

    def build(c):
        z = R.conv_elu_ref(c)[1].clone()
        z[4, :, 12] = z[4, :, 11]                                # row 64 = (b 4, l 12), row 63 = (4, 11)
        return z
    z_defect(c, build)


def test_elu_before_the_bias():
    c = case("plain")
    z_defect(c, lambda c: R.elu64(_conv(c, bias=torch.zeros(c["Cout"], dtype=torch.float64))) + R.f64(c["bias"]).reshape(1, -1, 1))


@pytest.mark.parametrize("mode", [1, 2])
def test_batch_statistics_defects(mode):
    c = case("plain")
    good = ideal_out(c, mode)
    R.judge_layer("good", c, mode, good)
    z = good["z"].double()
    n = z.shape[0] * z.shape[2]
    mean, var = z.mean((0, 2)), z.var((0, 2), unbiased=False)
    bc = lambda t: t.reshape(1, -1, 1)
    g, be, rm, rv = (R.f64(c[k]) for k in ("gamma", "beta", "rm", "rv"))
    # normalisation by the unbiased variance
    y = (z - bc(mean)) / torch.sqrt(bc(var * n / (n - 1)) + R.EPS) * bc(g) + bc(be)
    bad = dict(good, y=f32(y)); bad["pooled"] = R.maxpool_fwd_ref(bad["y"])
    if mode == 2:
        bad["stat"] = None
    rejected("unbiased normalisation", c, mode, bad, match="bound .* y")
    # running variance from the biased one
    rejected("biased running variance", c, mode, dict(good, rv=f32(R.KEEP * rv + R.MOM * var)), match="bound .* rv")
    # momentum weights swapped
    rejected("swapped momentum", c, mode, dict(good, rm=f32(R.MOM * rm + R.KEEP * mean)), match="bound .* rm")
    rejected("swapped momentum", c, mode, dict(good, rv=f32(R.MOM * rv + R.KEEP * var * n / (n - 1))), match="bound .* rv")
    # the counter
    rejected("counter", c, mode, dict(good, nbt=c["nbt"].clone()), match="bound .* nbt")


def test_eps_outside_the_square_root_in_the_eval_fold():
    for name in ("plain", "skip_odd"):
        c = case(name)
        _s, z, _d = R.conv_elu_ref(c)
        g, be, rm, rv = (R.f64(c[k]).reshape(1, -1, 1) for k in ("gamma", "beta", "rm", "rv"))
        y = (z - rm) / (torch.sqrt(rv) + R.EPS) * g + be
        out = dict(ideal_out(c, 0), y=f32(y)); out["pooled"] = R.maxpool_fwd_ref(out["y"])
        rejected("eps outside", c, 0, out, match="bound .* y")


def pool_rows(L):
    """The rows of the GPU MaxPool test: a coarse grid with ties, all-negative rows (the pad zero wins at the ends of an odd row), constant rows."""
    x = torch.round(R.rnd((12, L), 40 + L) * 2.0) / 2.0
    x[0] = -x[0].abs() - 0.5; x[1] = -1.0; x[2] = 0.0; x[3] = 1.0
    return x


def plant_nonfinite(x):
    """NaN at the first / last / both positions of a pair, at both ends of the row, and +-inf."""
    x = x.clone(); L = x.shape[-1]; odd = L % 2
    nan, inf = float("nan"), float("inf")
    x[4, 0] = nan; x[5, L - 1] = nan; x[6, 0] = inf; x[7, L - 1] = -inf; x[8, 0] = -inf; x[8, L - 1] = inf
    if L >= 3:
        p0 = 2 - odd                                             # an inner pair: positions p0, p0 + 1
        x[9, p0] = nan; x[10, p0 + 1] = nan; x[11, p0] = nan; x[11, p0 + 1] = nan
        x[4, p0 + 1] = inf; x[5, p0] = -inf
    return x


@pytest.mark.parametrize("L", [1, 2, 3, 47])
def test_maxpool_defects(L):
    odd = L % 2
    x = pool_rows(L)
    R.check_pool("good", R.maxpool_fwd_ref(x), x)
    if odd:
        # pad on one side only: MaxPool1d(2) of the odd padded length L + 2 never reaches the right zero, so it is the LEFT one that counts;
        # with the zero on the right alone every pair is shifted by one
        # (at L = 1 the single pair holds x[0] and one zero either way)
        right_only = F.max_pool1d(F.pad(x, (0, 1)).unsqueeze(0), 2, 2)[0]
        if L > 1:
            with pytest.raises(AssertionError, match="exact pooled stage"):
                R.check_pool("pad on the right only", right_only, x)
        # the pad zero not taking part in the max: -inf padding
        neg = F.max_pool1d(F.pad(x, (1, 1), value=float("-inf")).unsqueeze(0), 2, 2)[0]
        with pytest.raises(AssertionError, match="exact pooled stage"):
            R.check_pool("pad not in the max", neg, x)
    # NaN dropped by the max (fmaxf)
    xn = plant_nonfinite(x)
    want = R.maxpool_fwd_ref(xn)
    assert bool(torch.isnan(want).any()) and not bool(torch.isnan(want).all())
    R.check_pool("good, non-finite", want, xn)
    p = F.pad(xn, (1, 1)) if odd else xn
    p = p[:, :2 * want.shape[-1]]                               # (the right zero of an odd row belongs to no pair)
    dropped = torch.fmax(p[:, 0::2], p[:, 1::2])
    with pytest.raises(AssertionError, match="exact pooled stage .* NaN positions differ"):
        R.check_pool("NaN dropped", dropped, xn)


def clf_case(C1, ncls, S, win, tail, seed=70):
    L = S * win + tail
    x = R.rnd((3, C1, L), seed)
    P = [R.rnd((C1, C1), seed + 1, 0.5), R.rnd((C1,), seed + 2, 0.1), R.rnd((ncls, C1), seed + 3, 0.5), R.rnd((ncls,), seed + 4, 0.1),
         R.rnd((ncls, ncls), seed + 5, 0.5), R.rnd((ncls,), seed + 6, 0.1)]
    return x, P, L


def clf_with_mean(x, P, mean_fn, dtype=torch.float64):
    w0, b0, w3, b3, w5, b5 = (p.to(dtype) for p in P)
    lin = lambda w, b, v: F.conv1d(v, w[:, :, None], b)
    m = mean_fn(torch.tanh(lin(w0, b0, x.to(dtype))))
    return lin(w5, b5, F.elu(lin(w3, b3, m)))


@pytest.mark.parametrize("S", [1, 2])
def test_classifier_accepts_and_rejects(S):
    win, tail = 37, 5
    x, P, L = clf_case(6, 5, S, win, tail)
    y, d = R.clf_fwd_ref(x, P, win)
    R.check_bound("clf RNE(ref)", f32(y), y, d)
    w32 = R.check_bound("clf torch fp32", clf_with_mean(x, P, lambda t: F.avg_pool1d(t, win), torch.float32), y, d)
    print(f"[numerics] model clf S={S}: torch fp32 worst error / bound {w32:.3f}")
    # the mean taken over L instead of S * win (each window's sum divided by L / S)
    over_l = clf_with_mean(x, P, lambda t: F.avg_pool1d(t, win) * (win * S / L))
    with pytest.raises(AssertionError, match="bound"):
        R.check_bound("mean over L", f32(over_l), y, d)
    # the tail included in the mean of the last window
    def with_tail(t):
        m = F.avg_pool1d(t, win).clone()
        m[..., -1] = t[..., (S - 1) * win:].mean(-1)
        return m
    with pytest.raises(AssertionError, match="bound"):
        R.check_bound("tail included", f32(clf_with_mean(x, P, with_tail)), y, d)
    # and the reference does not read the tail
    x2 = x.clone(); x2[..., S * win:] = float("nan")
    assert torch.equal(R.clf_fwd_ref(x2, P, win)[0], y)
