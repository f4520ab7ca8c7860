"""-m gpu: the U-Sleep forward kernel by kernel -- the inference path of csrc/usleep.hip (eval fold, batch statistics) and the taped training
forward of csrc/usleep_train.hip, through the primitive entries eegldm_usleep_layer_fwd / _maxpool_fwd / _clf_fwd, against the float64
references and operation-count bounds of tests/usleep_reference.py (proved sharp on the CPU by tests/test_usleep_fwd_numerics_cpu.py); small
whole networks the other files never build against the float64 oracle with the float32 oracle as the yardstick; non-finite inputs; and the
streaming feature moments at the edges of their row split.  Every shape is tiny: the file takes a few seconds of GPU time."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import usleep_reference as R  # noqa: E402
from param_gen import gen_param, normal  # noqa: E402

U = 2.0 ** -24
DEV = "cuda:0"
GUARD, SENTINEL = 64, -7.0e33


def _lib():
    import eegldm
    from eegldm._lib import lib, check, ptr
    return lib, check, ptr, eegldm.default_context(0)


def dev(t):
    return None if t is None else torch.as_tensor(t, dtype=torch.float32).contiguous().to(DEV)


class Guarded:
    """A device buffer with GUARD sentinel elements on both sides; the body starts NaN-filled (or holds `init`)."""

    def __init__(self, shape, init=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), device=DEV)
        self.buf[:GUARD] = SENTINEL; self.buf[GUARD + self.n:] = SENTINEL
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


def run_layer(c, mode, pooled=True):
    """-> the outputs of eegldm_usleep_layer_fwd on the CPU: y, rm, rv, nbt, [pooled], [z] (modes 1, 2), [stat] (mode 2); guards checked."""
    lib, check, ptr, ctx = _lib()
    B, L, Cout = c["B"], c["L"], c["Cout"]
    Lo = (L + (2 if L % 2 else 0)) // 2
    held = [dev(c[k]) for k in ("a", "b2", "w", "bias", "gamma", "beta")]
    a, b2, w, bias, gamma, beta = held
    g = dict(y=Guarded((B, Cout, L)), rm=Guarded((Cout,), c["rm"]), rv=Guarded((Cout,), c["rv"]), nbt=Guarded((1,), c["nbt"]))
    if pooled:
        g["pooled"] = Guarded((B, Cout, Lo))
    if mode:
        g["z"] = Guarded((B, Cout, L))
    if mode == 2:
        g["stat"] = Guarded((2 * Cout,))
    p = lambda k: ptr(g[k].t) if k in g else None
    check(lib.eegldm_usleep_layer_fwd(ctx.h, mode, ptr(a), c["Ca"], c["La"], c["ups"], ptr(b2), c["Cb"], c["Lb"], L, ptr(w), ptr(bias), ptr(gamma), ptr(beta),
                                      p("rm"), p("rv"), p("nbt"), B, Cout, c["K"], c["left"], p("y"), p("pooled"), p("z"), p("stat")))
    torch.cuda.synchronize()
    for k, v in g.items():
        assert v.intact(), f"guard elements of {k} overwritten"
    return {k: v.t.cpu().clone() for k, v in g.items()}


def maxpool_fwd(x):
    lib, check, ptr, ctx = _lib()
    nrows, L = int(np.prod(x.shape[:-1])), x.shape[-1]
    Lo = (L + (2 if L % 2 else 0)) // 2
    x_d = dev(x); y = Guarded((*x.shape[:-1], Lo))
    check(lib.eegldm_usleep_maxpool_fwd(ctx.h, ptr(x_d), ptr(y.t), nrows, L))
    torch.cuda.synchronize()
    assert y.intact(), "guard elements of the pooled output overwritten"
    return y.t.cpu().clone()


# ---------------------------------------------------------------------------------------------------- layer sweep
@pytest.mark.parametrize("form", ["plain", "ups", "ups_skip"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_layer_vs_float64(mode, form):
    """One conv -> + bias -> ELU -> BatchNorm -> pad + MaxPool layer over R.LAYER_SWEEP (one factor at a time around rows = 65, Cout = 17,
    Cin = 33, K = 7, plus three mixed corners), staged as R.judge_layer describes.  Outputs start NaN-filled between guard elements.  Mode 2: two
    runs bit-equal, the fused pass's pooled output bit-equal to eegldm_usleep_maxpool_fwd of its own y, gamma = 0 gives y == beta exactly.
    B * L = 1 belongs to mode 0 alone: batch statistics over one value do not exist."""
    worst, ulps, ran = {}, 0.0, 0
    for n, sw in enumerate(R.LAYER_SWEEP):
        c = R.layer_case(form, seed=200 + 7 * n, **sw)
        if mode and c["B"] * c["L"] < 2:
            continue
        out = run_layer(c, mode)
        w = R.judge_layer(f"mode {mode} {form} {sw}", c, mode, out)
        ulps = max(ulps, w.pop("expm1 ulps", 0.0))
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if mode == 2:
            again = run_layer(c, mode)
            assert all(R.check_exact(f"second run {k}", again[k], out[k]) is None for k in out), (form, sw)
            R.check_exact(f"mode 2 {form} {sw}: fused pooled against maxpool_fwd(y)", maxpool_fwd(out["y"]), out["pooled"])
            for ch, kind in enumerate(c["kinds"]):
                if kind == "gamma0":
                    assert torch.equal(out["y"][:, ch], c["beta"][ch].expand_as(out["y"][:, ch])), (form, sw, ch, "gamma == 0: y must be beta exactly")
        ran += 1
    route = ("eval fold", "inference path, batch statistics", "training path")[mode]
    print(f"[numerics] layer_fwd mode {mode} ({route}) {form}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          (f"; expm1f branch: worst error beyond the conv term {ulps:.2f} ulp of z (4 granted)" if mode else "") + f" over {ran} shapes")


def test_layer_refusals():
    c = R.layer_case("plain", seed=3, rows=1, Cout=4, Cin=3, K=3)
    with pytest.raises(RuntimeError, match="B \\* L >= 2"):
        run_layer(c, 1)
    with pytest.raises(RuntimeError, match="B \\* L >= 2"):
        run_layer(c, 2)


# ---------------------------------------------------------------------------------------------------- MaxPool
def pool_rows(L):
    """A coarse grid with ties, all-negative rows (the pad zero wins the first pair of an odd row), constant rows."""
    x = torch.round(R.rnd((12, L), 40 + L) * 2.0) / 2.0
    x[0] = -x[0].abs() - 0.5; x[1] = -1.0; x[2] = 0.0; x[3] = 1.0
    return x


def plant_nonfinite(x):
    """NaN at the first / last / both positions of a pair and at both ends of the row, +-inf beside them."""
    x = x.clone(); L = x.shape[-1]; odd = L % 2
    nan, inf = float("nan"), float("inf")
    x[4, 0] = nan; x[5, L - 1] = nan; x[6, 0] = inf; x[7, L - 1] = -inf; x[8, 0] = -inf; x[8, L - 1] = inf
    if L >= 3:
        p0 = 2 - odd                                             # an inner pair: positions p0, p0 + 1
        x[9, p0] = nan; x[10, p0 + 1] = nan; x[11, p0] = nan; x[11, p0 + 1] = nan
        x[4, p0 + 1] = inf; x[5, p0] = -inf
    return x


@pytest.mark.parametrize("L", [1, 2, 3, 47])
def test_maxpool_fwd_exact(L):
    """eegldm_usleep_maxpool_fwd against torch's pad + MaxPool1d(2): exact, and the NaN positions are torch's (a NaN wins its pair)."""
    x = pool_rows(L)
    R.check_pool(f"L={L}", maxpool_fwd(x), x)
    xn = plant_nonfinite(x)
    want = R.maxpool_fwd_ref(xn)
    assert bool(torch.isnan(want).any()) and not bool(torch.isnan(want).all())
    R.check_pool(f"L={L}, non-finite rows", maxpool_fwd(xn), xn)
    print(f"[numerics] maxpool_fwd L={L}: exact, {int(torch.isnan(want).sum())} NaN and {int(torch.isinf(want).sum())} infinite outputs as torch")


# ---------------------------------------------------------------------------------------------------- classifier head
@pytest.mark.parametrize("C1,ncls", [(1, 1), (6, 5), (16, 16)])
def test_clf_fwd_vs_float64(C1, ncls):
    """usleep_clf_kernel at S in {1, 2} and win in {1, 37, 300} (below, at and above one 256-thread pass), with a non-zero tail that must not be
    read: NaN there leaves the result bit-equal."""
    lib, check, ptr, ctx = _lib()
    worst = 0.0
    for S in (1, 2):
        for win in (1, 37, 300):
            tail = 5 if win > 1 else 0
            B, L = 3, S * win + tail
            x = R.rnd((B, C1, L), 70 + S + win)
            P = [R.rnd((C1, C1), 71, 0.5), R.rnd((C1,), 72, 0.1), R.rnd((ncls, C1), 73, 0.5), R.rnd((ncls,), 74, 0.1), R.rnd((ncls, ncls), 75, 0.5),
                 R.rnd((ncls,), 76, 0.1)]
            y_ref, d = R.clf_fwd_ref(x, P, win)
            Pd = [dev(p) for p in P]; wp = (C.c_void_p * 6)(*[p.data_ptr() for p in Pd])
            outs = []
            for poison in (False, True):
                xx = x.clone()
                if poison and tail:
                    xx[..., S * win:] = float("nan")
                x_d = dev(xx); y = Guarded((B, ncls, S))
                check(lib.eegldm_usleep_clf_fwd(ctx.h, ptr(x_d), wp, B, C1, L, win, ncls, ptr(y.t)))
                torch.cuda.synchronize()
                assert y.intact()
                outs.append(y.t.cpu().clone())
            assert torch.equal(outs[0], outs[1]), (C1, ncls, S, win, "the tail was read")
            worst = max(worst, R.check_bound(f"clf C1={C1} ncls={ncls} S={S} win={win}", outs[0], y_ref, d))
    print(f"[numerics] clf_fwd C1={C1} ncls={ncls}: worst error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------- whole network
NETS = {
    "d6_T37": dict(kw=dict(in_chans=2, depth=6, time_conv_size_s=0.07, input_size_s=0.12), B=3, T=37),     # lengths 37, 19, 10, 5, 3, 2, 1; S = 3, tail 1
    "d3_T64": dict(kw=dict(in_chans=2, depth=3, time_conv_size_s=0.07, input_size_s=0.64), B=3, T=64),
    "k3": dict(kw=dict(in_chans=2, depth=3, time_conv_size_s=0.03, input_size_s=0.2), B=2, T=45),
    "k9_in1": dict(kw=dict(in_chans=1, depth=3, time_conv_size_s=0.09, input_size_s=0.2), B=2, T=45),
    "k13_in3": dict(kw=dict(in_chans=3, depth=2, time_conv_size_s=0.13, input_size_s=0.2), B=2, T=50),
    "k15_noskip": dict(kw=dict(in_chans=2, depth=3, time_conv_size_s=0.15, input_size_s=0.2, with_skip_connection=False), B=2, T=45),
    "c16": dict(kw=dict(in_chans=2, depth=2, time_conv_size_s=0.07, input_size_s=0.2, n_time_filters=13), B=2, T=41),       # ch[1] = 16: the classifier's widest
}
_net_cache = {}


def net_case(name):
    """State dict, input and the float64 / float32 oracle forwards (eval and train) of a small network: computed once, never modified."""
    if name in _net_cache:
        return _net_cache[name]
    from oracle.usleep import usleep_forward, usleep_param_shapes
    spec = NETS[name]; kw = dict(sfreq=100, n_classes=5, **spec["kw"])
    skw = {k: kw[k] for k in ("in_chans", "sfreq", "depth", "n_time_filters", "n_classes", "time_conv_size_s", "with_skip_connection") if k in kw}
    shapes = usleep_param_shapes(**skw)
    sd = {k: torch.from_numpy(gen_param(78, k, s)) for k, s in shapes.items()}
    x = torch.from_numpy(normal((spec["B"], kw["in_chans"], spec["T"]), seed=6))
    win = int(np.ceil(kw["input_size_s"] * kw["sfreq"]))
    skip = kw.get("with_skip_connection", True)
    out = dict(kw=kw, sd=sd, x=x, win=win, skip=skip)
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        sdt = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
        for training in (False, True):
            running = {}
            with torch.no_grad():
                y, dec, bot = usleep_forward(sdt, x.to(dt), depth=kw["depth"], input_size=win, training=training, running=running, with_skip_connection=skip)
            out[("train" if training else "eval") + tag] = dict(y_pred=y.reshape(y.shape[0], 5, -1), decoder_out=dec, bottom=bot, running=running)
    _net_cache[name] = out
    return out


def native_net(nc):
    from eegldm.metrics import USleep
    m = USleep(**nc["kw"])
    assert {k: tuple(e[3]) for k, e in m.entries.items()} == {k: tuple(v.shape) for k, v in nc["sd"].items()}
    m.load_state_dict(nc["sd"])
    return m


def yardstick(name, got, o64, o32, lines, bad):
    """||native - f64|| <= 4 max(||f32 oracle - f64||, u ||f64||) for one tensor."""
    e_nat = float((got.detach().cpu().double() - o64).norm()); e_ref = float((o32.double() - o64).norm()); n64 = float(o64.norm())
    bound = 4 * max(e_ref, U * n64)
    lines.append(f"{name}: e_nat {e_nat:.3e} e_ref {e_ref:.3e} bound {bound:.3e}")
    if not e_nat <= bound:
        bad.append((name, e_nat, bound))
    return e_nat / bound if bound > 0 else 0.0


@pytest.mark.parametrize("name", list(NETS))
def test_small_networks_vs_oracle(name):
    """Eval mode on gen_param running statistics, train mode through USleep.forward (the inference path on batch statistics) and through
    forward_train (the training path): every output tensor and every updated running statistic against the float64 oracle, judged by the
    float32 oracle's own distance from it."""
    nc = net_case(name)
    lines, bad, worst = [], [], 0.0
    for mode in ("eval", "train"):
        m = native_net(nc)
        m.train(mode == "train")
        y, dec, bot = m(nc["x"])
        torch.cuda.synchronize()
        o64, o32 = nc[mode + "64"], nc[mode + "32"]
        for key, got in (("y_pred", y.reshape(y.shape[0], 5, -1)), ("decoder_out", dec), ("bottom", bot)):
            assert tuple(got.shape) == tuple(o64[key].shape), (name, mode, key, got.shape, o64[key].shape)
            worst = max(worst, yardstick(f"{mode} {key}", got, o64[key], o32[key], lines, bad))
        sd = m.state_dict()
        if mode == "eval":
            assert all(torch.equal(sd[k].cpu(), nc["sd"][k].float()) for k in sd if "running" in k), "eval mode changed a running statistic"
            assert all(int(v) == int(nc["sd"][k]) for k, v in sd.items() if k.endswith("num_batches_tracked")), "eval mode changed a counter"
        else:
            for k, v in o64["running"].items():
                worst = max(worst, yardstick(f"train {k}", sd[k], v, o32["running"][k], lines, bad))
            assert all(int(v) == int(nc["sd"][k]) + 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    m = native_net(nc)
    if not nc["skip"] and nc["x"].shape[-1] % (1 << nc["kw"]["depth"]):
        # without skip connections nothing is cropped: the decoder output (and the oracle's) is longer than T, which the inference path above
        # returns and the training wrapper refuses before any launch
        assert o64["decoder_out"].shape[-1] > nc["x"].shape[-1]
        with pytest.raises(ValueError, match="multiple of 2\\^depth"):
            m.forward_train(nc["x"])
        print(f"[numerics] network {name}: worst ||native - f64|| / (4 max(||f32 oracle - f64||, u ||f64||)) {worst:.3f} over {len(lines)} tensors")
        assert not bad, ("\n".join(lines), bad)
        return
    yt = m.forward_train(nc["x"])
    torch.cuda.synchronize()
    o64, o32 = nc["train64"], nc["train32"]
    worst = max(worst, yardstick("forward_train y_pred", yt, o64["y_pred"], o32["y_pred"], lines, bad))
    sd = m.state_dict()
    for k, v in o64["running"].items():
        worst = max(worst, yardstick(f"forward_train {k}", sd[k], v, o32["running"][k], lines, bad))
    assert all(int(v) == int(nc["sd"][k]) + 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    print(f"[numerics] network {name}: worst ||native - f64|| / (4 max(||f32 oracle - f64||, u ||f64||)) {worst:.3f} over {len(lines)} tensors")
    assert not bad, ("\n".join(lines), bad)


# ---------------------------------------------------------------------------------------------------- non-finite inputs
def nonfinite(t):
    return ~torch.isfinite(t.detach().cpu())


def poisoned_input(nc):
    """Four samples: one NaN sample value, one +inf sample value, one all-NaN channel, one clean."""
    kw = nc["kw"]
    x = torch.from_numpy(normal((4, kw["in_chans"], 64), seed=8))
    x[0, 0, 5] = float("nan"); x[1, 0, 20] = float("inf"); x[2, 1, :] = float("nan")
    return x


def test_nonfinite_inputs_whole_network():
    """Eval mode: the non-finite pattern of bottom, decoder_out and y_pred is the float64 oracle's, and that pattern is neither empty nor
    everything (the clean sample stays finite; the NaN that enters the encoder's pools at single positions must win its pair there, or the
    bottleneck is poisoned at fewer positions than the oracle's).  forward_train: BatchNorm on batch statistics spreads a NaN over the whole
    batch by construction (the channel mean is NaN), so the oracle's pattern there is everything; it must be matched, and be non-empty."""
    from oracle.usleep import usleep_forward
    nc = net_case("d3_T64")
    x = poisoned_input(nc)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in nc["sd"].items()}
    with torch.no_grad():
        y, dec, bot = usleep_forward(sd64, x.double(), depth=nc["kw"]["depth"], input_size=nc["win"], training=False)
        yt, _d, _b = usleep_forward(sd64, x.double(), depth=nc["kw"]["depth"], input_size=nc["win"], training=True)
    m = native_net(nc).eval()
    ny, ndec, nbot = m(x)
    torch.cuda.synchronize()
    for key, got, want in (("bottom", nbot, bot), ("decoder_out", ndec, dec), ("y_pred", ny.reshape(4, 5, -1), y.reshape(4, 5, -1))):
        pat = nonfinite(want)
        assert bool(pat.any()) and not bool(pat.all()), (key, "the oracle's pattern must be neither empty nor everything")
        diff = nonfinite(got) != pat
        assert not bool(diff.any()), (f"eval {key}: non-finite pattern differs from the oracle's at {int(diff.sum())} of {diff.numel()} positions "
                                      f"(native {int(nonfinite(got).sum())}, oracle {int(pat.sum())}): the encoder's pooled stage", diff.nonzero()[:4].tolist())
    m = native_net(nc)
    nyt = m.forward_train(x)
    torch.cuda.synchronize()
    pat = nonfinite(yt.reshape(4, 5, -1))
    assert bool(pat.any()) and torch.equal(nonfinite(nyt), pat)
    print(f"[numerics] non-finite d3_T64: eval patterns equal the oracle's (bottom {int(nonfinite(bot).sum())}/{bot.numel()}, decoder {int(nonfinite(dec).sum())}/"
          f"{dec.numel()}, y_pred {int(nonfinite(y).sum())}/{y.numel()}); forward_train {int(pat.sum())}/{pat.numel()}")


@pytest.mark.parametrize("mode", [0, 2])
def test_nonfinite_inputs_layer(mode):
    """The layer entry with pooled output on a K = 1 layer (a poisoned input position poisons that output position alone): one NaN, one +inf and
    one all-NaN input channel in separate samples.  Mode 0: y's pattern is the reference's, partial, and the pooled stage's is torch's on the stored
    y.  Mode 2: the batch statistics are NaN, every output is NaN, as the reference says; the pooled stage likewise -- L = 13 is odd, so the first pair
    of every row holds the pad's zero and a NaN, which the fused pass must not resolve to 0."""
    c = R.layer_case("plain", seed=31, rows=65, Cout=17, Cin=4, K=1)
    a = c["a"]
    a[0, 0, 5] = float("nan"); a[1, 0, 8] = float("inf"); a[1, 1, 3] = float("-inf"); a[2, 1, :c["L"]] = float("nan")
    out = run_layer(c, mode)
    w = R.judge_layer(f"non-finite layer mode {mode}", c, mode, out)          # check_bound compares the NaN / infinity patterns first
    pat = nonfinite(out["y"]); ppat = nonfinite(out["pooled"])
    assert bool(pat.any()) and bool(ppat.any())
    if mode == 0:
        assert not bool(pat.all()) and not bool(ppat.all())
        assert bool(torch.isfinite(out["y"][3:]).all()) and bool(torch.isnan(out["y"][0, :, 5]).all()) and bool(torch.isnan(out["y"][2]).all())
    else:
        assert bool(torch.isnan(out["y"]).all()) and bool(torch.isnan(out["pooled"]).all())
    print(f"[numerics] non-finite layer mode {mode}: y {int(pat.sum())}/{pat.numel()} non-finite, pooled {int(ppat.sum())}/{ppat.numel()}, as the reference; "
          f"finite part worst error / bound {max([v for k, v in w.items() if k != 'expm1 ulps'] or [0.0]):.3f}")


# ---------------------------------------------------------------------------------------------------- feature moments
@pytest.mark.parametrize("D", [1, 15, 16, 17])
def test_feature_moments_edges(D):
    """eegldm_feature_moments at N in {1, 63, 64, 65, 4097} (one row split; the split's first step; its cap of 64 splits with a ragged last one)
    against float64 numpy, with the tolerances of test_feature_moments_and_fid_vs_oracle; streaming in two chunks equals one shot within them."""
    lib, check, ptr, ctx = _lib()
    r = np.random.default_rng(100 + D)
    worst = 0.0
    for Nn in (1, 63, 64, 65, 4097):
        f = (r.standard_normal((Nn, D)) * 1.5 + 0.3).astype(np.float32)
        fd = torch.from_numpy(f).to(DEV)
        res = []
        for chunks in ((fd,), (fd[:Nn // 2 + 1], fd[Nn // 2 + 1:])):
            s = torch.zeros(D + 2 * GUARD, dtype=torch.float64, device=DEV); o = torch.zeros(D * D + 2 * GUARD, dtype=torch.float64, device=DEV)
            for ch in chunks:
                if ch.shape[0]:
                    ch = ch.contiguous()
                    check(lib.eegldm_feature_moments(ctx.h, ptr(ch), ch.shape[0], D, C.c_void_p(s.data_ptr() + 8 * GUARD), C.c_void_p(o.data_ptr() + 8 * GUARD)))
            torch.cuda.synchronize()
            assert not bool(s[:GUARD].any()) and not bool(s[GUARD + D:].any()) and not bool(o[:GUARD].any()) and not bool(o[GUARD + D * D:].any()), "guards"
            res.append((s[GUARD:GUARD + D].cpu().numpy(), o[GUARD:GUARD + D * D].cpu().numpy().reshape(D, D)))
        f64 = f.astype(np.float64)
        for s, o in res:
            mu = s / Nn
            assert np.allclose(mu, f64.mean(0), rtol=0, atol=1e-12 + 1e-12 * np.abs(f64.mean(0)).max()), (D, Nn)
            worst = max(worst, float(np.abs(mu - f64.mean(0)).max() / (1e-12 + 1e-12 * np.abs(f64.mean(0)).max())))
            assert np.allclose(o, f64.T @ f64, rtol=1e-9, atol=1e-11), (D, Nn)
            if Nn > 1:
                cov = (o - Nn * np.outer(mu, mu)) / (Nn - 1)
                assert np.allclose(cov, np.cov(f64, rowvar=False).reshape(D, D), rtol=1e-9, atol=1e-11), (D, Nn)
        assert np.allclose(res[0][0], res[1][0], rtol=1e-9, atol=1e-11) and np.allclose(res[0][1], res[1][1], rtol=1e-9, atol=1e-11), (D, Nn, "streaming")
    print(f"[numerics] feature_moments D={D}: mean worst error / tolerance {worst:.3f}; covariance within rtol 1e-9, atol 1e-11")
