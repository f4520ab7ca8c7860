"""CPU: the host side of the weighted diffusion loss -- weight tables (schedulers.loss_weights) against an independent float64 restatement,
their identities and refusals, the new flags of the train scripts, and the NoiseLevelLoss accumulator against numpy."""
import math

import numpy as np
import pytest
import torch

GAMMA = 5.0
# the two schedules the trainers build (train_ldm.py --schedule; DDPMScheduler(1000, ., 0.0015, 0.0195))
SCHEDULES = ["linear_beta", "scaled_linear_beta"]
PREDS = ["epsilon", "v_prediction", "sample"]


def _acp(schedule):
    from eegldm.schedulers import _betas
    return torch.cumprod(1.0 - _betas(schedule, 1000, 0.0015, 0.0195), dim=0)


def _restated(acp, pred, gamma):
    """The table of the issue, written again from the definitions: float64 numpy on the float32 alphas_cumprod values."""
    a = acp.double().numpy()
    snr = a / (1.0 - a)
    m = np.minimum(snr, gamma)
    return {"epsilon": m / snr, "v_prediction": m / (snr + 1.0), "sample": m}[pred]


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("pred", PREDS)
def test_tables_equal_the_float64_restatement(schedule, pred):
    from eegldm.schedulers import loss_weights
    acp = _acp(schedule)
    for gamma in (GAMMA, 1.0, 20.0):
        got = loss_weights(acp, "min_snr", pred, gamma)
        want = _restated(acp, pred, gamma)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (1000,)
        # both sides are float64 evaluations of a few operations: they agree far inside one float32 ulp, and so do their float32 roundings
        assert (np.abs(got - want) <= _ulp32(want)).all()
        assert (np.abs(got.astype(np.float32).astype(np.float64) - want) <= _ulp32(want)).all()
    ones = loss_weights(acp, "none", pred)
    assert ones.dtype == np.float64 and (ones == 1.0).all() and ones.shape == (1000,)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_table_identities(schedule):
    from eegldm.schedulers import loss_weights
    acp = _acp(schedule)
    a = acp.double().numpy(); snr = a / (1.0 - a)
    we, wv, ws = (loss_weights(acp, "min_snr", p, GAMMA) for p in PREDS)
    low = snr <= GAMMA
    assert low.any() and (~low).any()
    assert (we[low] == 1.0).all() and (we[~low] < 1.0).all()                       # SNR / SNR is exactly 1
    assert np.allclose(wv, we * snr / (snr + 1.0), rtol=4 * np.finfo(np.float64).eps, atol=0.0)
    assert np.allclose(ws, we * snr, rtol=4 * np.finfo(np.float64).eps, atol=0.0)
    # SNR falls strictly with t.  epsilon: min(SNR, g) / SNR rises to 1 and stays; sample: min(SNR, g) stays at g and then falls;
    # v: g / (SNR + 1) rises while SNR > g and SNR / (SNR + 1) falls after -- one peak, at the clamp point.
    assert (np.diff(snr) < 0).all()
    assert (np.diff(we) >= 0).all() and (np.diff(ws) <= 0).all()
    k = int(np.argmax(low))                                                      # first timestep with SNR <= gamma
    assert (np.diff(wv[:k]) > 0).all() and (np.diff(wv[k:]) < 0).all()
    assert (we > 0).all() and (wv > 0).all() and (ws > 0).all() and (wv < 1).all()


def test_user_table_is_taken_as_it_is():
    from eegldm.schedulers import loss_weights
    acp = _acp("linear_beta")
    tab = np.linspace(0.0, 2.0, 1000)
    for given in (tab, list(tab), torch.from_numpy(tab), torch.from_numpy(tab).float()):
        got = loss_weights(acp, given, "epsilon")
        assert got.dtype == np.float64 and np.allclose(got, tab, rtol=1e-7, atol=0)


@pytest.fixture
def native_calls_fail(monkeypatch):
    """Every compute entry of the native library raises: a refusal that reaches one was not raised on the host."""
    from eegldm import _lib, losses, schedulers, training

    class Dead:
        def __getattr__(self, name):
            raise AssertionError(f"native call {name} reached")

    def no_context(*a, **k):
        raise AssertionError("a device context was requested")
    for mod in (losses, schedulers, training):
        monkeypatch.setattr(mod, "lib", Dead())
    for mod in (losses, schedulers, _lib):
        monkeypatch.setattr(mod, "default_context", no_context)


class _Sched:
    """What the train steps read of a scheduler, without a device."""
    prediction_type = "epsilon"
    num_train_timesteps = 1000
    device = "cpu"

    def __init__(self):
        self.alphas_cumprod = _acp("linear_beta")
        self._acp_dev = self.alphas_cumprod


BAD = [("p2", 5.0, "unknown loss weighting"), ("min_snr", 0.0, "snr_gamma"), ("min_snr", -1.0, "snr_gamma"), ("min_snr", math.inf, "snr_gamma"),
       ("min_snr", math.nan, "snr_gamma"), ("none", math.inf, "snr_gamma"), (np.ones(999), 5.0, "shape"), (np.ones((1000, 1)), 5.0, "shape"),
       (-np.ones(1000), 5.0, "finite and >= 0"), (np.full(1000, np.nan), 5.0, "finite and >= 0"), (np.full(1000, np.inf), 5.0, "finite and >= 0")]


@pytest.mark.parametrize("weighting,gamma,msg", BAD, ids=[str(i) for i in range(len(BAD))])
def test_refusals_before_the_device_is_touched(native_calls_fail, weighting, gamma, msg):
    from eegldm import losses, schedulers, training
    sched = _Sched()
    with pytest.raises(ValueError, match=msg):
        schedulers.loss_weights(sched.alphas_cumprod, weighting, "epsilon", gamma)
    with pytest.raises(ValueError, match=msg):
        schedulers.device_loss_weights(sched, weighting, gamma)
    x = torch.zeros(2, 1, 8); t = torch.zeros(2, dtype=torch.int64)

    class Net:
        device, num_classes = "cpu", None
    with pytest.raises(ValueError, match=msg):
        training.ldm_train_step(Net(), sched, x, x, t, loss_weighting=weighting, snr_gamma=gamma)
    with pytest.raises(ValueError, match=msg):
        training.dm_train_step(Net(), sched, x, x, t, loss_weighting=weighting, snr_gamma=gamma)
    with pytest.raises(ValueError, match=msg):
        losses.diffusion_loss(x, x, x, t, sched, weighting=weighting, snr_gamma=gamma)


def test_per_sample_out_needs_the_weighted_loss(native_calls_fail):
    from eegldm import training
    x = torch.zeros(2, 1, 8); t = torch.zeros(2, dtype=torch.int64)

    class Net:
        device, num_classes = "cpu", None
    with pytest.raises(ValueError, match="per_sample_out"):
        training.ldm_train_step(Net(), _Sched(), x, x, t, per_sample_out=torch.zeros(2))
    with pytest.raises(ValueError, match="per_sample_out"):
        training.ldm_train_step(Net(), _Sched(), x, x, t, loss_weighting="none", per_sample_out=torch.zeros(3))
    with pytest.raises(ValueError, match="prediction_type"):
        from eegldm.schedulers import loss_weights
        loss_weights(_acp("linear_beta"), "min_snr", "velocity")


def test_new_flags_parse():
    from eegldm.entry import common, train_dm as TD, train_ldm as TL
    base = {TL: ["--config_file", "c.yaml", "--autoencoderkl_config_file_path", "a.yaml"], TD: ["--config_file", "c.yaml"]}
    for mod, argv in base.items():
        a = mod.parse_args(argv)
        assert a.loss_weighting is None and a.snr_gamma == 5.0 and a.loss_by_noise_level == 0
        assert common.step_weighting(a) == {}
        a = mod.parse_args(argv + ["--loss_weighting", "min_snr", "--snr_gamma", "3.5", "--loss_by_noise_level", "10"])
        assert a.loss_weighting == "min_snr" and a.snr_gamma == 3.5 and a.loss_by_noise_level == 10
        assert common.step_weighting(a) == {"loss_weighting": "min_snr", "snr_gamma": 3.5}
        a = mod.parse_args(argv + ["--loss_by_noise_level", "4"])
        assert common.step_weighting(a) == {"loss_weighting": "none", "snr_gamma": 5.0}      # per-sample losses come from the weighted loss
        assert mod.parse_args(argv + ["--loss_weighting", "none"]).loss_weighting == "none"
        with pytest.raises(SystemExit):
            mod.parse_args(argv + ["--loss_weighting", "p2"])


def test_resume_restores_or_refuses():
    from eegldm.entry import common, train_ldm as TL
    argv = ["--config_file", "c.yaml", "--autoencoderkl_config_file_path", "a.yaml"]
    ck = {"loss_weighting": {"weighting": "min_snr", "snr_gamma": 3.0}}
    a = TL.parse_args(argv); common.loss_weighting_resume(a, ck)
    assert a.loss_weighting == "min_snr" and a.snr_gamma == 3.0
    a = TL.parse_args(argv + ["--loss_weighting", "min_snr", "--snr_gamma", "3"]); common.loss_weighting_resume(a, ck)
    a = TL.parse_args(argv); common.loss_weighting_resume(a, {})
    assert a.loss_weighting is None
    for flags, saved in ((["--loss_weighting", "none"], ck), (["--loss_weighting", "min_snr"], ck), (["--loss_weighting", "min_snr"], {})):
        with pytest.raises(ValueError, match="loss_weighting"):
            common.loss_weighting_resume(TL.parse_args(argv + flags), saved)


def _numpy_bins(ps, ts, T, K):
    s, n = np.zeros(K), np.zeros(K, dtype=np.int64)
    for m, t in zip(ps, ts):
        s[t * K // T] += m; n[t * K // T] += 1
    return s, n


@pytest.mark.parametrize("T,K", [(1000, 10), (1000, 7), (10, 10), (1000, 1)])
def test_noise_level_loss_binning_merge_reset(T, K):
    from eegldm.training import NoiseLevelLoss
    r = np.random.default_rng(T + K)
    ts = np.concatenate([r.integers(0, T, 300), [0, T - 1], [-(-k * T // K) for k in range(K)]]).astype(np.int64)
    ps = r.random(len(ts)) * 10.0 ** r.integers(-4, 1, len(ts))
    acc = NoiseLevelLoss(T, bins=K)
    acc.add(ps[:100], ts[:100]).add(torch.from_numpy(ps[100:]), torch.from_numpy(ts[100:]))
    s, n = _numpy_bins(ps, ts, T, K)
    rows = acc.table()
    assert [r_["count"] for r_ in rows] == n.tolist() and sum(r_["count"] for r_ in rows) == len(ts)
    for k, row in enumerate(rows):
        inside = [t for t in range(T) if t * K // T == k]
        assert (row["t_lo"], row["t_hi"]) == (inside[0], inside[-1])
        assert row["mean"] == pytest.approx(s[k] / n[k], rel=1e-12)
    # merge over one process leaves the sums; two accumulators add through their states
    before = acc.state()
    assert acc.merge().state() == before and len(before) == 2 * K
    other = NoiseLevelLoss(T, bins=K).add(ps[:50], ts[:50])
    both = NoiseLevelLoss(T, bins=K).load_state([a + b for a, b in zip(acc.state(), other.state())])
    s2, n2 = _numpy_bins(np.concatenate([ps, ps[:50]]), np.concatenate([ts, ts[:50]]), T, K)
    assert [r_["count"] for r_ in both.table()] == n2.tolist()
    assert np.allclose([r_["mean"] for r_ in both.table()], s2 / n2, rtol=1e-12)
    acc.reset()
    assert all(r_["count"] == 0 and r_["mean"] is None for r_ in acc.table())
    # timesteps outside [0, T) are not counted
    assert sum(r_["count"] for r_ in NoiseLevelLoss(T, K).add([1.0, 1.0, 1.0], [-1, T, 0]).table()) == 1
    with pytest.raises(ValueError):
        NoiseLevelLoss(T, bins=0)
    with pytest.raises(ValueError):
        acc.add([1.0], [1, 2])


def test_device_table_is_built_once(monkeypatch):
    """Every weighted train step asks for the device table: after the first call a named weighting is a dictionary lookup (the host
    table is not rebuilt, alphas_cumprod is not read), "none" never builds one, and a user table is converted once per object."""
    from eegldm import schedulers
    sched = _Sched()
    calls = []
    real = schedulers.loss_weights
    monkeypatch.setattr(schedulers, "loss_weights", lambda *a, **k: (calls.append(a[1] if isinstance(a[1], str) else "table"), real(*a, **k))[1])
    first = schedulers.device_loss_weights(sched, "min_snr", 5.0)
    assert calls == ["min_snr"] and first.dtype == torch.float32 and tuple(first.shape) == (1000,)
    assert np.array_equal(first.numpy(), real(sched.alphas_cumprod, "min_snr", "epsilon", 5.0).astype(np.float32))

    class Unreadable:
        def __iter__(self):
            raise AssertionError("alphas_cumprod was read on a cache hit")
    acp, sched.alphas_cumprod = sched.alphas_cumprod, Unreadable()
    for _ in range(3):
        assert schedulers.device_loss_weights(sched, "min_snr", 5.0) is first
        assert schedulers.device_loss_weights(sched, "none", 5.0) is None
    assert calls == ["min_snr"]
    with pytest.raises(ValueError, match="snr_gamma"):          # the cheap refusals still come on every call
        schedulers.device_loss_weights(sched, "min_snr", math.inf)
    with pytest.raises(ValueError, match="unknown loss weighting"):
        schedulers.device_loss_weights(sched, "p2", 5.0)
    sched.alphas_cumprod = acp
    other = schedulers.device_loss_weights(sched, "min_snr", 3.0)      # another gamma / prediction type is another entry
    sched.prediction_type = "v_prediction"
    v = schedulers.device_loss_weights(sched, "min_snr", 5.0)
    assert calls == ["min_snr"] * 3 and other is not first and v is not first and not torch.equal(v, first)
    sched.prediction_type = "epsilon"
    assert schedulers.device_loss_weights(sched, "min_snr", 5.0) is first and calls == ["min_snr"] * 3
    tab = torch.linspace(0.0, 2.0, 1000)
    t1 = schedulers.device_loss_weights(sched, tab)
    assert schedulers.device_loss_weights(sched, tab) is t1 and calls[3:] == ["table"]
    assert schedulers.device_loss_weights(sched, tab.clone()) is not t1 and calls[3:] == ["table", "table"]


def test_per_sample_out_must_live_on_the_models_device(native_calls_fail):
    from eegldm import training
    x = torch.zeros(2, 1, 8); t = torch.zeros(2, dtype=torch.int64)

    class Net:
        device, num_classes = torch.device("cuda", 0), None
    with pytest.raises(ValueError, match="device"):
        training.ldm_train_step(Net(), _Sched(), x, x, t, loss_weighting="none", per_sample_out=torch.zeros(2))
    with pytest.raises(ValueError, match="device"):
        training.dm_train_step(Net(), _Sched(), x, x, t, loss_weighting="none", per_sample_out=torch.zeros(2))
