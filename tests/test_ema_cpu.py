"""CPU: the weight EMA's host side -- decay schedule, argument validation of the three C entry points (no device is touched) and the
flags of the four entry scripts."""
import ctypes as C
import types

import pytest
import torch


def _host_model(n=8):
    """What EMA needs of a model, without a GPU: a flat buffer and a parameter table."""
    return types.SimpleNamespace(flat=torch.arange(n, dtype=torch.float32), entries={"w": (0, n, (n,))}, sync_weights=lambda: None)


@pytest.mark.parametrize("n", [0, 1, 9, 10 ** 6])
def test_decay_schedule_closed_form(n):
    from eegldm import EMA
    from eegldm.training import EMA as EMA2
    assert EMA is EMA2
    for decay in (0.9999, 0.999, 0.5, 0.0):
        warm = EMA(_host_model(), decay=decay, warmup=True)
        const = EMA(_host_model(), decay=decay, warmup=False)
        assert warm.decay_at(n) == min(decay, (1 + n) / (10 + n))
        assert const.decay_at(n) == decay
    # spelled out: 1/10, 2/11, 10/19 while below the target, the target afterwards
    want = {0: 0.1, 1: 2 / 11, 9: 10 / 19, 10 ** 6: 0.9999}[n]
    assert EMA(_host_model(), decay=0.9999).decay_at(n) == want
    # the value handed to the kernel: 1 - decay in double, for the NEXT update
    e = EMA(_host_model(), decay=0.9999)
    e.num_updates = n
    assert e.one_minus_decay() == 1.0 - want


def test_construction_state_and_bad_decay():
    from eegldm import EMA
    md = _host_model()
    e = EMA(md)
    assert e.decay == 0.9999 and e.warmup is True and e.num_updates == 0
    assert torch.equal(e.shadow, md.flat) and e.shadow.data_ptr() != md.flat.data_ptr()
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            EMA(md, decay=bad)
    with pytest.raises(ValueError):
        e.decay_at(-1)
    # state dict: a plain model state dict in the table's order; load is its inverse
    sd = e.state_dict()
    assert list(sd) == ["w"] and torch.equal(sd["w"], md.flat)
    e.load_state_dict({"w": torch.full((8,), 2.0)}, num_updates=7)
    assert e.num_updates == 7 and float(e.shadow.sum()) == 16.0


def test_adam_refuses_an_ema_of_another_model():
    from eegldm.training import Adam, EMA
    a, b = _host_model(), _host_model()
    a.flat_grad = torch.zeros(8)
    with pytest.raises(ValueError, match="another model"):
        Adam(a, ema=EMA(b))
    assert Adam(a, ema=EMA(a)).ema is not None and Adam(a).ema is None


def _err():
    from eegldm._lib import lib
    return lib.eegldm_last_error().decode()


def test_entry_points_reject_bad_arguments_without_a_device():
    """Null, negative-n and aliased buffers fail with a message before anything is launched: ctx is NULL in every call, so reaching the
    device would crash rather than return.  The buffers are host arrays whose addresses are only compared."""
    from eegldm._lib import lib
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    at = lambda i: C.c_void_p(base + 4 * i)
    p, g, m, v, e = at(0), at(8), at(16), at(24), at(32)
    adam = lambda p, g, m, v, e, n=8: lib.eegldm_adam_step_ema(None, p, g, m, v, e, n, 1e-4, 0.9, 0.999, 1e-8, 1, 1.0, 1e-4)
    for args in ((None, g, m, v, e), (p, None, m, v, e), (p, g, None, v, e), (p, g, m, None, e), (p, g, m, v, None)):
        assert adam(*args) != 0 and "null" in _err() and "eegldm_adam_step_ema" in _err()
    assert adam(p, g, m, v, e, -1) != 0 and "negative n" in _err()
    assert adam(p, g, m, v, p) != 0 and "alias" in _err()                 # ema == p
    assert adam(p, g, m, v, at(4)) != 0 and "alias" in _err()             # ema overlaps the tail of p
    assert adam(p, g, m, v, m) != 0 and "alias" in _err()
    assert adam(p, g, m, v, e) != 0 and "null ctx" in _err()              # valid buffers: only then is the context looked at

    assert lib.eegldm_ema_update(None, None, p, 8, 0.1) != 0 and "null" in _err() and "eegldm_ema_update" in _err()
    assert lib.eegldm_ema_update(None, e, None, 8, 0.1) != 0 and "null" in _err()
    assert lib.eegldm_ema_update(None, e, p, -3, 0.1) != 0 and "negative n" in _err()
    assert lib.eegldm_ema_update(None, p, p, 8, 0.1) != 0 and "alias" in _err()
    assert lib.eegldm_ema_update(None, p, p, 0, 0.1) != 0 and "alias" in _err()      # the same buffer is refused whatever n is
    assert lib.eegldm_ema_update(None, e, p, 8, 0.1) != 0 and "null ctx" in _err()

    assert lib.eegldm_swap(None, None, p, 8) != 0 and "null" in _err() and "eegldm_swap" in _err()
    assert lib.eegldm_swap(None, p, None, 8) != 0 and "null" in _err()
    assert lib.eegldm_swap(None, p, g, -1) != 0 and "negative n" in _err()
    assert lib.eegldm_swap(None, p, p, 8) != 0 and "alias" in _err()
    assert lib.eegldm_swap(None, p, at(7), 8) != 0 and "alias" in _err()
    assert lib.eegldm_swap(None, p, g, 8) != 0 and "null ctx" in _err()


def test_entry_scripts_take_the_ema_flags_and_default_them_off():
    from eegldm.entry import sample_trials as ST, sample_trials_dm as SD, train_dm as TD, train_ldm as TL
    ldm = ["--config_file", "c.yaml", "--autoencoderkl_config_file_path", "a.yaml"]
    a = TL.parse_args(ldm)
    assert a.ema_decay is None and a.ema_no_warmup is False
    a = TL.parse_args(ldm + ["--ema_decay", "0.999", "--ema_no_warmup"])
    assert a.ema_decay == 0.999 and a.ema_no_warmup is True
    a = TD.parse_args(["--config_file", "c.yaml"])
    assert a.ema_decay is None and a.ema_no_warmup is False
    a = TD.parse_args(["--config_file", "c.yaml", "--ema_decay", "0.9"])
    assert a.ema_decay == 0.9 and a.ema_no_warmup is False
    st = ["--output_dir", "o", "--best_model_path", "b", "--diffusion_path", "d", "--autoencoderkl_config_file_path", "a.yaml",
          "--ldm_config_file_path", "l.yaml"]
    assert ST.parse_args(st).use_ema is False and ST.parse_args(st + ["--use_ema"]).use_ema is True
    sd = ["--output_dir", "o", "--config_file", "c.yaml", "--diffusion_path", "d"]
    assert SD.parse_args(sd).use_ema is False and SD.parse_args(sd + ["--use_ema"]).use_ema is True
