"""CPU: the class-conditional UNet's restatement (tests/cond_unet.py) against the goldens the reference produced
(tests/golden/make_golden_cond.py), and the sleep-stage labels of WindowLoader (centre-sample rule of run_sleep_decode.py:44-47)."""
import os

import numpy as np
import pytest
import torch

from make_golden_cond import COND_CASES, golden_path
from param_gen import gen_param, normal, timesteps


def test_restated_conditional_forward_matches_reference_golden():
    from cond_unet import cond_param_shapes, unet_forward_cond
    kw, B, L, labels, seed = COND_CASES["small_k5"]
    g = np.load(golden_path("small_k5"))
    shapes = cond_param_shapes(kw)
    assert list(shapes) == [str(k) for k in g["keys"]] and len(shapes) == 279
    sd = {k: torch.from_numpy(gen_param(seed, k, s)).requires_grad_(True) for k, s in shapes.items()}
    x = torch.from_numpy(normal((B, kw["in_channels"], L), seed=seed + 1)).requires_grad_(True)
    t = torch.from_numpy(g["t"])
    assert g["labels"].tolist() == labels
    y = unet_forward_cond(sd, kw, x, t, torch.from_numpy(g["labels"]))
    y.backward(torch.from_numpy(normal(tuple(y.shape), seed=seed + 3)))
    np.testing.assert_allclose(y.detach().numpy(), g["y"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(x.grad.numpy(), g["dx"], rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(sd["label_emb.weight"].grad.numpy(), g["g_label_emb"], rtol=1e-4, atol=1e-5)
    for k in shapes:
        gr = sd[k].grad.double().reshape(-1)
        assert abs(float(gr.norm()) - float(g["g_l2:" + k])) <= 1e-4 * float(g["g_l2:" + k]) + 1e-7, k
    # classes absent from the batch (2 and 3) get exactly nothing
    assert not g["g_label_emb"][[2, 3]].any() and g["g_label_emb"][[0, 1, 4]].any()


def test_full_size_golden_key_list():
    from cond_unet import cond_param_shapes
    kw = COND_CASES["full_k6"][0]
    g = np.load(golden_path("full_k6"))
    keys = [str(k) for k in g["keys"]]
    assert keys == list(cond_param_shapes(kw)) and len(keys) == 279 and keys[4] == "label_emb.weight"
    assert tuple(g["g_label_emb"].shape) == (6, 512) and int(g["n_params"]) == 30537731


def _stage_recording(tmp_path, n_samples, stages, name="SC4001E0-PSG-Fpz-Cz"):
    rec = np.arange(n_samples, dtype=np.float64)[None] * 1e-9      # a ramp: the window's first value gives its crop start back
    np.save(tmp_path / f"{name}.npy", rec)
    np.save(tmp_path / f"{name}.stages.npy", np.asarray(stages, dtype=np.int64))
    return n_samples


def _start_of(window, n_samples):
    return int(round(float(window[0, 36]) * (n_samples - 1)))


def test_window_loader_centre_sample_labels(tmp_path):
    from eegldm.entry.common import WindowLoader
    n = _stage_recording(tmp_path, 9000, [0, 2, 4])
    # centre sample = start + 1500: start 1499 -> sample 2999 (epoch 0), 1500 -> 3000 (epoch 1), 6000 -> 7500 (epoch 2)
    starts = [1499, 1500, 6000, 0]
    ld = WindowLoader(str(tmp_path), batch_size=4, shuffle=False, crop_starts=starts, windows_per_recording=4, stages=True)
    assert len(ld.files) == 1                                  # the stage file is not taken for a recording
    batch = next(iter(ld))
    assert batch["label"].dtype == torch.int64 and batch["label"].tolist() == [0, 2, 4, 0]
    assert [_start_of(w, n) for w in batch["eeg"]] == starts
    # without stages: the same loader output as before, no label
    plain = next(iter(WindowLoader(str(tmp_path), batch_size=4, shuffle=False, crop_starts=starts, windows_per_recording=4)))
    assert set(plain) == {"eeg"} and torch.equal(plain["eeg"], batch["eeg"])


def test_window_loader_redraws_unscored_centres(tmp_path):
    from eegldm.entry.common import WindowLoader
    n = _stage_recording(tmp_path, 12000, [-1, 3, -1, 1])
    starts = [0, 6000] * 8                                    # centres in epochs 0 and 2: unscored, drawn again
    ld = WindowLoader(str(tmp_path), batch_size=16, shuffle=False, crop_starts=starts, windows_per_recording=16, stages=True, seed=5)
    batch = next(iter(ld))
    for w, lab in zip(batch["eeg"], batch["label"].tolist()):
        s = _start_of(w, n)
        assert lab == [-1, 3, -1, 1][(s + 1500) // 3000] and lab in (3, 1)


def test_window_loader_stage_dir_and_missing_file(tmp_path):
    from eegldm.entry.common import WindowLoader
    (tmp_path / "rec").mkdir(); (tmp_path / "st").mkdir()
    np.save(tmp_path / "rec" / "A.npy", np.arange(6000, dtype=np.float64)[None])
    with pytest.raises(FileNotFoundError):
        WindowLoader(str(tmp_path / "rec"), batch_size=1, stages=True)
    np.save(tmp_path / "st" / "A.stages.npy", np.array([2, 2], np.int64))
    ld = WindowLoader(str(tmp_path / "rec"), batch_size=1, stages=True, path_stages=str(tmp_path / "st"))
    assert next(iter(ld))["label"].tolist() == [2]
