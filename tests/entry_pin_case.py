"""Shared by tests/test_gpu_dpm_solver.py and tests/golden/make_golden_entry_pin.py: seeded stage-1 / UNet checkpoints written the way
the training scripts leave them, and one run of each sampling entry script over them.  No training is involved (a trained checkpoint
depends on the order of the gradient atomics), so the windows are a function of the seeds and the sampler alone."""
import os

import numpy as np
import torch
import yaml

from param_gen import gen_param

AEKL_YAML = {"autoencoderkl": {"params": {"spatial_dims": 1, "in_channels": 1, "out_channels": 1, "num_res_blocks": 2, "norm_num_groups": 1,
                                          "attention_levels": [False, False, False], "with_encoder_nonlocal_attn": False,
                                          "with_decoder_nonlocal_attn": False, "num_channels": [8, 8, 16], "latent_channels": 1}}}
LDM_YAML = {"model": {"params": {"timesteps": 1000, "unet_config": {"params": {
    "image_size": 768, "in_channels": 3, "out_channels": 1, "model_channels": 32, "attention_resolutions": [8, 4], "num_res_blocks": 1,
    "channel_mult": [1, 2, 4], "dropout": 0.0, "conv_resample": True, "num_heads": 1, "use_scale_shift_norm": False, "resblock_updown": True}}}}}
SEEDS = (3, 6)              # --start_seed / --stop_seed
STEPS = 5
SCALE_FACTOR = 0.8125


def _seeded(model, seed):
    return {k: torch.from_numpy(gen_param(seed, k, v.shape)) for k, v in model.state_dict().items()}


def write_checkpoints(out):
    """-> (aekl yaml, ldm yaml, stage-1 run dir, LDM run dir, pixel-space run dir)"""
    from eegldm.models import AutoencoderKL, UNetModel
    a_yaml, l_yaml = os.path.join(out, "aekl.yaml"), os.path.join(out, "ldm.yaml")
    yaml.safe_dump(AEKL_YAML, open(a_yaml, "w")); yaml.safe_dump(LDM_YAML, open(l_yaml, "w"))
    run_a, run_l, run_d = (os.path.join(out, d) for d in ("aekl_eeg", "ldm_eeg", "dm_eeg"))
    for d in (run_a, run_l, run_d):
        os.makedirs(d, exist_ok=True)
    torch.save(_seeded(AutoencoderKL(**AEKL_YAML["autoencoderkl"]["params"]), 301), os.path.join(run_a, "best_model.pth"))
    up = dict(LDM_YAML["model"]["params"]["unet_config"]["params"], in_channels=1, out_channels=1)
    sd = _seeded(UNetModel(**up), 302)
    torch.save(sd, os.path.join(run_l, "best_model.pth")); torch.save(sd, os.path.join(run_d, "best_model.pth"))
    torch.save({"scale_factor": SCALE_FACTOR}, os.path.join(run_l, "checkpoint.pth"))
    return a_yaml, l_yaml, run_a, run_l, run_d


def _windows(sdir):
    return np.stack([np.load(os.path.join(sdir, f"sample_{i}.npy")) for i in range(*SEEDS)])


def run_sample_trials(out, paths, extra=()):
    from eegldm.entry import sample_trials as ST
    a_yaml, l_yaml, run_a, run_l, _run_d = paths
    sdir = ST.main(ST.parse_args(["--output_dir", out, "--best_model_path", run_a, "--diffusion_path", run_l,
                                  "--autoencoderkl_config_file_path", a_yaml, "--ldm_config_file_path", l_yaml, "--start_seed", str(SEEDS[0]),
                                  "--stop_seed", str(SEEDS[1]), "--num_inference_steps", str(STEPS), "--latent_channels", "1", *extra]))
    return _windows(sdir)


def run_sample_trials_dm(out, paths, extra=()):
    from eegldm.entry import sample_trials_dm as SD
    _a, l_yaml, _run_a, _run_l, run_d = paths
    sdir = SD.main(SD.parse_args(["--output_dir", out, "--config_file", l_yaml, "--diffusion_path", run_d, "--start_seed", str(SEEDS[0]),
                                  "--stop_seed", str(SEEDS[1]), "--num_inference_steps", str(STEPS), *extra]))
    return _windows(sdir)
