"""DDIM sampling of 30-s EEG windows: the loop of /root/reference/src/sample_trials.py:149-170
(noise -> UNet/DDIM steps -> decode(z / scale_factor) -> crop [36:-36]), batched over seeds instead of
one window at a time (the reference runs batch 1, which is launch-bound), with the step count a real
parameter (the reference hard-codes 200, sample_trials.py:144)."""
import ctypes as C
import os

import torch

from ._lib import lib, check, ptr, PRED
from .schedulers import DDIMScheduler, DPMSolverMultistepScheduler
from .training import randn


def _step_tables(scheduler):
    """Host-side schedule arrays for eegldm_sample: (timesteps, a_t, a_prev, beta_t, ancestral)."""
    from .schedulers import DDPMScheduler
    ts = [int(t) for t in scheduler.timesteps]
    acp = scheduler.alphas_cumprod
    ancestral = isinstance(scheduler, DDPMScheduler)
    if ancestral:
        prev = [t - 1 for t in ts]
        final = 1.0
    else:
        ratio = scheduler.num_train_timesteps // scheduler.num_inference_steps
        prev = [t - ratio for t in ts]
        final = scheduler.final_alpha_cumprod
    a_t = [float(acp[t]) for t in ts]
    a_prev = [float(acp[p]) if p >= 0 else float(final) for p in prev]
    beta = [float(scheduler.betas[t]) for t in ts]
    return ts, a_t, a_prev, beta, ancestral


def _multistep_tables(scheduler):
    """Host-side arrays for eegldm_sample_multistep: (timesteps, a_t, cx, c0, c1), the coefficients as set_timesteps computed them."""
    ts = [int(t) for t in scheduler.timesteps]
    return ts, [float(scheduler.alphas_cumprod[t]) for t in ts], list(scheduler.cx), list(scheduler.c0), list(scheduler.c1)


def _labels_host(unet, labels, B, guidance_scale, null_class):
    """(labels as a host int64 list of B entries, null class) for a class-conditional UNet; checked before anything runs."""
    if getattr(unet, "num_classes", None) is None:
        if labels is not None or float(guidance_scale) != 1.0:
            raise ValueError("labels / guidance_scale need a UNet built with num_classes")
        return None, 0
    if labels is None:
        raise ValueError("a class-conditional UNet samples with labels: pass labels=")
    lab = torch.as_tensor(labels).reshape(-1)
    if lab.numel() == 1:
        lab = lab.expand(B)
    if lab.numel() != B:
        raise ValueError(f"{lab.numel()} labels for {B} samples")
    lab = [int(v) for v in unet.check_labels(lab).cpu()]
    nc = 0
    if float(guidance_scale) != 1.0:
        if null_class is None:
            raise ValueError("guidance_scale != 1 needs null_class")
        nc = int(null_class)
        if not 0 <= nc < unet.num_classes:
            raise IndexError(f"null_class {nc} is out of range for num_classes={unet.num_classes}")
    return lab, nc


@torch.no_grad()
def ddim_sample(unet, autoencoder, scheduler, noise, scale_factor=1.0, crop=36, use_graph=None, seed=0, info=None, labels=None,
                guidance_scale=1.0, null_class=None):
    """noise (B, lat, Ll) on the device -> (windows (B, out, 3072 - 2*crop), final latents).  ONE native call
    (eegldm_sample): the scheduler loop, z / scale_factor and the decode run inside the library.  The UNet forward CAN be
    replayed from a hipGraph (use_graph=True or EEGLDM_SAMPLE_GRAPH=1) but that is no longer the default: measured on
    MI355X (rounds 2 and 3) the replay is SLOWER than the eager launches at the reference's batch of one window per call
    (sample_trials.py:149-163: 92.6 vs 87 ms per 50-step window -- ROCm's graph launch does not shorten the ~5 us per
    dependent kernel) and indistinguishable at batch 256, where launch overhead does not matter.
    `scheduler` may be a DDIMScheduler (eta 0), a DDPMScheduler (ancestral steps; noise from the device Philox
    stream `seed`) or a DPMSolverMultistepScheduler (DPM-Solver++ 2M through eegldm_sample_multistep: the same loop with one
    eegldm_multistep_step launch behind every forward).  info (optional dict) receives {"graph": bool}.
    A UNet built with num_classes needs `labels` (one class per sample, or one for all).  guidance_scale w != 1 is classifier-free
    guidance: out = out(null_class) + w (out(labels) - out(null_class)) on the raw model output, every forward on 2B rows."""
    unet.eval()
    x = noise.to(unet.device, torch.float32).contiguous()
    B, Cc, L = x.shape
    if Cc != unet.in_channels:
        raise ValueError(f"noise has {Cc} channels, the UNet takes {unet.in_channels}")
    lab, nc = _labels_host(unet, labels, B, guidance_scale, null_class)
    multistep = isinstance(scheduler, DPMSolverMultistepScheduler)
    if multistep:
        ts, a_t, cx, c0, c1 = _multistep_tables(scheduler)
    else:
        ts, a_t, a_prev, beta, ancestral = _step_tables(scheduler)
    n = len(ts)
    if use_graph is None:
        use_graph = os.environ.get("EEGLDM_SAMPLE_GRAPH", "0") == "1" and os.environ.get("EEGLDM_NO_GRAPH") is None
    down = autoencoder.down if autoencoder is not None else 1
    out_c = autoencoder.out_channels if autoencoder is not None else Cc
    lat = torch.empty_like(x)
    win = torch.empty(B, out_c, L * down, device=unet.device, dtype=torch.float32)
    if B == 0:
        return (win[:, :, crop:-crop] if crop else win), lat
    used = C.c_int(0)
    ae_h = autoencoder.h if autoencoder is not None else None
    i64, f32 = (lambda v: (C.c_int64 * len(v))(*v)), (lambda v: (C.c_float * len(v))(*v))
    tail = (ptr(lat), ptr(win), B, L, 1 if use_graph else 0, C.byref(used))
    if multistep:
        check(lib.eegldm_sample_multistep(unet.h, ae_h, ptr(x), i64(ts), f32(a_t), f32(cx), f32(c0), f32(c1), n, PRED[scheduler.prediction_type],
                                          int(scheduler.clip_sample), 1.0 / float(scale_factor), *tail, None if lab is None else i64(lab),
                                          float(guidance_scale), nc))
    else:
        args = (unet.h, ae_h, ptr(x), i64(ts), f32(a_t), f32(a_prev), f32(beta), n, 1 if ancestral else 0, PRED[scheduler.prediction_type],
                int(scheduler.clip_sample), 1.0 / float(scale_factor), int(seed), *tail)
        if lab is None:
            check(lib.eegldm_sample(*args))
        else:
            check(lib.eegldm_sample_cond(*args, i64(lab), float(guidance_scale), nc))
    unet._bump_tape()
    if autoencoder is not None:
        autoencoder._bump_tape()
    if info is not None:
        info["graph"] = bool(used.value)
    return (win[:, :, crop:-crop] if crop else win), lat


sample = ddim_sample      # the neutral name: the sampler is whatever `scheduler` is


@torch.no_grad()
def ddim_sample_hostloop(unet, autoencoder, scheduler, noise, scale_factor=1.0, crop=36, labels=None, guidance_scale=1.0, null_class=None):
    """The same loop driven from Python, one scheduler.step call per timestep (what round 1 shipped; kept as the
    reference composition the native sampler is tested against, and for schedulers the native loop does not know).
    Class-conditional: the UNet is called with the labels and, for guidance_scale != 1, a second time with null_class; the two
    outputs are mixed as out_u + w (out_c - out_u) ahead of scheduler.step."""
    unet.eval()
    x = noise.to(unet.device, torch.float32).contiguous()
    B = x.shape[0]
    lab, nc = _labels_host(unet, labels, B, guidance_scale, null_class)
    kw = {} if lab is None else {"y": torch.tensor(lab, dtype=torch.int64, device=unet.device)}
    null = None if lab is None else torch.full((B,), nc, dtype=torch.int64, device=unet.device)
    w = float(guidance_scale)
    tt = torch.empty(B, device=unet.device, dtype=torch.int64)
    for t in scheduler.timesteps:
        tt.fill_(int(t))
        out = unet(x, timesteps=tt, **kw)
        if lab is not None and w != 1.0:
            out_u = unet(x, timesteps=tt, y=null)
            out = out_u + w * (out - out_u)
        x, _ = scheduler.step(out, int(t), x)
    if autoencoder is None:      # pixel-space model (sample_trials_ddpm.py:99-104): the UNet output IS the window
        return (x[:, :, crop:-crop] if crop else x), x
    z = x
    if float(scale_factor) != 1.0:
        z = x.clone()
        check(lib.eegldm_axpy(unet.ctx.h, ptr(z), ptr(z), 1.0 / float(scale_factor) - 1.0, z.numel()))
    sample = autoencoder.decode_stage_2_outputs(z)
    return (sample[:, :, crop:-crop] if crop else sample), x


def make_sampling_scheduler(num_inference_steps=50, prediction_type="epsilon", beta_start=0.0015, beta_end=0.0205, device=0, sampler="ddim",
                            solver_order=2):
    """DDIMScheduler as built at sample_trials.py:136-145 (scaled-linear betas, clip_sample=False).  The reference
    script passes prediction_type="v_prediction" while training with epsilon: it is a parameter here.
    sampler="dpmpp_2m": DPMSolverMultistepScheduler on the same schedule (linspace grid, solver_order 2 unless given)."""
    if sampler == "dpmpp_2m":
        s = DPMSolverMultistepScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=beta_start, beta_end=beta_end,
                                        prediction_type=prediction_type, clip_sample=False, solver_order=solver_order, device=device)
        s.set_timesteps(num_inference_steps)
        return s
    if sampler != "ddim":
        raise ValueError('sampler must be "ddim" or "dpmpp_2m"')
    s = DDIMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=beta_start, beta_end=beta_end,
                      prediction_type=prediction_type, clip_sample=False, device=device)
    s.set_timesteps(num_inference_steps)
    return s


def sample_seeds(unet, autoencoder, scheduler, seeds, latent_len=768, scale_factor=1.0, crop=36, labels=None, guidance_scale=1.0, null_class=None):
    """One window per seed (sample_trials.py:149-151 draws a fresh N(0,1) latent per seed), batched.
    autoencoder=None samples a pixel-space model: latent_len is then the window length (3072).  labels / guidance_scale / null_class:
    class-conditional sampling (ddim_sample)."""
    lat = unet.in_channels
    noise = torch.empty(len(seeds), lat, latent_len, device=unet.device)
    for i, sd in enumerate(seeds):
        noise[i] = randn(unet.ctx, (lat, latent_len), seed=int(sd))
    return ddim_sample(unet, autoencoder, scheduler, noise, scale_factor, crop, labels=labels, guidance_scale=guidance_scale, null_class=null_class)
