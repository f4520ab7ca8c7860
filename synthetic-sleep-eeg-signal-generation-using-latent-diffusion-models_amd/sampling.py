"""DDIM sampling of 30-s EEG windows: the loop of the reference's src/sample_trials.py:149-170
(noise -> UNet/DDIM steps -> decode(z / scale_factor) -> crop [36:-36]), batched over seeds instead of
one window at a time (the reference runs batch 1, which is launch-bound), with the step count a real
parameter (the reference hard-codes 200, sample_trials.py:144)."""
import ctypes as C
import os

import numpy as np
import torch

from ._lib import lib, check, ptr, PRED, SampleDesc
from .schedulers import DDIMScheduler, DPMSolverMultistepScheduler, RESAMPLE_KEY, scheduler_edit_tables, scheduler_resample_tables
from .training import context_window, randn


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


def _fma32(a, b, c):
    """float32 fma(a, b, c) on tensors (a may be a Python float holding a float32 value): the product of two float32 is exact in
    float64, the sum is rounded there and once more to float32."""
    a = a.double() if torch.is_tensor(a) else float(a)
    return (a * b.double() + c.double()).float()


def _renoise(z0, noise, a):
    """k(a) = fma(sqrt(a), z0, sqrt(1 - a) * noise) with the library's roundings (eegldm_edit_start: the product, then a fused
    multiply-add), a == 1: z0 itself.  A bfloat16 UNet turns a last-bit difference of its input into a bfloat16 ulp."""
    a32 = np.float32(a)          # (numpy's float32 sqrt is correctly rounded, as the library's sqrtf; torch's scalar sqrt is not always)
    if a32 >= 1.0:
        return z0
    ka, kb = float(np.sqrt(a32)), float(np.sqrt(np.float32(1.0) - a32))
    return _fma32(ka, z0, noise * kb)


# how the messages of a run from an input name its arguments: windows (ddim_sample) and recordings (sample_long)
_EDIT_WORDS = dict(latents="init_latents", both="init (windows) or init_latents", composite="init (windows)")
_LONG_EDIT_WORDS = dict(latents="init_canvas", both="init (the recording) or init_canvas (latents)",
                        composite="init (the recording at window resolution)")


def _edit_args(autoencoder, scheduler, shape, init, strength, mask, composite, latents, words=_EDIT_WORDS, mask_erode=0):
    """Checks the arguments of a run that starts from an input, on the host and before anything runs; -> None without init / latents,
    else dict(tab = the truncated tables, composite = bool).  shape = (B, C, L) of the latents the run works on -- windows, or the (R, C, Lc)
    canvases of a long recording; init (B, in_channels, L * down) at window resolution for an LDM, (B, C, L) for a pixel-space model;
    latents (init_latents / init_canvas, named by `words`) (B, C, L); mask (B, 1, L * down), 1 = keep."""
    from .schedulers import edit_start_index
    edit_start_index(1, strength)           # the range of strength, whatever else is given
    if int(mask_erode) != mask_erode or mask_erode < 0:
        raise ValueError(f"mask_erode must be an integer >= 0 (got {mask_erode})")
    name = words["latents"]
    if init is None and latents is None:
        if mask is not None:
            raise ValueError(f"mask needs init (or {name}): the kept samples have to come from somewhere")
        if composite:
            raise ValueError("composite needs init and mask")
        if float(strength) != 1.0:
            raise ValueError(f"strength needs init (or {name})")
        return None
    if init is not None and latents is not None:
        raise ValueError(f"pass {words['both']}, not both")
    tab = scheduler_edit_tables(scheduler, strength)        # (refuses the ancestral scheduler)
    B, Cc, L = (int(v) for v in shape)
    down = autoencoder.down if autoencoder is not None else 1
    if init is not None:
        want = (B, autoencoder.in_channels, L * down) if autoencoder is not None else (B, Cc, L)
        if tuple(init.shape) != want:
            raise ValueError(f"init has shape {tuple(init.shape)}, expected {want}")
        if autoencoder is not None and autoencoder.in_channels != autoencoder.out_channels and mask is not None and composite is not False:
            raise ValueError("the composite needs an autoencoder with in_channels == out_channels")
    elif tuple(latents.shape) != (B, Cc, L):
        raise ValueError(f"{name} has shape {tuple(latents.shape)}, expected {(B, Cc, L)}")
    if mask is not None and tuple(mask.shape) != (B, 1, L * down):
        raise ValueError(f"mask has shape {tuple(mask.shape)}, expected {(B, 1, L * down)}")
    if composite and (mask is None or init is None):
        raise ValueError(f"composite needs mask and {words['composite']}")
    return dict(tab=tab, composite=(mask is not None and init is not None) if composite is None else bool(composite))


def _resample_args(scheduler, edit, mask, resamples, jump_length):
    """Checks resamples / jump_length on the host, before anything runs -> None for resamples == 1 (the calls made without the keywords),
    else the tables of schedulers.resample_tables, one entry per forward."""
    if int(resamples) != resamples or int(jump_length) != jump_length or resamples < 1 or jump_length < 1:
        raise ValueError(f"resamples and jump_length must be integers >= 1 (got {resamples}, {jump_length})")
    if resamples == 1:
        return None
    if edit is None or mask is None:
        raise ValueError("resamples > 1 needs init (or latents) and mask: resampling reconciles a regenerated span with a kept one")
    return scheduler_resample_tables(scheduler, edit["tab"], resamples, jump_length)


def _blend(mk, k, p):
    """m == 0: p, m == 1: k, else fma(m, k, (1 - m) * p) -- the library's edit_blend"""
    return torch.where(mk == 0, p, torch.where(mk == 1, k, _fma32(mk, k, (1.0 - mk) * p)))


def _jump(ctx, x, z0, nz, m_lat, rt, i, jump_index, seed):
    """The jump in front of forward i of a resampled run, composed in torch with the library's roundings: eps from the Philox stream
    RESAMPLE_KEY + seed at offset jump_index * ceil(n / 4), p = fma(jump_x, x, jump_n * eps), then the blend towards k(a_t[i])."""
    eps = randn(ctx, tuple(x.shape), RESAMPLE_KEY + int(seed), jump_index * ((x.numel() + 3) // 4))
    p = _fma32(rt["jump_x"][i], x, eps * rt["jump_n"][i])
    return _blend(m_lat, _renoise(z0, nz, rt["a_t"][i]), p)


def _encode_windows(unet, autoencoder, init_d, scale_factor, native):
    """scale_factor * the posterior mean of the encoded windows (no reparameterisation draw)"""
    z_mu, _sigma = autoencoder.encode(init_d)
    if not native:
        return z_mu * float(scale_factor)
    z0 = torch.empty_like(z_mu)
    check(lib.eegldm_edit_start(unet.ctx.h, ptr(z_mu), float(scale_factor), None, 1.0, ptr(z0), None, z0.numel()))
    return z0


def _edit_inputs(unet, autoencoder, x, init, mask, latents, encode, mask_erode=0, native=True):
    """-> (z0 (B, C, L), the mask as given on the device or None, the keep-mask at the sampler's resolution or None, init on the device or
    None), x (B, C, L) being the latents of the run: windows, or the canvases of a long recording.  encode(init on the device, native) -> z0
    for an LDM (_encode_windows / encode_long).  The keep-mask is the min-pool over the mask eroded by mask_erode samples: latent position p
    is kept only if all the samples [p down, (p + 1) down) are.  native: it comes from eegldm_edit_window; else from torch ops (the host
    loops' reference composition)."""
    dev = unet.device
    B, Cc, L = x.shape
    down = autoencoder.down if autoencoder is not None else 1
    init_d = None if init is None else torch.as_tensor(init).to(dev, torch.float32).contiguous()
    if latents is not None:
        z0 = torch.as_tensor(latents).to(dev, torch.float32).contiguous()
    elif autoencoder is None:
        z0 = init_d
    else:
        z0 = encode(init_d, native)
    m_win = m_lat = None
    if mask is not None:
        m_win = torch.as_tensor(mask).to(dev, torch.float32).contiguous()
        if not bool(((m_win >= 0) & (m_win <= 1)).all()):
            raise ValueError("mask values must lie in [0, 1]")
        m_er = erode_mask(m_win, mask_erode).contiguous()
        if native:
            m_lat = torch.empty(B, Cc, L, device=dev, dtype=torch.float32)
            check(lib.eegldm_edit_window(unet.ctx.h, ptr(m_er), B, L * down, down, Cc, ptr(m_lat), None, None, 0, None))
        else:
            m_lat = (-torch.nn.functional.max_pool1d(-m_er, down, down)).expand(B, Cc, L).contiguous()
    return z0, m_win, m_lat, init_d


def _context_args(unet, context, blend, resamples, rows, L):
    """Host-side checks of the context keywords, behind those of the other arguments and before anything runs -> is `unet` a context
    model.  context: (rows', context_channels, L) with rows % rows' == 0 -- for a long recording canvas-shaped, one row per recording."""
    cc = getattr(unet, "context_channels", 0)
    if not cc:
        if context is not None:
            raise ValueError("context needs a UNetModel built with context_channels")
        if not blend:
            raise ValueError("blend=False needs a context model: without the blend nothing but the start ties the result to the input")
        return False
    if not blend and resamples != 1:
        raise ValueError("resamples > 1 needs blend=True: resampling reconciles the regenerated span with the replaced one")
    if context is not None:
        shape = tuple(context.shape) if torch.is_tensor(context) else None
        if shape is None or len(shape) != 3 or shape[1:] != (cc, int(L)) or shape[0] < 1 or rows % shape[0] != 0:
            raise ValueError(f"context has shape {shape}, expected (rows, {cc}, {int(L)}) with rows dividing {rows}")
    return True


def _form_context(unet, autoencoder, x, context, z0, m_lat, init_d, encode, native=True):
    """The context of a run on a context model -> (rows, C + 1, L) on the device, or None (the model then reads zeros: plain generation).
    As in training: with the keep-mask m at the sampler's resolution (the min-pooled mask) the context is [m * src | m], src being the
    encoding of the MASKED input -- scale_factor * encode_mean(init * upsample(m)), so that no latent carries what the encoder saw inside
    the span to regenerate -- or, for latents given directly and for a pixel-space model, the input itself."""
    dev = unet.device
    if context is not None:
        return context.detach().to(dev, torch.float32).contiguous()
    if m_lat is None:
        return None
    B, Cc, L = x.shape
    if unet.context_channels != Cc + 1:
        raise ValueError(f"the context of a repair has {Cc} + 1 channels (masked signal, mask), the model takes {unet.context_channels}")
    m1 = m_lat[:, :1, :].contiguous()
    if init_d is not None and autoencoder is not None:
        down = autoencoder.down
        masked = context_window(unet.ctx, init_d, m1[:, 0], down) if native else init_d * m1.repeat_interleave(down, dim=2)
        src = encode(masked, native)
    else:
        src = z0
    return torch.cat([m1 * src, m1], 1).contiguous()


# the host arrays of a call, under the names its tables and the descriptor share
_DESC_TABLES = ("a_t", "a_prev", "beta_t", "cx", "c0", "c1", "a_next", "jump_x", "jump_n")


def _run_loop(unet, autoencoder, scheduler, x, tab, lab, guidance_scale, null_class, scale_factor, use_graph, seed, info, ancestral=False,
              known=None, mask=None, blend=True, strength=1.0, context=None, context_rows=0, **own):
    """ONE call of the native loop (eegldm_sample_run) from the start noise x.  What ddim_sample and sample_long share is set here, by
    member name: the schedule (tab: host lists keyed like the descriptor -- timesteps, a_t, then whichever of a_prev / beta_t / cx / c0 /
    c1 / a_next / jump_x / jump_n the form has; the library selects the step by what is there), classes, the edit start and blend
    (known is dropped when only the learned conditioning is asked for -- blend=False at full strength -- and the mask with it), jumps
    (key RESAMPLE_KEY + seed; `seed` itself is the ancestral step's key, the two never meet), the context and the graph switch.  own:
    the caller's members -- shape and outputs.  Tensors are passed as addresses and stay alive as this function's arguments; host arrays
    are assigned to the descriptor, which keeps them.  info (optional dict) receives {"graph", "forwards"}."""
    if use_graph is None:
        use_graph = os.environ.get("EEGLDM_SAMPLE_GRAPH", "0") == "1" and os.environ.get("EEGLDM_NO_GRAPH") is None
    if known is not None and not (blend or float(strength) != 1.0):
        known = None
    if known is None or not blend:
        mask = None
    n = len(tab["timesteps"])
    used = C.c_int(0)
    d = SampleDesc(size=C.sizeof(SampleDesc), unet=unet.h, ae=autoencoder.h if autoencoder is not None else None, noise=x.data_ptr(),
                   n_steps=n, timesteps=(C.c_int64 * n)(*tab["timesteps"]), ancestral=1 if ancestral else 0,
                   noise_seed=RESAMPLE_KEY + int(seed) if "jump_x" in tab else int(seed),
                   pred_type=PRED[scheduler.prediction_type], clip_sample=int(scheduler.clip_sample), inv_scale_factor=1.0 / float(scale_factor),
                   guidance_scale=float(guidance_scale), null_class=null_class,
                   known=None if known is None else known.data_ptr(), mask=None if mask is None else mask.data_ptr(),
                   context=None if context is None else context.data_ptr(), context_rows=context_rows,
                   use_graph=1 if use_graph else 0, graph_used=C.pointer(used), **own)
    for k in _DESC_TABLES:
        if k in tab:
            setattr(d, k, (C.c_float * n)(*tab[k]))
    if lab is not None:
        d.labels = (C.c_int64 * len(lab))(*lab)
    check(lib.eegldm_sample_run(C.byref(d)))
    unet._bump_tape()
    if autoencoder is not None:
        autoencoder._bump_tape()
    if info is not None:
        info["graph"], info["forwards"] = bool(used.value), n


@torch.no_grad()
def ddim_sample(unet, autoencoder, scheduler, noise, scale_factor=1.0, crop=36, use_graph=None, seed=0, info=None, labels=None,
                guidance_scale=1.0, null_class=None, init=None, strength=1.0, mask=None, composite=None, init_latents=None, resamples=1,
                jump_length=1, context=None, blend=True):
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
    guidance: out = out(null_class) + w (out(labels) - out(null_class)) on the raw model output, every forward on 2B rows.
    init (windows; init_latents for callers who hold latents) starts the run from an input instead of from noise (eegldm_sample_edit): with
    z0 = scale_factor * posterior mean of the encoded window (pixel-space model: the window itself) the last n_run = min(n, max(1,
    round(strength * n))) steps of the grid run from x = sqrt(a_t) z0 + sqrt(1 - a_t) noise; `noise` is the one noise tensor of the call,
    nothing else is drawn.  mask ((B, 1, window length), 1 = keep) regenerates only the samples marked 0: after every step the kept region
    is reset to z0 noised to that step's level (inside the step's kernel); a latent position is kept only if all the window samples it
    covers are.  composite (default: on with mask and init) returns mask * init + (1 - mask) * decoded windows, kept samples bit for bit.
    The ancestral DDPMScheduler, mask without init and strength outside (0, 1] are refused.
    resamples = r > 1 (needs init and mask) is RePaint's resampling (eegldm_sample_edit_resample): at the levels l in range(0, n_run - j, j)
    (l = steps still to run, j = jump_length) the run goes back up j levels in one jump, x <- sqrt(rho) x + sqrt(1 - rho) eps with FRESH
    noise drawn inside the jump's kernel (Philox key schedulers.RESAMPLE_KEY + seed; the kept part stays k(a) of the call's one noise
    tensor), and comes down again, r - 1 times per level: n_run + (r - 1) j len(range(0, n_run - j, j)) forwards in all, which is the cost.
    The step behind a jump is first order.  jump_length = 1 is a convention; no (resamples, jump_length) has been measured on sleep data.
    info also receives {"forwards": the number of forwards}.
    A UNetModel built with context_channels (learned repair, eegldm_sample_edit_ctx): with init and mask the context is formed as in
    training -- [m * src | m] with m the min-pooled mask and src = scale_factor * encode_mean(init * upsample(m)), the encoding of the
    MASKED window (init_latents and pixel-space models: the input itself) -- and every forward reads it, at one forward per step.
    blend=True (default) keeps the replacement blend as well, so kept latents still end as z0 and kept samples stay the input's bytes;
    blend=False uses the learned conditioning alone (the run then starts from noise unless strength < 1, and composite defaults to off).
    context= passes a (rows, context_channels, L) tensor directly (rows dividing B).  With neither init / mask nor context the context is
    zero: plain generation.  Whether such a model repairs EEG more plausibly than replacement is not measured here."""
    if composite is None and not blend:
        composite = False                      # the learned conditioning alone: nothing is pasted back unless asked for
    edit = _edit_args(autoencoder, scheduler, noise.shape, init, strength, mask, composite, init_latents)
    rt = _resample_args(scheduler, edit, mask, resamples, jump_length)
    ctx_model = _context_args(unet, context, blend, resamples, int(noise.shape[0]), int(noise.shape[2]))
    if edit is None and context is not None:
        edit = dict(tab=scheduler_edit_tables(scheduler, 1.0), composite=False)      # the edit loop with nothing known: a context and noise
    unet.eval()
    x = noise.to(unet.device, torch.float32).contiguous()
    B, Cc, L = x.shape
    if Cc != getattr(unet, "x_channels", unet.in_channels):
        raise ValueError(f"noise has {Cc} channels, the UNet takes {getattr(unet, 'x_channels', unet.in_channels)}")
    lab, nc = _labels_host(unet, labels, B, guidance_scale, null_class)
    ancestral = False
    if edit is not None:
        tab = edit["tab"] if rt is None else rt
    elif isinstance(scheduler, DPMSolverMultistepScheduler):
        tab = dict(zip(("timesteps", "a_t", "cx", "c0", "c1"), _multistep_tables(scheduler)))
    else:
        ts, a_t, a_prev, beta, ancestral = _step_tables(scheduler)
        tab = dict(timesteps=ts, a_t=a_t, a_prev=a_prev, beta_t=beta)
    down = autoencoder.down if autoencoder is not None else 1
    out_c = autoencoder.out_channels if autoencoder is not None else Cc
    lat = torch.empty_like(x)
    win = torch.empty(B, out_c, L * down, device=unet.device, dtype=torch.float32)
    if B == 0:
        return (win[:, :, crop:-crop] if crop else win), lat
    z0 = m_win = m_lat = init_d = cx_t = None
    if edit is not None:
        encode = lambda w, native: _encode_windows(unet, autoencoder, w, scale_factor, native)
        if init is not None or init_latents is not None:
            z0, m_win, m_lat, init_d = _edit_inputs(unet, autoencoder, x, init, mask, init_latents, encode)
        if ctx_model:
            cx_t = _form_context(unet, autoencoder, x, context, z0, m_lat, init_d, encode)
    _run_loop(unet, autoencoder, scheduler, x, tab, lab, guidance_scale, nc, scale_factor, use_graph, seed, info, ancestral=ancestral,
              known=z0, mask=m_lat, blend=blend, strength=strength, context=cx_t, context_rows=0 if cx_t is None else cx_t.shape[0],
              B=B, L=L, latents_out=lat.data_ptr(), windows_out=win.data_ptr())
    if edit is not None and edit["composite"]:
        check(lib.eegldm_edit_window(unet.ctx.h, ptr(m_win), B, L * down, down, 0, None, ptr(init_d), ptr(win), out_c, ptr(win)))
    return (win[:, :, crop:-crop] if crop else win), lat


sample = ddim_sample      # the neutral name: the sampler is whatever `scheduler` is


@torch.no_grad()
def ddim_sample_hostloop(unet, autoencoder, scheduler, noise, scale_factor=1.0, crop=36, labels=None, guidance_scale=1.0, null_class=None,
                         init=None, strength=1.0, mask=None, composite=None, init_latents=None, resamples=1, jump_length=1, seed=0,
                         context=None, blend=True):
    """The same loop driven from Python, one scheduler.step call per timestep (what round 1 shipped; kept as the
    reference composition the native sampler is tested against, and for schedulers the native loop does not know).
    Class-conditional: the UNet is called with the labels and, for guidance_scale != 1, a second time with null_class; the two
    outputs are mixed as out_u + w (out_c - out_u) ahead of scheduler.step.  init / strength / mask / composite / init_latents as in
    ddim_sample, composed from torch ops: the noised start, the blend m k + (1 - m) x after every scheduler.step, the min-pooled mask and
    the composite.  resamples / jump_length / seed as in ddim_sample: the loop runs over the entries of schedulers.resample_tables; in front
    of a forward with a jump it draws eps = training.randn(...) and forms the jump and its blend in torch (_jump), and the multistep
    scheduler takes the step behind a jump with first_order=True.  context / blend as in ddim_sample: the reference composition of the
    learned repair is model(x, timesteps=t, context=c) per step, the context formed from torch ops."""
    if composite is None and not blend:
        composite = False                      # the learned conditioning alone: nothing is pasted back unless asked for
    edit = _edit_args(autoencoder, scheduler, noise.shape, init, strength, mask, composite, init_latents)
    rt = _resample_args(scheduler, edit, mask, resamples, jump_length)
    ctx_model = _context_args(unet, context, blend, resamples, int(noise.shape[0]), int(noise.shape[2]))
    if edit is None and context is not None:
        edit = dict(tab=scheduler_edit_tables(scheduler, 1.0), composite=False)
    unet.eval()
    x = noise.to(unet.device, torch.float32).contiguous()
    B = x.shape[0]
    lab, nc = _labels_host(unet, labels, B, guidance_scale, null_class)
    kw = {} if lab is None else {"y": torch.tensor(lab, dtype=torch.int64, device=unet.device)}
    null = None if lab is None else torch.full((B,), nc, dtype=torch.int64, device=unet.device)
    w = float(guidance_scale)
    tt = torch.empty(B, device=unet.device, dtype=torch.int64)
    timesteps, first = scheduler.timesteps, {}
    if edit is not None:
        tab = edit["tab"]
        nz = x
        z0 = m_win = m_lat = init_d = None
        encode = lambda w, native: _encode_windows(unet, autoencoder, w, scale_factor, native)
        if init is not None or init_latents is not None:
            z0, m_win, m_lat, init_d = _edit_inputs(unet, autoencoder, x, init, mask, init_latents, encode, native=False)
        if ctx_model:
            cx_t = _form_context(unet, autoencoder, x, context, z0, m_lat, init_d, encode, native=False)
            if cx_t is not None:
                kw["context"] = cx_t
            if not blend:
                m_lat = None
                if float(strength) == 1.0:
                    z0 = None
        if z0 is not None:
            x = _renoise(z0, nz, tab["a_t"][0])
        timesteps = tab["timesteps"]
        if isinstance(scheduler, DPMSolverMultistepScheduler):
            first = {"first_order": True}
        if rt is not None:
            tab, timesteps = rt, rt["timesteps"]
    jumps = 0
    for j, t in enumerate(timesteps):
        jumped = rt is not None and rt["jump_n"][j] != 0.0
        if jumped:
            x = _jump(unet.ctx, x, z0, nz, m_lat, rt, j, jumps, seed)
            jumps += 1
        tt.fill_(int(t))
        out = unet(x, timesteps=tt, **kw)
        if lab is not None and w != 1.0:
            out_u = unet(x, timesteps=tt, **dict(kw, y=null))
            out = out_u + w * (out - out_u)
        x, _ = scheduler.step(out, int(t), x, **(first if j == 0 or jumped else {}))
        if edit is not None and m_lat is not None:
            x = m_lat * _renoise(z0, nz, tab["a_next"][j]) + (1.0 - m_lat) * x
    comp = (lambda win: m_win * init_d + (1.0 - m_win) * win) if edit is not None and edit["composite"] else (lambda win: win)
    if autoencoder is None:      # pixel-space model (sample_trials_ddpm.py:99-104): the UNet output IS the window
        sample = comp(x)
        return (sample[:, :, crop:-crop] if crop else sample), x
    z = x
    if float(scale_factor) != 1.0:
        z = x.clone()
        alpha = 1.0 / float(scale_factor) - 1.0
        if edit is not None:
            # the native loop's value: 1 / scale_factor rounded to float32, then minus one in float32.  The double expression above can
            # differ from it in the last bit, which a bfloat16 decoder turns into a bfloat16 ulp of a window sample now and then
            alpha = float(np.float32(1.0 / float(scale_factor)) - np.float32(1.0))
        check(lib.eegldm_axpy(unet.ctx.h, ptr(z), ptr(z), alpha, z.numel()))
    sample = comp(autoencoder.decode_stage_2_outputs(z))
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
    lat = getattr(unet, "x_channels", unet.in_channels)      # (a context model samples from zero context here: plain generation)
    noise = torch.empty(len(seeds), lat, latent_len, device=unet.device)
    for i, sd in enumerate(seeds):
        noise[i] = randn(unet.ctx, (lat, latent_len), seed=int(sd))
    return ddim_sample(unet, autoencoder, scheduler, noise, scale_factor, crop, labels=labels, guidance_scale=guidance_scale, null_class=null_class)


# ------------------------------------------------------------------ long recordings: overlapped windows on one latent canvas
class LongLayout:
    """Where the W windows of one recording sit on its canvas and what each contributes (include/eegldm.h has the same text): window k
    covers canvas positions [k S, k S + L), S = L - (2 m + r), Lc = (W - 1) S + L.  Host-side integers and float64 / float32 arrays."""

    def __init__(self, n_windows, window_len, margin, ramp):
        W, L, m, r = int(n_windows), int(window_len), int(margin), int(ramp)
        if (W, L, m, r) != (n_windows, window_len, margin, ramp):
            raise ValueError("n_windows, window_len, margin and ramp must be integers")
        if W < 1 or m < 0 or r < 0:
            raise ValueError(f"needs n_windows >= 1, margin >= 0 and ramp >= 0 (got {W}, {m}, {r})")
        if L < 1 or L < 3 * m + 2 * r:
            raise ValueError(f"window_len {L} < 3 * margin + 2 * ramp = {3 * m + 2 * r}: more than two windows would carry weight somewhere")
        self.n_windows, self.window_len, self.margin, self.ramp = W, L, m, r
        self.stride = L - (2 * m + r)
        self.canvas_len = (W - 1) * self.stride + L
        self.starts = [k * self.stride for k in range(W)]

    def weights(self, k):
        """float32 array (L,): the weight of window k at each of its positions.  u = (j - m + 0.5) / r is evaluated in float64 and rounded
        once; the falling side is 1 - u in float32, the value the kernels form, so the two weights of a position sum to exactly 1."""
        W, L, S, m, r = self.n_windows, self.window_len, self.stride, self.margin, self.ramp
        if not 0 <= k < W:
            raise IndexError(f"window {k} of {W}")
        w = np.ones(L, np.float32)
        u = ((np.arange(r, dtype=np.float64) + 0.5) / r).astype(np.float32) if r else np.zeros(0, np.float32)
        if k > 0:
            w[:m] = 0.0
            w[m:m + r] = u
        if k < W - 1:                                  # the next window's rising side, seen from this one: j = S + j'
            w[S + m:S + m + r] = np.float32(1.0) - u
            w[S + m + r:] = 0.0
        return w

    def scaled(self, down):
        """The same layout at window resolution: m, r, S, L times the autoencoder's downsampling factor."""
        d = int(down)
        if d < 1:
            raise ValueError("down must be >= 1")
        return LongLayout(self.n_windows, self.window_len * d, self.margin * d, self.ramp * d)

    def seams(self):
        """[(first, stop)] canvas spans of the W - 1 ramps (empty spans when ramp == 0: the hard switch sits at `first`)."""
        return [(k * self.stride + self.margin, k * self.stride + self.margin + self.ramp) for k in range(1, self.n_windows)]

    def owner(self):
        """(k1, j) int arrays (Lc,): the last window whose leading margin position p has left, and p's index inside it."""
        p = np.arange(self.canvas_len)
        k1 = np.where(p < self.stride + self.margin, 0, np.minimum(self.n_windows - 1, (p - self.margin) // self.stride))
        return k1, p - k1 * self.stride


def long_layout(n_windows, window_len, margin, ramp):
    return LongLayout(n_windows, window_len, margin, ramp)


def window_labels_from_hypnogram(stages, layout, down=1, sfreq=100.0, epoch_seconds=30.0):
    """One class per window from a hypnogram (one stage per epoch): window k takes the stage at its centre time
    (k S + L / 2) * down / sfreq seconds; a centre past the last epoch is an error."""
    stages = np.asarray(stages).reshape(-1)
    out = []
    for k in range(layout.n_windows):
        t = (k * layout.stride + layout.window_len / 2.0) * down / float(sfreq)
        e = int(t // float(epoch_seconds))
        if e >= len(stages):
            raise ValueError(f"window {k} is centred at {t:.2f} s: the hypnogram has {len(stages)} epochs of {epoch_seconds} s")
        out.append(int(stages[e]))
    return np.asarray(out, np.int64)


def _long_args(unet, autoencoder, scheduler, noise_shape, n_windows, margin, ramp, crop, labels):
    """Host-side checks of a long-recording call, before anything touches the model or the device -> (layout, R, labels or None as
    given, expanded to R * W)."""
    if not isinstance(scheduler, DPMSolverMultistepScheduler):
        raise ValueError("sample_long needs a DPMSolverMultistepScheduler (solver_order=1 is DDIM on the same grid)")
    if len(noise_shape) != 3:
        raise ValueError(f"noise has shape {tuple(noise_shape)}, expected (R, C, canvas length)")
    R, Cc, Lc = (int(v) for v in noise_shape)
    W = int(n_windows)
    if W < 1:
        raise ValueError("n_windows must be >= 1")
    down = autoencoder.down if autoencoder is not None else 1
    if margin is None:
        margin = 2 * int(crop) // down
    if ramp is None:
        ramp = 4 * int(crop) // down
    m, r = int(margin), int(ramp)
    if m < 0 or r < 0:
        raise ValueError("margin and ramp must be >= 0")
    if W == 1:
        L = Lc
    else:
        S, rem = divmod(Lc - (2 * m + r), W)           # Lc = (W - 1) S + L = W S + 2 m + r
        if rem or S < 1:
            raise ValueError(f"noise has length {Lc}: no window length gives {W} windows with margin {m} and ramp {r} "
                             f"(needs (W - 1) * (L - {2 * m + r}) + L)")
        L = S + 2 * m + r
    lay = LongLayout(W, L, m, r)
    if lay.canvas_len != Lc or R < 1:
        raise ValueError(f"noise has shape {tuple(noise_shape)}, expected (R >= 1, C, {lay.canvas_len})")
    if labels is not None:
        lab = torch.as_tensor(labels).reshape(-1)
        if lab.numel() == W:
            lab = lab.repeat(R)
        if lab.numel() != R * W:
            raise ValueError(f"{lab.numel()} labels for {R} recordings of {W} windows: pass R * W (recording-major) or W")
        labels = lab
    return lay, R, labels


def erode_mask(mask, erode):
    """mask (R, 1, n), 1 = keep -> the mask with every kept region shrunk by `erode` samples on each side that borders a regenerated span:
    out[t] = min(mask[t - erode .. t + erode]); samples past a free end of the recording do not count as regenerated.  Host-side torch
    work, once per call."""
    e = int(erode)
    if e != erode or e < 0:
        raise ValueError(f"mask_erode must be an integer >= 0 (got {erode})")
    m = torch.as_tensor(mask)
    if e == 0:
        return m
    return -torch.nn.functional.max_pool1d(-m.to(torch.float32), 2 * e + 1, 1, e)        # (max_pool1d pads with -inf: +inf for the min)


def _slices_of(cv, lay):
    """(R, C, Lc) -> (R * W, C, L) by torch slicing"""
    R, Cc, _ = cv.shape
    S, L = lay.stride, lay.window_len
    return torch.stack([cv[:, :, k * S:k * S + L] for k in range(lay.n_windows)], 1).reshape(R * lay.n_windows, Cc, L)


@torch.no_grad()
def encode_long(autoencoder, recording, layout, scale_factor=1.0, native=True):
    """recording (R, in_channels, down * Lc) at window resolution -- the `crop` zero samples at its two free ends included, as a training
    window holds them -- -> z0 (R, C, Lc), the clean latent canvas of `layout` (the LATENT LongLayout).  Composed from existing exports:
    eegldm_canvas_gather at window resolution, the posterior mean of the R * W windows (each encoded as its own row, so the encoder's
    GroupNorm statistics span one 30-s window as in training; no reparameterisation draw), eegldm_edit_start for the scale, and
    eegldm_canvas_compose with the latent layout: the owner window's latent outside the ramps, the cross-fade of the two inside.  A
    zero-weight margin thereby discards exactly the latents that were encoded next to a window edge.  native=False: the same composition
    in torch ops (the host loop's reference)."""
    lay, down = layout, autoencoder.down
    W, L, S = lay.n_windows, lay.window_len, lay.stride
    rec = torch.as_tensor(recording).to(autoencoder.device, torch.float32).contiguous()
    if rec.dim() != 3 or tuple(rec.shape[1:]) != (autoencoder.in_channels, lay.canvas_len * down):
        raise ValueError(f"recording has shape {tuple(rec.shape)}, expected (R, {autoencoder.in_channels}, {lay.canvas_len * down})")
    R, Ci = rec.shape[0], rec.shape[1]
    big = lay.scaled(down)
    if not native:
        z_mu, _sigma = autoencoder.encode(_slices_of(rec, big).contiguous())
        rows = z_mu * float(scale_factor)
        return _long_crossfade(rows.reshape(R, W, rows.shape[1], L), lay)
    h = autoencoder.ctx.h
    win = torch.empty(R * W, Ci, L * down, device=rec.device, dtype=torch.float32)
    check(lib.eegldm_canvas_gather(h, ptr(rec), R, Ci, W, L * down, S * down, ptr(win), None))
    z_mu, _sigma = autoencoder.encode(win)
    z_mu = z_mu.contiguous()
    rows = torch.empty_like(z_mu)
    check(lib.eegldm_edit_start(h, ptr(z_mu), float(scale_factor), None, 1.0, ptr(rows), None, rows.numel()))
    z0 = torch.empty(R, rows.shape[1], lay.canvas_len, device=rec.device, dtype=torch.float32)
    check(lib.eegldm_canvas_compose(h, ptr(rows), R, rows.shape[1], W, L, S, lay.margin, lay.ramp, ptr(z0)))
    return z0


@torch.no_grad()
def sample_long(unet, autoencoder, scheduler, noise, n_windows, margin=None, ramp=None, scale_factor=1.0, crop=36, labels=None,
                guidance_scale=1.0, null_class=None, use_graph=None, info=None, init=None, init_canvas=None, strength=1.0, mask=None,
                composite=None, mask_erode=0, resamples=1, jump_length=1, seed=0, context=None, blend=True):
    """noise (R, C, Lc) on the device -> (recording (R, out, down * Lc - 2 * crop), canvas (R, C, Lc)).  Overlapped-window sampling on one
    latent canvas (MultiDiffusion): the R * W overlapping slices of the canvases are the rows of ONE forward batch, and behind every
    forward ONE eegldm_canvas_step launch fuses the slices' data predictions with a partition-of-unity taper, takes the solver step on
    the canvas and rewrites the slices.  The whole loop, the window-by-window decode and the cross-fade onto the recording are ONE native
    call (eegldm_sample_long).  The window length follows from the noise: Lc = (W - 1) (L - (2 margin + ramp)) + L.
    `scheduler`: a DPMSolverMultistepScheduler (order 1 or 2).  labels: R * W classes, recording-major (or W, the same for every
    recording); guidance as in `sample`.  margin / ramp (latent positions) default to 2 crop / down and 4 crop / down -- 18 and 36 latents
    for the 3072-sample window, stride 696 latents = 27.84 s: conventions derived from the training crop, NOT tuned against any seam
    measure (tools/seam_report.py is what one tunes them by).  info (optional dict) receives {"graph": bool, "layout": LongLayout}.
    Repairing, varying or continuing a REAL recording (eegldm_sample_long_edit: every step is then ONE eegldm_canvas_edit_step launch, the
    canvas step and the blend).  init ((R, in_channels, down * Lc) for an LDM, (R, C, Lc) for a pixel-space model: the recording at window
    resolution WITH the `crop` zero samples at its two free ends, as a training window holds them; init_canvas (R, C, Lc) for callers who hold latents)
    starts the run from a real recording instead of from noise: z0 = encode_long(...), and the last n_run = min(n, max(1, round(strength *
    n))) steps of the grid run from canvas = sqrt(a_t) z0 + sqrt(1 - a_t) noise (schedulers.edit_tables; the first executed step is first
    order).  `noise` is the one noise tensor of the call; nothing else is drawn.  mask ((R, 1, down * Lc), 1 = keep) regenerates only the
    samples marked 0: after every step the kept canvas positions are reset to z0 noised to the level the step landed on, inside the
    step's kernel; a canvas position is kept only if all `down` samples it covers are.  composite (default: on with mask and init)
    returns mask * init + (1 - mask) * recording, kept samples bit for bit; the crop applies afterwards.  mask_erode = e (window samples):
    the canvas keep-mask is taken from the mask with every kept region shrunk by e samples beside each regenerated span -- the encoder's
    receptive field contaminates the latents next to a regenerated or absent span -- while the composite uses the mask as given.  The
    default is 0; no other default is proposed and NO value has been measured against anything.  Continuing a recording: init = the real
    samples followed by zeros, mask = 1 over the real samples and 0 beyond.
    resamples / jump_length / seed: RePaint's resampling as in `sample` (eegldm_sample_long_edit_resample; needs init and mask): a jump is
    ONE eegldm_edit_jump launch on the canvas, fresh noise from the Philox key schedulers.RESAMPLE_KEY + seed, and a gather.  The cost is
    the forward count n_run + (r - 1) j len(range(0, n_run - j, j)); info also receives {"forwards"}.  jump_length = 1 is a convention; no
    (resamples, jump_length) has been measured on sleep data.
    context / blend: as in `sample`, on a UNetModel built with context_channels (eegldm_sample_long_edit_ctx).  The context is
    canvas-shaped, (R, C + 1, Lc): with init and mask it is [m * src | m], m the canvas keep-mask and src = encode_long of the MASKED
    recording (window by window); the native loop gathers it once per call into window rows."""
    lay, R, labels = _long_args(unet, autoencoder, scheduler, noise.shape, n_windows, margin, ramp, crop, labels)
    if composite is None and not blend:
        composite = False
    edit = _edit_args(autoencoder, scheduler, (R, int(noise.shape[1]), lay.canvas_len), init, strength, mask, composite, init_canvas,
                      _LONG_EDIT_WORDS, mask_erode)
    rt = _resample_args(scheduler, edit, mask, resamples, jump_length)
    ctx_model = _context_args(unet, context, blend, resamples, R, lay.canvas_len)
    if context is not None and int(context.shape[0]) != R:
        raise ValueError(f"context has {int(context.shape[0])} rows, expected one canvas per recording ({R})")
    if edit is None and context is not None:
        edit = dict(tab=scheduler_edit_tables(scheduler, 1.0), composite=False)
    from .models import UNetModel
    if not isinstance(unet, UNetModel):
        raise TypeError("sample_long runs the native loop: unet must be a UNetModel")
    unet.eval()
    x = noise.to(unet.device, torch.float32).contiguous()
    Cc = x.shape[1]
    if Cc != unet.x_channels:
        raise ValueError(f"noise has {Cc} channels, the UNet takes {unet.x_channels}")
    W, L = lay.n_windows, lay.window_len
    lab, nc = _labels_host(unet, labels, R * W, guidance_scale, null_class)
    down = autoencoder.down if autoencoder is not None else 1
    out_c = autoencoder.out_channels if autoencoder is not None else Cc
    canvas = torch.empty_like(x)
    rec = torch.empty(R, out_c, lay.canvas_len * down, device=unet.device, dtype=torch.float32)
    z0 = m_win = m_lat = init_d = cx_t = None
    if edit is None:
        tab = dict(zip(("timesteps", "a_t", "cx", "c0", "c1"), _multistep_tables(scheduler)))
    else:
        tab = edit["tab"] if rt is None else rt
        encode = lambda r, native: encode_long(autoencoder, r, lay, scale_factor, native=native)
        if init is not None or init_canvas is not None:
            z0, m_win, m_lat, init_d = _edit_inputs(unet, autoencoder, x, init, mask, init_canvas, encode, mask_erode)
        if ctx_model:
            cx_t = _form_context(unet, autoencoder, x, context, z0, m_lat, init_d, encode)
    _run_loop(unet, autoencoder, scheduler, x, tab, lab, guidance_scale, nc, scale_factor, use_graph, seed, info, known=z0, mask=m_lat,
              blend=blend, strength=strength, context=cx_t, context_rows=0 if cx_t is None else R,
              R=R, W=W, L=L, m=lay.margin, r=lay.ramp, canvas_out=canvas.data_ptr(), recording_out=rec.data_ptr())
    if edit is not None and edit["composite"]:
        check(lib.eegldm_edit_window(unet.ctx.h, ptr(m_win), R, lay.canvas_len * down, down, 0, None, ptr(init_d), ptr(rec), out_c, ptr(rec)))
    if info is not None:
        info["layout"] = lay
        if edit is not None:
            info["n_run"] = len(edit["tab"]["timesteps"])
    return (rec[:, :, crop:-crop] if crop else rec), canvas


def _long_x0(o, x, a_t, prediction_type, clip_sample):
    """The data prediction with the library's roundings: sqrt(a_t) and sqrt(1 - a_t) rounded to float32, the products feeding a
    fused multiply-add."""
    a32 = np.float32(a_t)
    sa, sb = float(np.sqrt(a32)), float(np.sqrt(np.float32(1.0) - a32))
    if prediction_type == "epsilon":
        x0 = (_fma32(-sb, o, x).double() / sa).float()
    elif prediction_type == "v_prediction":
        x0 = _fma32(sa, x, -(o * sb))
    else:
        x0 = o
    return x0.clamp(-1.0, 1.0) if clip_sample else x0


def _long_crossfade(rows, lay):
    """rows (R, W, Cc, L) -> (R, Cc, Lc): the owner window's value, fma(u, later, (1 - u) * earlier) inside the ramps (float32 roundings)."""
    R, W, Cc, L = rows.shape
    k1, j = lay.owner()
    k1_t, j_t = torch.from_numpy(k1).to(rows.device), torch.from_numpy(j).to(rows.device)
    out = rows[:, k1_t, :, j_t].permute(1, 2, 0).contiguous()                     # advanced indices first: (Lc, R, Cc) -> (R, Cc, Lc)
    m, r, S = lay.margin, lay.ramp, lay.stride
    if r:
        u = torch.from_numpy(((np.arange(r, dtype=np.float64) + 0.5) / r).astype(np.float32)).to(rows.device)
        for k in range(1, W):
            later, earlier = rows[:, k, :, m:m + r], rows[:, k - 1, :, S + m:S + m + r]
            out[:, :, k * S + m:k * S + m + r] = _fma32(u, later, (1.0 - u) * earlier)
    return out


@torch.no_grad()
def sample_long_hostloop(unet, autoencoder, scheduler, noise, n_windows, margin=None, ramp=None, scale_factor=1.0, crop=36, labels=None,
                         guidance_scale=1.0, null_class=None, use_graph=None, info=None, init=None, init_canvas=None, strength=1.0, mask=None,
                         composite=None, mask_erode=0, resamples=1, jump_length=1, seed=0, context=None, blend=True):
    """The reference composition of sample_long in torch, none of the canvas kernels: slice the canvas, model(...) on all slices, the
    guidance mix, x0 from the scheduler's formulas, the taper of layout.weights (as a cross-fade of the two windows that carry weight),
    prev = cx x + c0 x0 + c1 hist on the canvas, then decode per window and cross-fade.  The float32 roundings are placed where the
    library places them (fused multiply-adds are formed in float64 and rounded once more).  `unet` is any callable
    model(x, timesteps=, [y=]) with .device / .eval(); use_graph is accepted and ignored.
    init / init_canvas / strength / mask / composite / mask_erode as in sample_long (mask_erode defaults to 0; no other value has been
    measured against anything), composed from torch ops: the encode per window and its cross-fade, the noised start, the truncated
    tables, the blend m k + (1 - m) x after every step with the library's roundings (_fma32), the min-pooled mask and the composite.
    resamples / jump_length / seed as in sample_long: the loop runs over the entries of schedulers.resample_tables (whose coefficients are
    first order behind a jump) and forms each jump on the canvas in torch (_jump; the draw is training.randn on the scheduler's context).
    context / blend as in sample_long: the canvas-shaped context is sliced like the canvas and model(win, timesteps=t, context=c) runs per step."""
    lay, R, labels = _long_args(unet, autoencoder, scheduler, noise.shape, n_windows, margin, ramp, crop, labels)
    if composite is None and not blend:
        composite = False
    edit = _edit_args(autoencoder, scheduler, (R, int(noise.shape[1]), lay.canvas_len), init, strength, mask, composite, init_canvas,
                      _LONG_EDIT_WORDS, mask_erode)
    rt = _resample_args(scheduler, edit, mask, resamples, jump_length)
    ctx_model = _context_args(unet, context, blend, resamples, R, lay.canvas_len)
    if context is not None and int(context.shape[0]) != R:
        raise ValueError(f"context has {int(context.shape[0])} rows, expected one canvas per recording ({R})")
    if edit is None and context is not None:
        edit = dict(tab=scheduler_edit_tables(scheduler, 1.0), composite=False)
    unet.eval()
    dev = unet.device
    x = noise.to(dev, torch.float32).contiguous().clone()
    Cc = x.shape[1]
    W, L, S = lay.n_windows, lay.window_len, lay.stride
    lab, nc = _labels_host(unet, labels, R * W, guidance_scale, null_class)
    kw = {} if lab is None else {"y": torch.tensor(lab, dtype=torch.int64, device=dev)}
    null = None if lab is None else torch.full((R * W,), nc, dtype=torch.int64, device=dev)
    w = float(np.float32(guidance_scale))
    ts, a_t, cx, c0, c1 = _multistep_tables(scheduler)
    m_win = m_lat = init_d = None
    if edit is not None:
        tab = edit["tab"] if rt is None else rt
        ts, a_t, cx, c0, c1, a_next = (tab[k] for k in ("timesteps", "a_t", "cx", "c0", "c1", "a_next"))
        nz = x
        z0 = None
        encode = lambda r, native: encode_long(autoencoder, r, lay, scale_factor, native=native)
        if init is not None or init_canvas is not None:
            z0, m_win, m_lat, init_d = _edit_inputs(unet, autoencoder, x, init, mask, init_canvas, encode, mask_erode, native=False)
        if ctx_model:
            cx_t = _form_context(unet, autoencoder, x, context, z0, m_lat, init_d, encode, native=False)
            if cx_t is not None:
                kw["context"] = _slices_of(cx_t, lay).contiguous()
            if not blend:
                m_lat = None
                if float(strength) == 1.0:
                    z0 = None
        if z0 is not None:
            x = _renoise(z0, nz, a_t[0]).clone()
    tt = torch.empty(R * W, device=dev, dtype=torch.int64)
    hist = None
    jumps = 0
    for i, t in enumerate(ts):
        if rt is not None and rt["jump_n"][i] != 0.0:
            x = _jump(scheduler.ctx, x, z0, nz, m_lat, rt, i, jumps, seed)
            jumps += 1
        tt.fill_(t)
        win = _slices_of(x, lay)
        out = unet(win, timesteps=tt, **kw).float()
        if lab is not None and w != 1.0:
            out_u = unet(win, timesteps=tt, **dict(kw, y=null)).float()
            out = _fma32(w, out - out_u, out_u)
        x0 = _long_crossfade(_long_x0(out, win, a_t[i], scheduler.prediction_type, scheduler.clip_sample).reshape(R, W, Cc, L), lay)
        inner = _fma32(c0[i], x0, hist * c1[i]) if c1[i] != 0.0 else x0 * c0[i]
        x = _fma32(cx[i], x, inner)
        hist = x0
        if m_lat is not None:
            x = _blend(m_lat, _renoise(z0, nz, a_next[i]), x)
    if info is not None:
        info["graph"], info["layout"], info["forwards"] = False, lay, len(ts)
    comp = (lambda rec: _blend(m_win, init_d, rec)) if edit is not None and edit["composite"] else (lambda rec: rec)
    if autoencoder is None:
        rec = comp(x)
        return (rec[:, :, crop:-crop] if crop else rec), x
    z = _slices_of(x, lay).contiguous()
    if float(scale_factor) != 1.0:
        # 1 / scale_factor rounded to float32, minus one in float32: the native loop's value (see ddim_sample_hostloop)
        check(lib.eegldm_axpy(autoencoder.ctx.h, ptr(z), ptr(z), float(np.float32(1.0 / float(scale_factor)) - np.float32(1.0)), z.numel()))
    dec = autoencoder.decode_stage_2_outputs(z)
    rec = comp(_long_crossfade(dec.reshape(R, W, dec.shape[1], dec.shape[2]), lay.scaled(autoencoder.down)))
    return (rec[:, :, crop:-crop] if crop else rec), x
