"""Train-step bodies of the reference loops, each one native call per phase:
  ldm_train_step  <-> /root/reference/src/training/training.py:419-443
  Adam            <-> torch.optim.Adam as used at /root/reference/src/train_ldm.py:208
  EMA             exponential moving average of a model's weights, updated inside the Adam kernel (the reference has none)
Gradients live in each model's flat fp32 buffer, so data-parallel training is ONE
all-reduce over a contiguous tensor (see eegldm.distributed)."""
import contextlib
import ctypes as C

import torch

from ._lib import lib, check, ptr, PRED
from .models._flat import pack_into, unpack


class EMA:
    """Exponential moving average of a model's weights: one more flat fp32 buffer (`shadow`) beside `model.flat`.

        ema = EMA(unet, decay=0.9999)           # shadow = copy of unet.flat, num_updates = 0
        opt = Adam(unet, lr=1e-4, ema=ema)      # every opt.step() also moves the shadow, inside the Adam kernel
        with ema.applied():                     # the model computes with the averaged weights; the raw ones come back on exit
            windows, _ = ddim_sample(unet, ...)

    Update n + 1 is ``shadow += (1 - decay_at(n)) * (flat - shadow)``.  With `warmup` the decay ramps up as (1 + n) / (10 + n) until it
    reaches `decay` (the rule of ADM-descended EMA helpers and of diffusers' EMAModel), so that the first updates are not dominated by
    the random initial weights.  Works for any model shim with `flat` / `entries` / `sync_weights` (UNetModel, AutoencoderKL).
    Data-parallel runs: build it after the parameters have been broadcast; gradients are averaged before Adam.step, so every rank's
    shadow stays identical without a collective of its own."""

    def __init__(self, model, decay=0.9999, warmup=True):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"decay must lie in [0, 1), got {decay}")
        self.model, self.decay, self.warmup = model, decay, bool(warmup)
        self.shadow = model.flat.clone()
        self.num_updates = 0
        self._applied = False

    def decay_at(self, n):
        """The decay used by update number n + 1 (n = updates made so far)."""
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        return min(self.decay, (1 + n) / (10 + n)) if self.warmup else self.decay

    def one_minus_decay(self):
        """1 - decay of the NEXT update, in double; the C ABI takes it as a float (rounded once, at the call)."""
        return 1.0 - self.decay_at(self.num_updates)

    def _check_live(self, what):
        if self._applied:
            raise RuntimeError(f"{what} inside `with ema.applied()`: the model holds the averaged weights there")

    def update(self):
        """Stand-alone update from the model's current weights (parameters driven by torch.optim through the autograd bridge)."""
        self._check_live("EMA.update()")
        md = self.model
        check(lib.eegldm_ema_update(md.ctx.h, ptr(self.shadow), ptr(md.flat), md.flat.numel(), self.one_minus_decay()))
        self.num_updates += 1

    def reset(self):
        """shadow = the model's current weights, num_updates = 0 (a run resumed from a checkpoint that has no EMA)."""
        self._check_live("EMA.reset()")
        self.shadow.copy_(self.model.flat)
        self.num_updates = 0

    def _exchange(self):
        md = self.model
        check(lib.eegldm_swap(md.ctx.h, ptr(md.flat), ptr(self.shadow), md.flat.numel()))
        md.sync_weights()                       # every derived copy (16-bit, K-blocked, paired-row) follows the flat buffer
        bump = getattr(md, "_bump_tape", None)
        if bump is not None:
            bump()                              # an autograd graph built over the other weights must not reuse the executor's tape

    @contextlib.contextmanager
    def applied(self):
        """Exchange `model.flat` and the shadow (one pass, in place) and refresh the model's weight copies; on exit exchange them back:
        `model.flat` is bit-identical afterwards.  Does not nest."""
        if self._applied:
            raise RuntimeError("EMA.applied() does not nest")
        self._exchange()
        self._applied = True
        try:
            yield self.model
        finally:
            self._applied = False
            self._exchange()

    def copy_to(self, model=None):
        """Overwrite the weights of `model` (default: the tracked one) with the average."""
        self._check_live("EMA.copy_to()")
        md = self.model if model is None else model
        if md.flat.numel() != self.shadow.numel():
            raise ValueError(f"the model has {md.flat.numel()} parameters, the EMA {self.shadow.numel()}")
        md.flat.copy_(self.shadow.to(md.flat.device))
        md.sync_weights()
        bump = getattr(md, "_bump_tape", None)
        if bump is not None:
            bump()

    def state_dict(self):
        """The averaged weights as a plain model state dict: keys, order and tensor layout of `model.state_dict()`, so the file loads
        into the reference's model and into this one unchanged.  `num_updates` travels separately (see the train scripts' "ema" entry)."""
        self._check_live("EMA.state_dict()")
        return unpack(self.shadow, self.model.entries)

    def load_state_dict(self, sd, num_updates=None):
        self._check_live("EMA.load_state_dict()")
        pack_into(self.shadow, self.model.entries, sd)
        if num_updates is not None:
            self.num_updates = int(num_updates)


def _check_max_norm(max_norm, what="max_grad_norm"):
    x = float(max_norm)
    if not x > 0.0:                        # (a NaN fails the comparison)
        raise ValueError(f"{what} must be > 0 (inf = measure only), got {max_norm}")
    return x


class Adam:
    """torch.optim.Adam defaults (betas 0.9/0.999, eps 1e-8, no weight decay) as one fused HIP
    kernel over the model's flat parameter buffer.  ema: an `EMA` of the same model, updated inside that kernel at every step
    (a step that GradScaler skips therefore skips the EMA update too).
    max_grad_norm: clip the global L2 norm of the (un-scaled) gradient to this value, as torch.nn.utils.clip_grad_norm_ before the step
    would: one more read of the gradient (eegldm_grad_norm), the coefficient stays on the device and multiplies into the update
    (eegldm_adam_step_clip) -- no host read, no rescaling pass, `flat_grad` is left as it is.  None (default): the calls made without it.
    `grad_norm` is a device view of the last norm; `clip_stats()` reads the counters (one host read).  Not optimizer state: `state_dict()`
    keeps torch's layout.  Data-parallel runs: step after the all-reduce -- every rank computes the same coefficient from the averaged gradient."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, ema=None, max_grad_norm=None):
        if max_grad_norm is not None:
            max_grad_norm = _check_max_norm(max_grad_norm)
        if ema is not None and ema.model is not model:
            raise ValueError("the EMA tracks another model")
        self.model, self.lr, self.betas, self.eps, self.ema = model, lr, betas, eps, ema
        self.m = torch.zeros_like(model.flat)
        self.v = torch.zeros_like(model.flat)
        self.step_count = 0
        self.param_groups = [{"lr": lr}]
        self.max_grad_norm, self._clip, self._norm_for, self._clip_snap = None, None, None, None
        self.set_max_grad_norm(max_grad_norm)

    def set_max_grad_norm(self, max_grad_norm):
        """Turns clipping on (a value > 0; inf measures the norm without clipping) or off (None).  The counters start from zero."""
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm)
        self._clip = None if self.max_grad_norm is None else torch.zeros(8, device=self.model.flat.device)      # the `state` of include/eegldm.h
        self._norm_for = self._clip_snap = None

    def zero_grad(self, set_to_none=True):
        self.model.zero_grad()

    @property
    def grad_norm(self):
        """Device scalar: the global norm the last step (or GradScaler.unscale_) measured, before clipping."""
        self._need_clip("grad_norm")
        return self._clip[0]

    def _need_clip(self, what):
        if self._clip is None:
            raise RuntimeError(f"{what} needs Adam(max_grad_norm=...)")

    def clip_stats(self):
        """{"last_norm", "max_norm_seen", "clipped", "steps"} since the last reset_clip_stats() (reads the device, after waiting for the
        context's stream: also right for a Context with a stream of its own)."""
        self._need_clip("clip_stats()")
        self.model.ctx.sync()
        s = self._clip.tolist()
        return {"last_norm": s[0], "max_norm_seen": s[5], "clipped": int(s[3]), "steps": int(s[4])}

    def reset_clip_stats(self):
        self._need_clip("reset_clip_stats()")
        self._clip[3:6].zero_()

    def _norm_pass(self, pre_scale, snapshot=False):
        """The norm pass of the coming step (GradScaler.unscale_ runs it ahead of step(), which then does not repeat it).
        snapshot: keep the counters so that a skipped step can put them back (_norm_discard): a 3-float device copy on torch's current
        stream, which is the context's stream for the default Context (use_torch_stream=True) -- the GradScaler path needs that one."""
        md = self.model
        self._clip_snap = self._clip[3:6].clone() if snapshot else None
        check(lib.eegldm_grad_norm(md.ctx.h, ptr(md.flat_grad), md.flat_grad.numel(), pre_scale, self.max_grad_norm, ptr(self._clip)))
        self._norm_for = float(pre_scale)

    def _norm_discard(self):
        if self._clip_snap is not None:
            self._clip[3:6].copy_(self._clip_snap)
        self._norm_for = self._clip_snap = None

    def step(self, grad_inv_scale=1.0):
        self.step_count += 1
        md, ema = self.model, self.ema
        if ema is not None and ema._applied:
            self.step_count -= 1
            raise RuntimeError("Adam.step() inside `with ema.applied()`: the model holds the averaged weights there")
        if self._clip is not None:             # norm of the un-scaled gradient, then the update with grad_inv_scale * coef (read on the device)
            if self._norm_for is None or self._norm_for != float(grad_inv_scale):
                self._norm_pass(grad_inv_scale)
            self._norm_for = self._clip_snap = None
            check(lib.eegldm_adam_step_clip(md.ctx.h, ptr(md.flat), ptr(md.flat_grad), ptr(self.m), ptr(self.v),
                                            None if ema is None else ptr(ema.shadow), md.flat.numel(), self.param_groups[0]["lr"], self.betas[0],
                                            self.betas[1], self.eps, self.step_count, grad_inv_scale, 0.0 if ema is None else ema.one_minus_decay(),
                                            ptr(self._clip)))
            if ema is not None:
                ema.num_updates += 1
        elif ema is None:
            check(lib.eegldm_adam_step(md.ctx.h, ptr(md.flat), ptr(md.flat_grad), ptr(self.m), ptr(self.v), md.flat.numel(),
                                       self.param_groups[0]["lr"], self.betas[0], self.betas[1], self.eps, self.step_count, grad_inv_scale))
        else:                              # the same update + the EMA of the new weights in one pass over the buffers
            check(lib.eegldm_adam_step_ema(md.ctx.h, ptr(md.flat), ptr(md.flat_grad), ptr(self.m), ptr(self.v), ptr(ema.shadow), md.flat.numel(),
                                           self.param_groups[0]["lr"], self.betas[0], self.betas[1], self.eps, self.step_count, grad_inv_scale,
                                           ema.one_minus_decay()))
            ema.num_updates += 1
        md.sync_weights()

    # ---- checkpoint wire format: torch.optim.Adam's own state_dict layout, so that the optimizer entry of a reference
    # checkpoint.pth (train_autoencoderkl.py:320-329, training/training.py:381-388 store `optimizer.state_dict()`) resumes here
    # and a checkpoint written here resumes under torch.optim.Adam.  Parameter index i = the i-th entry of the model's
    # parameter table (= the order of nn.Module.parameters() in the reference; BatchNorm buffers are not parameters).
    def state_dict(self):
        return flat_to_torch_adam_state(self.model.entries, self.m, self.v, self.step_count, self.param_groups[0]["lr"], self.betas, self.eps)

    def load_state_dict(self, sd):
        if "state" not in sd:             # round-1 private format {step, exp_avg, exp_avg_sq, lr} (flat tensors)
            self.step_count = int(sd["step"]); self.m.copy_(sd["exp_avg"]); self.v.copy_(sd["exp_avg_sq"])
            self.param_groups[0]["lr"] = sd.get("lr", self.lr)
            return
        step, hyper = torch_adam_state_to_flat(self.model.entries, sd, self.m, self.v)
        self.step_count = step
        self.param_groups[0]["lr"] = hyper.get("lr", self.lr)
        self.betas = tuple(hyper.get("betas", self.betas)); self.eps = hyper.get("eps", self.eps)


def _ref_layout(t, shape):
    """flat packed slice -> tensor in the reference shape (conv weights are stored [K][Cout][Cin])"""
    if len(shape) == 3:
        t = t.reshape(shape[2], shape[0], shape[1]).permute(1, 2, 0)
    return t.reshape(shape).contiguous()


def flat_to_torch_adam_state(entries, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8):
    """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]} exactly as torch.optim.Adam.state_dict() lays it out."""
    state = {}
    if step > 0:                       # torch creates per-parameter state lazily at the first step
        for i, (_k, (o, n, shape)) in enumerate(entries.items()):
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": _ref_layout(m[o:o + n], shape).cpu().clone(),
                        "exp_avg_sq": _ref_layout(v[o:o + n], shape).cpu().clone()}
    group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
             "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False,
             "params": list(range(len(entries)))}
    return {"state": state, "param_groups": [group]}


def torch_adam_state_to_flat(entries, sd, m_out, v_out):
    """Inverse of flat_to_torch_adam_state for a state_dict written by torch.optim.Adam (any torch version: `step` may be an int
    or a tensor) or by this class.  Fills the flat moment buffers; returns (step, hyper-parameters of the single param group)."""
    groups = sd["param_groups"]
    if len(groups) != 1:
        raise ValueError("the reference optimizers have a single param group")
    g = groups[0]
    if g.get("amsgrad") or g.get("weight_decay", 0) not in (0, 0.0) or g.get("maximize"):
        raise NotImplementedError("Adam with amsgrad / weight_decay / maximize is not used by the reference (train_ldm.py:208)")
    if len(g["params"]) != len(entries):
        raise ValueError(f"optimizer state covers {len(g['params'])} parameters, the model has {len(entries)}")
    state = sd["state"]
    m_out.zero_(); v_out.zero_()
    steps = set()
    for pos, (k, (o, n, shape)) in enumerate(entries.items()):
        st = state.get(g["params"][pos], state.get(str(g["params"][pos])))
        if st is None:
            continue                   # parameter that never received a gradient
        for name, dst in (("exp_avg", m_out), ("exp_avg_sq", v_out)):
            t = torch.as_tensor(st[name]).detach().to(torch.float32)
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{k}: optimizer state shape {tuple(t.shape)} != parameter shape {tuple(shape)}")
            if len(shape) == 3:
                t = t.permute(2, 0, 1)
            dst[o:o + n].copy_(t.reshape(-1).to(dst.device))
        steps.add(int(float(st["step"])))
    if len(steps) > 1:
        raise ValueError(f"per-parameter step counts differ ({sorted(steps)}); the fused Adam keeps one step count")
    return (steps.pop() if steps else 0), {k2: g[k2] for k2 in ("lr", "betas", "eps") if k2 in g}


class GradScaler:
    """Dynamic loss scaling with torch.cuda.amp.GradScaler's interface and update rule (the reference's LDM / DM loops:
    /root/reference/src/training/training.py:334,441-443 -- ``scaler.scale(loss).backward(); scaler.step(opt); scaler.update()``).

    The native train steps take the scale as their ``grad_scale`` argument (``get_scale()``), ``step`` checks the flat
    gradient buffer for inf/nan on the device (one host read of the flag, as torch's scaler does), skips the optimizer
    step when one is found and otherwise un-scales inside the Adam kernel; ``update`` backs off / grows the scale.
    bf16 and fp32 share fp32's exponent range, so the entry scripts leave it disabled unless asked (--grad-scaler)."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self._scale, self._growth_factor, self._backoff_factor = float(init_scale), float(growth_factor), float(backoff_factor)
        self._growth_interval, self._enabled = int(growth_interval), bool(enabled)
        self._growth_tracker, self._found_inf, self._flag = 0, None, None

    def is_enabled(self):
        return self._enabled

    def get_scale(self):
        return self._scale if self._enabled else 1.0

    def scale(self, outputs):
        return outputs * self.get_scale() if self._enabled else outputs

    def unscale_(self, optimizer, inv_scale_mult=1.0):
        """Records whether optimizer.model's gradients hold an inf/nan (the division itself happens inside the Adam kernel).
        A clipping optimizer (Adam(max_grad_norm=...)): the norm pass of the coming step runs here, with pre_scale = inv_scale_mult / scale,
        and its inf/nan flag is the one read -- the gradient is not read a second time for the check.
        inv_scale_mult: a further factor on 1 / scale (a gradient-accumulation group cut short: K / k)."""
        if not self._enabled:
            return
        md = optimizer.model
        if getattr(optimizer, "max_grad_norm", None) is not None:
            optimizer._norm_pass(float(inv_scale_mult) / self._scale, snapshot=True)
            md.ctx.sync()
            self._found_inf = bool(float(optimizer._clip[2]) != 0.0)
            return
        if self._flag is None or self._flag.device != md.flat_grad.device:
            self._flag = torch.zeros(1, device=md.flat_grad.device)
        check(lib.eegldm_grad_check_finite(md.ctx.h, ptr(md.flat_grad), md.flat_grad.numel(), ptr(self._flag)))
        md.ctx.sync()
        self._found_inf = bool(float(self._flag) != 0.0)

    def step(self, optimizer, inv_scale_mult=1.0):
        clipping = getattr(optimizer, "max_grad_norm", None) is not None
        if not self._enabled:
            return optimizer.step() if inv_scale_mult == 1.0 else optimizer.step(grad_inv_scale=float(inv_scale_mult))
        if self._found_inf is None or (clipping and optimizer._norm_for != float(inv_scale_mult) / self._scale):
            self.unscale_(optimizer, inv_scale_mult)
        if self._found_inf:
            if clipping:
                optimizer._norm_discard()   # the skipped step does not count: the clip counters go back to what they were
            return None                     # skipped: parameters, moments and the optimizer's step count stay as they are
        return optimizer.step(grad_inv_scale=float(inv_scale_mult) / self._scale)

    def update(self, new_scale=None):
        if not self._enabled:
            return
        if new_scale is not None:
            self._scale, self._found_inf = float(new_scale), None
            return
        found = bool(self._found_inf)
        if found:
            self._scale *= self._backoff_factor
            self._growth_tracker = 0
        else:
            self._growth_tracker += 1
            if self._growth_tracker == self._growth_interval:
                self._scale *= self._growth_factor
                self._growth_tracker = 0
        self._found_inf = None

    def state_dict(self):
        return {"scale": self._scale, "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._growth_tracker} if self._enabled else {}

    def load_state_dict(self, sd):
        if not self._enabled or not sd:
            return
        self._scale, self._growth_factor, self._backoff_factor = float(sd["scale"]), float(sd["growth_factor"]), float(sd["backoff_factor"])
        self._growth_interval, self._growth_tracker = int(sd["growth_interval"]), int(sd["_growth_tracker"])


def clip_grad_norm_(model, max_norm):
    """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) on `model.flat_grad`, for parameters stepped by another optimizer (the
    autograd bridge + torch.optim): the norm pass, then flat_grad *= min(1, max_norm / (norm + 1e-6)) in place -- two launches, no host
    read.  Returns the norm before clipping as a device scalar tensor."""
    max_norm = _check_max_norm(max_norm, "max_norm")
    state = getattr(model, "_clip_state", None)
    if state is None or state.device != model.flat_grad.device:
        state = model._clip_state = torch.zeros(8, device=model.flat_grad.device)
    g = model.flat_grad
    check(lib.eegldm_grad_norm(model.ctx.h, ptr(g), g.numel(), 1.0, max_norm, ptr(state)))
    check(lib.eegldm_grad_scale_by(model.ctx.h, ptr(g), g.numel(), ptr(state)))
    return state[0].clone()


GRAD_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_long, C.c_long)


def set_grad_hook(unet, fn):
    """fn(offset, numel) is called from inside the native backward as soon as unet.flat_grad[offset:offset+numel]
    (out / output_blocks / middle_block) is final in stream order; None removes the hook.  The ctypes thunk is kept
    alive on the model."""
    if fn is None:
        unet._grad_hook_thunk = None
        check(lib.eegldm_unet_set_grad_hook(unet.h, None, None))
        return
    thunk = GRAD_HOOK(lambda _user, off, n: fn(int(off), int(n)))
    unet._grad_hook_thunk = thunk
    check(lib.eegldm_unet_set_grad_hook(unet.h, C.cast(thunk, C.c_void_p), None))


def _weighting_args(scheduler, loss_weighting, snr_gamma, per_sample_out, B, device):
    """-> (weighted, device table or None).  Raises before the device is touched."""
    if loss_weighting is None:
        if per_sample_out is not None:
            raise ValueError('per_sample_out needs the weighted loss: pass loss_weighting ("none" leaves every sample at weight 1)')
        return False, None
    from .schedulers import device_loss_weights
    wtab = device_loss_weights(scheduler, loss_weighting, snr_gamma)
    if per_sample_out is not None:
        if per_sample_out.dtype != torch.float32 or per_sample_out.numel() != B or not per_sample_out.is_contiguous():
            raise ValueError(f"per_sample_out must be a contiguous float32 tensor of {B} elements")
        if not per_sample_out.is_cuda or per_sample_out.device != torch.device(device):      # (a host pointer would reach the kernel)
            raise ValueError(f"per_sample_out must live on the model's device {device}, got {per_sample_out.device}")
    return True, wtab


CONTEXT_DRAW_DEFAULTS = {"p_none": 0.1, "p_prefix": 0.3}


def context_draw_args(spec, L):
    """The draw of the training masks as (p_none, p_prefix, span_min, span_max), checked as the library checks it -- a ValueError before the
    device is touched.  spec: a dict with any of p_none (0.1), p_prefix (0.3), span_min (max(1, L // 32)), span_max (max(span_min, L // 2));
    the span defaults are conventions, not values measured on sleep data."""
    unknown = set(spec) - {"p_none", "p_prefix", "span_min", "span_max"}
    if unknown:
        raise ValueError(f"unknown context_mask entries {sorted(unknown)}")
    L = int(L)
    p_none = float(spec.get("p_none", CONTEXT_DRAW_DEFAULTS["p_none"])); p_prefix = float(spec.get("p_prefix", CONTEXT_DRAW_DEFAULTS["p_prefix"]))
    span_min = spec.get("span_min"); span_max = spec.get("span_max")
    span_min = max(1, L // 32) if span_min is None else int(span_min)
    span_max = max(span_min, L // 2) if span_max is None else int(span_max)
    if not (0.0 <= p_none <= 1.0 and 0.0 <= p_prefix <= 1.0):
        raise ValueError(f"p_none={p_none} and p_prefix={p_prefix} must lie in [0, 1]")
    if float(torch.tensor(p_none, dtype=torch.float32) + torch.tensor(p_prefix, dtype=torch.float32)) > 1.0:      # the library's fp32 sum
        raise ValueError(f"p_none + p_prefix = {p_none + p_prefix} exceeds 1")
    if L < 1 or not 1 <= span_min <= span_max <= L:
        raise ValueError(f"the span range [{span_min}, {span_max}] must satisfy 1 <= span_min <= span_max <= L = {L}")
    return p_none, p_prefix, span_min, span_max


def _context_step_args(unet, context_mask, context_latents, mask_out, x, what):
    """-> (mask tensor or None, source tensor or None, draw tuple, mask_out) for eegldm_add_noise_context / eegldm_ldm_train_step_ctx;
    every refusal is a ValueError before the device is touched."""
    B, Cx, L = x.shape
    cc = getattr(unet, "context_channels", 0)
    if not cc:
        raise ValueError(f"context_mask needs a UNetModel built with context_channels ({what})")
    if cc != Cx + 1:
        raise ValueError(f"the step forms a context of {Cx} + 1 channels (masked signal, mask), the model takes {cc}")
    dev = unet.device
    def dev_f32(v, shape, name):
        if not torch.is_tensor(v) or tuple(v.shape) != shape:
            raise ValueError(f"{name} must be a tensor of shape {shape}, got {tuple(v.shape) if torch.is_tensor(v) else type(v).__name__}")
        return v.detach().to(dev, torch.float32).contiguous()
    mask, draw = None, (0.0, 0.0, 1, 1)
    if torch.is_tensor(context_mask):
        mask = dev_f32(context_mask, (B, L), "context_mask")
    elif isinstance(context_mask, dict):
        draw = context_draw_args(context_mask, L)
    else:
        raise ValueError("context_mask must be a (B, L) tensor (1 = keep, 0 = regenerate) or a dict of draw parameters")
    src = None if context_latents is None else dev_f32(context_latents, (B, Cx, L), "context_latents")
    if mask_out is not None:
        if (not torch.is_tensor(mask_out) or mask_out.dtype != torch.float32 or tuple(mask_out.shape) != (B, L) or not mask_out.is_contiguous()
                or not mask_out.is_cuda or mask_out.device != torch.device(dev)):
            raise ValueError(f"mask_out must be a contiguous float32 tensor of shape {(B, L)} on the model's device {dev}")
    return mask, src, draw, mask_out


def context_mask(ctx, B, L, spec=None, seed=0, offset=0, device=None):
    """(B, L) training masks (1 = keep, 0 = regenerate) from eegldm_context_mask: sample b from Philox(seed, offset + b); advance offset by B
    per step.  spec: see context_draw_args."""
    p_none, p_prefix, span_min, span_max = context_draw_args(spec or {}, L)
    if int(B) < 1:
        raise ValueError(f"B={B} must be >= 1")
    out = torch.empty(int(B), int(L), device=device or torch.device("cuda", ctx.device), dtype=torch.float32)
    check(lib.eegldm_context_mask(ctx.h, ptr(out), int(B), int(L), p_none, p_prefix, span_min, span_max, int(seed), int(offset)))
    return out


def context_window(ctx, windows, mask, down):
    """windows * upsample_nearest(mask, down) (eegldm_context_window): windows (B, Co, Lw), mask (B, Lw // down).  The masked input of the
    context encode, in training and in sampling alike."""
    down = int(down)
    if windows.dim() != 3 or mask.dim() != 2 or down < 1 or windows.shape[2] % down or tuple(mask.shape) != (windows.shape[0], windows.shape[2] // down):
        raise ValueError(f"windows {tuple(windows.shape)} and mask {tuple(mask.shape)} do not fit down={down}: mask must be (B, Lw / down)")
    dev = torch.device("cuda", ctx.device)
    w = windows.detach().to(dev, torch.float32).contiguous(); m = mask.detach().to(dev, torch.float32).contiguous()
    out = torch.empty_like(w)
    check(lib.eegldm_context_window(ctx.h, ptr(w), ptr(m), down, ptr(out), w.shape[0], w.shape[1], w.shape[2]))
    return out


def add_noise_context(unet, scheduler, x0, noise, timesteps, context_mask, context_latents=None, mask_seed=0, mask_offset=0, mask_out=None):
    """-> (noisy, context): eegldm_add_noise_context, one launch.  context = [m * (context_latents or x0) | m], (B, C + 1, L)."""
    return _add_noise_context(unet, scheduler, x0, noise, timesteps, _context_step_args(unet, context_mask, context_latents, mask_out, x0, "add_noise_context"),
                              mask_seed, mask_offset)


def _add_noise_context(unet, scheduler, x0, noise, timesteps, checked, mask_seed, mask_offset):
    """add_noise_context behind the checks: checked = what _context_step_args returned"""
    mask, src, draw, mask_out = checked
    B, Cx, L = x0.shape
    noisy = torch.empty_like(x0); context = torch.empty(B, Cx + 1, L, device=x0.device, dtype=torch.float32)
    check(lib.eegldm_add_noise_context(unet.ctx.h, ptr(x0), ptr(src), ptr(noise), ptr(timesteps), ptr(scheduler._acp_dev), ptr(mask), draw[0], draw[1],
                                       draw[2], draw[3], int(mask_seed), int(mask_offset), ptr(noisy), ptr(context), ptr(mask_out), B, Cx, L))
    return noisy, context


def ldm_train_step(unet, scheduler, latents, noise, timesteps, loss_out=None, grad_scale=1.0, grad_sync=None, labels=None, p_uncond=0.0,
                   null_class=None, seed=0, offset=0, loss_weighting=None, snr_gamma=5.0, per_sample_out=None, context_mask=None,
                   context_latents=None, mask_seed=0, mask_offset=0, mask_out=None):
    """add_noise -> UNet forward -> MSE against noise (epsilon) or velocity (v_prediction) -> backward.
    Accumulates into unet.flat_grad; returns the device scalar loss tensor.  grad_sync: an
    eegldm.distributed.OverlappedGradSync -- the tail of the gradient buffer is all-reduced while the input blocks'
    backward still runs, the rest right after the call; the caller then only has to `grad_sync.wait()`.
    labels (a UNet built with num_classes): the class of every sample, (B,) integers.  Classifier-free guidance training: with
    probability p_uncond a sample's label is replaced by null_class on the device, drawn from the Philox stream (seed, offset + b)
    -- advance `offset` by B per step; the backward uses the replaced labels.
    loss_weighting: None (default) = the plain MSE through the exports above.  "none" / "min_snr" / a (T,) table (schedulers.loss_weights,
    snr_gamma) = the weighted step (eegldm_ldm_train_step_weighted): sample b counts wtab[t_b] in the loss and its gradient, and
    per_sample_out (a (B,) float32 device tensor) receives the UNWEIGHTED per-sample losses (for NoiseLevelLoss).
    context_mask (a UNetModel built with context_channels = C + 1; required there, refused elsewhere): a (B, L) keep-mask (1 = keep, 0 =
    regenerate) or a dict of draw parameters (context_draw_args) -- the masks are then drawn on the device from Philox(mask_seed,
    mask_offset + b), advance mask_offset by B per step.  The model sees [m * context_latents | m] as its context (context_latents None:
    the latents themselves; the LDM passes the encoding of the MASKED window) and the loss runs over the whole sample
    (eegldm_ldm_train_step_ctx; weights as loss_weighting says, None = all ones).  mask_out ((B, L) float32 device tensor): the masks used."""
    B, _C, L = latents.shape
    ctx_model = bool(getattr(unet, "context_channels", 0))
    if ctx_model != (context_mask is not None):
        raise ValueError("context_mask must be given if and only if the UNet was built with context_channels")
    if ctx_model:
        cmask, csrc, cdraw, mask_out = _context_step_args(unet, context_mask, context_latents, mask_out, latents, "ldm_train_step")
        if loss_weighting is None:
            loss_weighting = "none"
    elif context_latents is not None or mask_out is not None:
        raise ValueError("context_latents / mask_out need context_mask")
    weighted, wtab = _weighting_args(scheduler, loss_weighting, snr_gamma, per_sample_out, B, unet.device)
    if loss_out is None:
        loss_out = torch.zeros(1, device=unet.device)
    cond = getattr(unet, "num_classes", None) is not None
    if cond != (labels is not None):
        raise ValueError("labels must be given if and only if the UNet is class-conditional")
    if cond:
        lab = unet.check_labels(labels)
        if tuple(lab.shape) != (B,):
            raise ValueError(f"labels must have shape ({B},), got {tuple(lab.shape)}")
        if not 0.0 <= float(p_uncond) <= 1.0:
            raise ValueError(f"p_uncond={p_uncond} outside [0, 1]")
        if float(p_uncond) > 0.0 and null_class is None:
            raise ValueError("p_uncond > 0 needs null_class")
        nc = 0 if null_class is None else int(null_class)
        if null_class is not None and not 0 <= nc < unet.num_classes:
            raise IndexError(f"null_class {nc} is out of range for num_classes={unet.num_classes}")
    if grad_sync is not None:
        grad_sync.begin()
        set_grad_hook(unet, grad_sync.on_ready)
    try:
        if ctx_model:
            check(lib.eegldm_ldm_train_step_ctx(unet.h, ptr(latents), ptr(noise), ptr(timesteps), ptr(scheduler._acp_dev),
                                                PRED[scheduler.prediction_type], B, L, grad_scale, ptr(loss_out), ptr(wtab),
                                                ptr(per_sample_out), ptr(lab) if cond else None, float(p_uncond) if cond else 0.0,
                                                nc if cond else 0, int(seed), int(offset), ptr(csrc), ptr(cmask), cdraw[0], cdraw[1], cdraw[2],
                                                cdraw[3], int(mask_seed), int(mask_offset), ptr(mask_out)))
        elif weighted:
            check(lib.eegldm_ldm_train_step_weighted(unet.h, ptr(latents), ptr(noise), ptr(timesteps), ptr(scheduler._acp_dev),
                                                     PRED[scheduler.prediction_type], B, L, grad_scale, ptr(loss_out), ptr(wtab),
                                                     ptr(per_sample_out), ptr(lab) if cond else None, float(p_uncond) if cond else 0.0,
                                                     nc if cond else 0, int(seed), int(offset)))
        elif cond:
            check(lib.eegldm_ldm_train_step_cond(unet.h, ptr(latents), ptr(noise), ptr(timesteps), ptr(scheduler._acp_dev),
                                                 PRED[scheduler.prediction_type], B, L, grad_scale, ptr(loss_out), ptr(lab), float(p_uncond),
                                                 nc, int(seed), int(offset)))
        else:
            check(lib.eegldm_ldm_train_step(unet.h, ptr(latents), ptr(noise), ptr(timesteps), ptr(scheduler._acp_dev),
                                            PRED[scheduler.prediction_type], B, L, grad_scale, ptr(loss_out)))
    finally:
        unet._bump_tape()                    # forward + backward ran inside the call: an older autograd graph's tape is gone
        if grad_sync is not None:
            set_grad_hook(unet, None)
    if grad_sync is not None:
        grad_sync.finish()
    return loss_out


def usleep_train_step(model, x, labels, class_weight=None, grad_scale=1.0, loss_out=None, grad_sync=None):
    """One U-Sleep stager step (eegldm.metrics.USleep.train_step): training forward -> weighted stage cross-entropy -> backward, accumulating
    into model.flat_grad; returns the device scalar loss.  grad_sync: an eegldm.distributed.OverlappedGradSync over model.flat_grad -- the
    step has no gradient hook, so the whole buffer is reduced right after the call; the caller then only has to `grad_sync.wait()`."""
    if grad_sync is not None:
        grad_sync.begin()
    loss = model.train_step(x, labels, class_weight=class_weight, grad_scale=grad_scale, loss_out=loss_out)
    if grad_sync is not None:
        grad_sync.finish()
    return loss


def dm_train_step(unet, scheduler, images, noise, timesteps, spectral_weight=0.0, spectral_loss=False, loss_out=None, grad_sync=None, grad_scale=1.0,
                  loss_weighting=None, snr_gamma=5.0, per_sample_out=None, context_mask=None, context_latents=None, mask_seed=0, mask_offset=0,
                  mask_out=None):
    """Pixel-space diffusion step of /root/reference/src/training/training_diffusion.py:141-151 (config_dm.yaml, BASELINE C5):
    epsilon prediction directly on the (B,1,3072) windows, loss = mse(noise_pred, noise) [+ spectral_weight *
    JukeboxLoss(sum)(noise_pred, noise)].  Composed from the same native calls as the latent step: add_noise, UNet forward,
    MSE (writes d pred), spectral loss (accumulates its gradient into d pred), hand-written backward.  Returns the loss tensor.
    grad_scale: the GradScaler's loss scale (training_diffusion.py:37,149-151 -- `scaler.scale(loss).backward()`): it multiplies d pred, i.e.
    every gradient of the backward; the reported loss stays unscaled and the optimizer step divides the scale out again (GradScaler.step).
    loss_weighting / snr_gamma / per_sample_out: as in ldm_train_step -- eegldm_diffusion_loss (target of the scheduler's prediction type) in
    place of eegldm_mse_loss; the spectral term still accumulates into d pred afterwards, unweighted.
    context_mask / context_latents / mask_seed / mask_offset / mask_out: as in ldm_train_step, on a UNetModel built with context_channels --
    eegldm_add_noise_context in place of add_noise, then unet(noisy, timesteps=t, context=c); the loss still runs over the whole window."""
    ctx_model = bool(getattr(unet, "context_channels", 0))
    if ctx_model != (context_mask is not None):
        raise ValueError("context_mask must be given if and only if the UNet was built with context_channels")
    if not ctx_model and (context_latents is not None or mask_out is not None):
        raise ValueError("context_latents / mask_out need context_mask")
    if ctx_model:                              # (the refusals, ahead of everything else)
        checked = _context_step_args(unet, context_mask, context_latents, mask_out, images, "dm_train_step")
    weighted, wtab = _weighting_args(scheduler, loss_weighting, snr_gamma, per_sample_out, images.shape[0], unet.device)
    dev = unet.device
    if loss_out is None:
        loss_out = torch.zeros(1, device=dev)
    unet.train()
    x = images.to(dev, torch.float32).contiguous(); nz = noise.to(dev, torch.float32).contiguous()
    B, Cc, L = x.shape
    if ctx_model:
        t = timesteps.to(dev, torch.int64).contiguous()
        noisy, context = _add_noise_context(unet, scheduler, x, nz, t, checked, mask_seed, mask_offset)
        pred = unet(noisy, timesteps=t, context=context)
    else:
        noisy = scheduler.add_noise(original_samples=x, noise=nz, timesteps=timesteps)
        pred = unet(noisy, timesteps=timesteps)
    dpred = torch.empty_like(pred)
    if weighted:
        t = timesteps.to(dev, torch.int64).contiguous()
        check(lib.eegldm_diffusion_loss(unet.ctx.h, ptr(pred), ptr(x), ptr(nz), ptr(t), ptr(scheduler._acp_dev), ptr(wtab),
                                        PRED[scheduler.prediction_type], B, Cc * L, float(grad_scale), ptr(loss_out), ptr(per_sample_out), ptr(dpred)))
    else:
        check(lib.eegldm_mse_loss(unet.ctx.h, ptr(pred), ptr(nz), ptr(loss_out), ptr(dpred), pred.numel(), float(grad_scale)))
    if spectral_loss:
        spec = torch.zeros(1, device=dev)
        check(lib.eegldm_spectral_loss(unet.ctx.h, ptr(pred), ptr(nz), ptr(spec), ptr(dpred), B, Cc, L, float(spectral_weight) * float(grad_scale)))
        loss_out.add_(spec, alpha=float(spectral_weight))
    if grad_sync is not None:
        grad_sync.begin()
        set_grad_hook(unet, grad_sync.on_ready)
    try:
        unet.backward(dpred)
    finally:
        if grad_sync is not None:
            set_grad_hook(unet, None)
    if grad_sync is not None:
        grad_sync.finish()
    return loss_out


class NoiseLevelLoss:
    """Loss by noise level: the unweighted per-sample losses of many steps, accumulated into `bins` equal ranges of the timestep
    (bin k = t * bins // num_train_timesteps), so that a run can be read at the noise levels that matter instead of as one average over
    values that differ by orders of magnitude.

        nll = NoiseLevelLoss(1000, bins=10)
        ldm_train_step(..., loss_weighting="min_snr", per_sample_out=per); nll.add(per, t)      # no host synchronisation
        nll.table()  -> [{"t_lo", "t_hi", "count", "mean"}, ...]      (mean None for an empty bin)

    Device tensors go through eegldm_loss_bins into fp32 / int64 device accumulators (samples in ascending order: order-fixed); numpy
    arrays and CPU tensors are accumulated on the host in float64.  state() / merge() add several ranks' accumulators.
    Precision of the device path: a bin's sum is ONE float32 running sum over everything added since reset(), so after n windows in a bin
    its mean can be off by up to about n * 2^-24 relative (1e5 windows: below 1 %, typically 1e-4 to 1e-3) -- a monitoring table, not a
    number to select models on at many digits.  reset() per epoch (as the train scripts do) or fold state() into a host accumulator
    (load_state) more often where that matters."""

    def __init__(self, num_train_timesteps, bins=10):
        T, K = int(num_train_timesteps), int(bins)
        if T < 1 or not 1 <= K <= T:
            raise ValueError(f"bins must lie in [1, num_train_timesteps], got bins={bins}, num_train_timesteps={num_train_timesteps}")
        self.num_train_timesteps, self.bins = T, K
        self.reset()

    def reset(self):
        self._sum, self._cnt = [0.0] * self.bins, [0] * self.bins
        self._dev = None            # (ctx, bin_sum float32 (K,), bin_cnt int64 (K,)) once a device tensor has been added

    def add(self, per_sample, timesteps, ctx=None):
        if torch.is_tensor(per_sample) and per_sample.is_cuda:
            ps = per_sample.detach().reshape(-1).to(torch.float32).contiguous()
            t = timesteps.to(ps.device, torch.int64).reshape(-1).contiguous()
            if t.numel() != ps.numel():
                raise ValueError(f"{ps.numel()} losses but {t.numel()} timesteps")
            if self._dev is None:
                from ._lib import default_context
                c = ctx or default_context(ps.device.index or 0)
                self._dev = (c, torch.zeros(self.bins, device=ps.device), torch.zeros(self.bins, dtype=torch.int64, device=ps.device))
            c, bsum, bcnt = self._dev
            check(lib.eegldm_loss_bins(c.h, ptr(ps), ptr(t), ps.numel(), self.num_train_timesteps, self.bins, ptr(bsum), ptr(bcnt)))
            return self
        ps = [float(v) for v in (per_sample.detach().reshape(-1).tolist() if torch.is_tensor(per_sample) else list(per_sample))]
        ts = [int(v) for v in (timesteps.reshape(-1).tolist() if torch.is_tensor(timesteps) else list(timesteps))]
        if len(ps) != len(ts):
            raise ValueError(f"{len(ps)} losses but {len(ts)} timesteps")
        for m, t in zip(ps, ts):
            if 0 <= t < self.num_train_timesteps:
                k = t * self.bins // self.num_train_timesteps
                self._sum[k] += m; self._cnt[k] += 1
        return self

    def state(self):
        """[sum_0 .. sum_{K-1}, count_0 .. count_{K-1}] as Python floats: host and device accumulators together (reads the device)."""
        s, n = list(self._sum), list(self._cnt)
        if self._dev is not None:
            _c, bsum, bcnt = self._dev
            s = [a + float(b) for a, b in zip(s, bsum.tolist())]; n = [a + int(b) for a, b in zip(n, bcnt.tolist())]
        return [float(v) for v in s] + [float(v) for v in n]

    def load_state(self, state):
        K = self.bins
        if len(state) != 2 * K:
            raise ValueError(f"a state of {2 * K} numbers is expected, got {len(state)}")
        self.reset()
        self._sum, self._cnt = [float(v) for v in state[:K]], [int(round(float(v))) for v in state[K:]]
        return self

    def merge(self, like=None):
        """Adds the accumulators of all ranks (distributed.allreduce_sum_scalars; one process: unchanged).  Every rank ends with the total."""
        from . import distributed as D
        return self.load_state(D.allreduce_sum_scalars(self.state(), like=like))

    def table(self):
        T, K = self.num_train_timesteps, self.bins
        st = self.state()
        rows = []
        for k in range(K):
            lo, hi = -(-k * T // K), -(-(k + 1) * T // K) - 1       # the timesteps t with t * K // T == k
            n = int(st[K + k])
            rows.append({"t_lo": lo, "t_hi": hi, "count": n, "mean": (st[k] / n) if n else None})
        return rows


def randn(ctx, shape, seed, offset=0, device=None):
    out = torch.empty(shape, device=device or torch.device("cuda", ctx.device), dtype=torch.float32)
    check(lib.eegldm_randn(ctx.h, ptr(out), out.numel(), seed, offset))
    return out


def label_dropout(ctx, labels, p_uncond, null_class, seed, offset=0):
    """The label dropout of the conditional train step on its own: each label -> null_class with probability p_uncond."""
    out = torch.empty_like(labels)
    check(lib.eegldm_label_dropout(ctx.h, ptr(labels), ptr(out), labels.numel(), float(p_uncond), int(null_class), int(seed), int(offset)))
    return out


def randint(ctx, n, high, seed, offset=0, device=None):
    out = torch.empty(n, device=device or torch.device("cuda", ctx.device), dtype=torch.int64)
    check(lib.eegldm_randint(ctx.h, ptr(out), n, high, seed, offset))
    return out


def aekl_train_step(autoencoder, discriminator, x, eps, adv_weight, kl_weight, spectral_weight, use_spectral,
                    losses_out=None, recon_out=None):
    """The step body of /root/reference/src/train_autoencoderkl.py:203-234 as ONE native call: fills
    autoencoder.flat_grad and discriminator.flat_grad (both must be zeroed first) and returns the device
    tensor [recons L1, spectral, KL, generator adversarial, D fake, D real]."""
    dev = autoencoder.device
    if losses_out is None:
        losses_out = torch.zeros(6, device=dev)
    B, _c, L = x.shape
    check(lib.eegldm_aekl_train_step(autoencoder.h, discriminator.h, ptr(x), ptr(eps), float(adv_weight), float(kl_weight),
                                     float(spectral_weight), 1 if use_spectral else 0, ptr(losses_out), ptr(recon_out), B, L))
    autoencoder._bump_tape(); discriminator._bump_tape()
    return losses_out
