"""Loss callables with the interfaces the reference trainer uses
(/root/reference/src/train_autoencoderkl.py:155-158): L1Loss, PatchAdversarialLoss("least_squares"),
JukeboxLoss(spatial_dims=1, reduction="sum"), plus mse_loss.  Each call is one native launch that produces the value and -- when the
input carries a graph (eegldm.autograd) -- its gradient; the fused native train step (eegldm.training.aekl_train_step) remains the
fast path."""
import torch

from ._lib import lib, check, ptr, default_context, PRED
from .autograd import grad_loss


class _Loss:
    def __init__(self, device=0, ctx=None):
        self.ctx = ctx or default_context(device)
        self.device = torch.device("cuda", self.ctx.device)

    def _prep(self, t):
        return t.to(self.device, torch.float32).contiguous()


class L1Loss(_Loss):
    def __call__(self, inp, target):
        a, b = self._prep(inp), self._prep(target).detach()

        def run(x, g):
            out = torch.zeros((), device=self.device)
            check(lib.eegldm_l1_loss(self.ctx.h, ptr(x), ptr(b), ptr(out), ptr(g), x.numel(), 1.0 if g is not None else 0.0))
            return out
        return grad_loss(run, a)


class JukeboxLoss(_Loss):
    def __init__(self, spatial_dims=1, fft_signal_size=None, fft_norm="ortho", reduction="mean", **k):
        super().__init__(**k)
        if spatial_dims != 1 or fft_signal_size is not None or fft_norm != "ortho":
            raise NotImplementedError("reference uses JukeboxLoss(spatial_dims=1, reduction='sum')")
        self.reduction = reduction

    def __call__(self, inp, target):
        a, b = self._prep(inp), self._prep(target).detach()
        B, Cc, L = a.shape

        def run(x, g):
            out = torch.zeros((), device=self.device)
            check(lib.eegldm_spectral_loss(self.ctx.h, ptr(x), ptr(b), ptr(out), ptr(g), B, Cc, L, 1.0 if g is not None else 0.0))
            return out
        out = grad_loss(run, a)
        return out if self.reduction == "sum" else out / a.numel()


class PatchAdversarialLoss(_Loss):
    def __init__(self, reduction="mean", criterion="least_squares", no_activation_leastsq=False, **k):
        super().__init__(**k)
        if criterion != "least_squares" or no_activation_leastsq or reduction != "mean":
            raise NotImplementedError("reference uses PatchAdversarialLoss(criterion='least_squares')")

    def __call__(self, logits, target_is_real, for_discriminator):
        if isinstance(logits, (list, tuple)):
            logits = logits[-1]
        if not for_discriminator:
            target_is_real = True
        a = self._prep(logits)

        def run(x, g):
            out = torch.zeros((), device=self.device)
            check(lib.eegldm_lsgan_loss(self.ctx.h, ptr(x), 1 if target_is_real else 0, ptr(out), ptr(g), x.numel(), 1.0 if g is not None else 0.0))
            return out
        return grad_loss(run, a)


def mse_loss(inp, target, ctx=None):
    """F.mse_loss(input, target) (training.py:437) on the native kernel: value and gradient from one launch."""
    c = ctx or default_context(inp.device.index or 0)
    a = inp.to(torch.float32).contiguous(); b = target.to(a.device, torch.float32).contiguous().detach()

    def run(x, g):
        out = torch.zeros((), device=a.device)
        check(lib.eegldm_mse_loss(c.h, ptr(x), ptr(b), ptr(out), ptr(g), x.numel(), 1.0))
        return out
    return grad_loss(run, a)


class _DiffusionLossFn(torch.autograd.Function):
    """(loss, per-sample losses) and d loss / d pred from ONE native call; backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, pred, run):
        need = ctx.needs_input_grad[0]
        g = torch.empty_like(pred) if need else None
        loss, per = run(pred, g)
        ctx.mark_non_differentiable(per)
        if need:
            ctx.save_for_backward(g)
        ctx.has_grad = need
        return loss, per

    @staticmethod
    def backward(ctx, dloss, _dper):
        if not ctx.has_grad:
            return None, None
        (g,) = ctx.saved_tensors
        return g * dloss, None


def diffusion_loss(pred, x0, noise, timesteps, scheduler, weighting="min_snr", snr_gamma=5.0):
    """Weighted diffusion loss of a model output against the target of the scheduler's prediction type (noise, velocity or x0), on
    eegldm_diffusion_loss: -> (loss, per_sample).  loss = mean over samples of w[t_b] * mse_b with the table of
    schedulers.loss_weights(weighting, snr_gamma); per_sample (B,) holds the unweighted mse_b and carries no gradient.  Differentiable
    w.r.t. `pred` (value and gradient from one native call), so the reference's loop body -- loss.backward(), torch.optim.Adam -- trains with the
    weighting through eegldm.autograd."""
    from .schedulers import device_loss_weights
    wtab = device_loss_weights(scheduler, weighting, snr_gamma)
    c, dev = scheduler.ctx, scheduler.device
    a = pred.to(dev, torch.float32).contiguous()
    x = x0.to(dev, torch.float32).contiguous().detach(); nz = noise.to(dev, torch.float32).contiguous().detach()
    t = timesteps.to(dev, torch.int64).contiguous()
    B = a.shape[0]
    if x.shape != a.shape or nz.shape != a.shape or tuple(t.shape) != (B,):
        raise ValueError(f"pred {tuple(a.shape)}, x0 {tuple(x.shape)}, noise {tuple(nz.shape)} must agree and timesteps be ({B},)")

    def run(p, g):
        out, per = torch.zeros((), device=dev), torch.empty(B, device=dev)
        check(lib.eegldm_diffusion_loss(c.h, ptr(p), ptr(x), ptr(nz), ptr(t), ptr(scheduler._acp_dev), ptr(wtab), PRED[scheduler.prediction_type],
                                        B, p[0].numel(), 1.0, ptr(out), ptr(per), ptr(g)))
        return out, per
    if a.requires_grad and torch.is_grad_enabled():
        return _DiffusionLossFn.apply(a, run)
    return run(a, None)
