"""`UNetModel` -- host-side mirror of the reference denoiser's interface
(/root/reference/src/models/unet.py:330-563: same constructor kwargs, same
`forward(x, timesteps=..., y=...)`, same 278-key `state_dict()` -- 279 with
`label_emb.weight` when built with `num_classes`), executing on the
hand-written HIP kernels of libeegldm.so through the C ABI.

torch is used for device memory only.  Two ways to train: the fused native step
(eegldm.training.ldm_train_step: add_noise + forward + MSE + backward in one call, the
fast path), or -- once `parameters()` has been handed to a torch optimizer -- the
reference's own loop body: `model(x=..., timesteps=...)` then returns a tensor with a
grad_fn whose backward is the hand-written native backward (eegldm.autograd).
"""
import ctypes as C
import math
from collections import OrderedDict

import torch

from .._lib import lib, check, ptr, default_context, UNetCfg, F32, BF16, F16
from ..autograd import FlatModule, _UNetFn

_DT = {"float32": F32, "fp32": F32, torch.float32: F32, "bfloat16": BF16, "bf16": BF16, torch.bfloat16: BF16, "float16": F16, "fp16": F16, "half": F16, torch.float16: F16, F32: F32, BF16: BF16, F16: F16}
_ZERO_INIT_SUFFIX = ("out_layers.3.weight", "out_layers.3.bias", "proj_out.weight", "proj_out.bias", "out.2.weight", "out.2.bias")


class UNetModel(FlatModule):
    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, num_classes=None, num_heads=1,
                 num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 n_embed=None, dtype="float32", device=0, ctx=None, context_channels=0):
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        self.dropout = float(dropout)
        if n_embed is not None:
            raise NotImplementedError("codebook heads (n_embed) are not used by the reference configs")
        if num_classes is not None and (int(num_classes) != num_classes or int(num_classes) < 1):
            raise ValueError(f"num_classes must be a positive integer, got {num_classes!r}")
        self.num_classes = None if num_classes is None else int(num_classes)
        # context conditioning: the last context_channels of the in_channels input channels come from `context` (forward), the first
        # in_channels - context_channels == out_channels from x; parameters and state_dict are a plain UNetModel(in_channels)'s
        if int(context_channels) != context_channels or int(context_channels) < 0:
            raise ValueError(f"context_channels must be a non-negative integer, got {context_channels!r}")
        self.context_channels = int(context_channels)
        if self.context_channels and in_channels - self.context_channels != out_channels:
            raise ValueError(f"a context model needs in_channels - context_channels == out_channels, got {in_channels} - "
                             f"{self.context_channels} != {out_channels}")
        self.x_channels = in_channels - self.context_channels
        num_heads, num_head_channels, num_heads_upsample = int(num_heads), int(num_head_channels), int(num_heads_upsample)
        if num_heads < 1 or num_head_channels == 0:
            raise ValueError("num_heads >= 1 and num_head_channels = -1 or > 0 (unet.py:146-153)")
        self.conv_resample, self.num_heads, self.num_head_channels = bool(conv_resample), num_heads, num_head_channels
        self.num_heads_upsample = num_heads if num_heads_upsample == -1 else num_heads_upsample      # unet.py:354-355
        self.use_scale_shift_norm, self.resblock_updown = bool(use_scale_shift_norm), bool(resblock_updown)
        self.image_size, self.in_channels, self.model_channels, self.out_channels = image_size, in_channels, model_channels, out_channels
        self.num_res_blocks, self.attention_resolutions, self.channel_mult = num_res_blocks, list(attention_resolutions), list(channel_mult)
        self.dtype = _DT[dtype]
        self.ctx = ctx or default_context(device if isinstance(device, int) else torch.device(device).index or 0)
        self.device = torch.device("cuda", self.ctx.device)
        cfg = UNetCfg()
        cfg.in_channels, cfg.out_channels, cfg.model_channels, cfg.num_res_blocks = in_channels, out_channels, model_channels, num_res_blocks
        cfg.n_mult = len(self.channel_mult)
        for i, m in enumerate(self.channel_mult):
            cfg.channel_mult[i] = int(m)
        cfg.n_attn = len(self.attention_resolutions)
        for i, a in enumerate(self.attention_resolutions):
            cfg.attention_resolutions[i] = int(a)
        cfg.num_heads, cfg.dtype = self.num_heads, self.dtype
        cfg.num_head_channels = self.num_head_channels if self.num_head_channels > 0 else 0
        cfg.num_heads_upsample = self.num_heads_upsample
        cfg.use_scale_shift_norm = int(self.use_scale_shift_norm)
        cfg.resample_layers = 0 if self.resblock_updown else 1                          # Downsample / Upsample layers (unet.py:462-470,493-498)
        cfg.resample_pool_only = 0 if self.conv_resample else 1
        h = C.c_void_p()
        if self.context_channels:
            check(lib.eegldm_unet_create_ctx(self.ctx.h, C.byref(cfg), self.num_classes or 0, self.context_channels, C.byref(h)))
        elif self.num_classes is None:
            check(lib.eegldm_unet_create(self.ctx.h, C.byref(cfg), C.byref(h)))
        else:                       # label_emb = nn.Embedding(num_classes, 4 * model_channels) (unet.py:379-380)
            check(lib.eegldm_unet_create_cond(self.ctx.h, C.byref(cfg), self.num_classes, C.byref(h)))
        self.h = h
        if self.dropout > 0.0:      # nn.Dropout(p) of every ResBlock (unet.py:289): training-mode forwards only, masks from the device Philox stream
            self.set_dropout_seed(0x0D50)
        self.n_flat = int(lib.eegldm_unet_num_params(self.h))
        self.entries = OrderedDict()
        name = C.create_string_buffer(256)
        off, numel, ndim, shape = C.c_long(), C.c_long(), C.c_int(), (C.c_int * 3)()
        for i in range(lib.eegldm_unet_num_entries(self.h)):
            check(lib.eegldm_unet_entry(self.h, i, name, 256, C.byref(off), C.byref(numel), C.byref(ndim), shape))
            self.entries[name.value.decode()] = (off.value, numel.value, tuple(shape[k] for k in range(ndim.value)))
        self.flat = torch.zeros(self.n_flat, device=self.device, dtype=torch.float32)
        self.flat_grad = torch.zeros(self.n_flat, device=self.device, dtype=torch.float32)
        check(lib.eegldm_unet_bind(self.h, ptr(self.flat), ptr(self.flat_grad)))
        self.training = True
        self.reset_parameters()

    def set_dropout_seed(self, seed):
        """(Re)start the dropout mask stream: the same seed gives the same masks for the same sequence of training forwards
        (torch's counterpart is `torch.manual_seed` ahead of the loop)."""
        check(lib.eegldm_unet_set_dropout(self.h, self.dropout, int(seed)))

    # ------------------------------------------------------------------ parameters
    def reset_parameters(self, generator=None):
        """torch.nn default init (kaiming_uniform(a=sqrt(5)) == U(+-1/sqrt(fan_in)) for weights and biases),
        GroupNorm (1, 0), the reference's zero_module layers (unet.py:39-45) and nn.Embedding's N(0, 1) for label_emb."""
        sd = OrderedDict()
        for k, (_o, _n, shape) in self.entries.items():
            if k == "label_emb.weight":
                sd[k] = torch.randn(shape, generator=generator)
            elif len(shape) == 1 and (".in_layers.0." in k or ".out_layers.0." in k or ".norm." in k or k.startswith("out.0.")):
                sd[k] = torch.ones(shape) if k.endswith("weight") else torch.zeros(shape)
            elif k.endswith(_ZERO_INIT_SUFFIX):
                sd[k] = torch.zeros(shape)
            else:
                wshape = shape if len(shape) > 1 else self.entries[k[:-4] + "weight"][2]
                bound = 1.0 / math.sqrt(int(torch.tensor(wshape[1:]).prod()))
                sd[k] = (torch.rand(shape, generator=generator) * 2 - 1) * bound
        self.load_state_dict(sd)

    def state_dict(self):
        out = OrderedDict()
        for k, (o, n, shape) in self.entries.items():
            t = self.flat[o:o + n]
            if len(shape) == 3:       # packed [K][Cout][Cin] -> reference (Cout, Cin, K)
                t = t.reshape(shape[2], shape[0], shape[1]).permute(1, 2, 0)
            out[k] = t.reshape(shape).clone()
        return out

    def grad_dict(self):
        out = OrderedDict()
        for k, (o, n, shape) in self.entries.items():
            t = self.flat_grad[o:o + n]
            if len(shape) == 3:
                t = t.reshape(shape[2], shape[0], shape[1]).permute(1, 2, 0)
            out[k] = t.reshape(shape).clone()
        return out

    def load_state_dict(self, sd, strict=True):
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}   # DataParallel prefix (compute_mmds.py:475-478)
        missing = [k for k in self.entries if k not in sd]
        extra = [k for k in sd if k not in self.entries]
        if strict and (missing or extra):
            raise KeyError(f"state_dict mismatch: missing {missing[:4]}..., unexpected {extra[:4]}...")
        for k, (o, n, shape) in self.entries.items():
            if k not in sd:
                continue
            v = torch.as_tensor(sd[k]).detach().to(torch.float32)
            if tuple(v.shape) != tuple(shape):
                raise ValueError(f"{k}: shape {tuple(v.shape)} != {tuple(shape)}")
            if len(shape) == 3:
                v = v.permute(2, 0, 1)
            self.flat[o:o + n].copy_(v.reshape(-1).to(self.device))
        self.sync_weights()

    def sync_weights(self):
        check(lib.eegldm_unet_sync_weights(self.h))
        self._mark_synced()

    def zero_grad(self, set_to_none=True):
        self.flat_grad.zero_()

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def to(self, *a, **k):
        return self

    # ------------------------------------------------------------------ compute
    def forward(self, x, timesteps=None, context=None, y=None, **kwargs):
        if self.num_classes is not None:                 # unet.py:517-519 (same assertion text; y on an unconditional model is ignored)
            assert y is not None, "must specify y if and only if the model is class-conditional"
        assert timesteps is not None, "need to implement no-timestep usage"      # unet.py:520-521 (same assertion text)
        x = x.to(self.device, torch.float32).contiguous()
        t = timesteps.to(self.device, torch.int64).contiguous()
        if x.dim() != 3:
            raise ValueError(f"UNetModel expects x of shape (B, {self.x_channels}, L), got {tuple(x.shape)}")
        B, Cc, L = x.shape
        if Cc != self.x_channels:
            raise ValueError(f"UNetModel was built with in_channels={self.in_channels}"
                             + (f" of which {self.context_channels} are context" if self.context_channels else "") + f", got x with {Cc} channels")
        context = self.check_context(context, B, L)
        if tuple(t.shape) != (B,):
            raise ValueError(f"timesteps must have shape ({B},) to match the batch, got {tuple(t.shape)}")
        if B == 0:
            return torch.empty(B, self.out_channels, L, device=self.device, dtype=torch.float32)      # empty batch in, empty batch out (as the reference modules do)
        levels = len(self.channel_mult)
        if L % (1 << (levels - 1)) != 0:
            raise ValueError(f"L={L} must be divisible by {1 << (levels - 1)} (one halving per resolution level; the reference's "
                             "length-mismatch crop at unet.py:544-551 is not implemented)")
        vec = 4 if self.dtype == F32 else 8              # contiguous-dimension granularity of the MFMA operand loads
        for lvl in range(levels):
            if (1 << lvl) in self.attention_resolutions and (L >> lvl) % vec != 0:
                raise ValueError(f"attention at downsample rate {1 << lvl} sees T={L >> lvl} positions; this engine needs T to be a "
                                 f"multiple of {vec} ({'fp32' if vec == 4 else 'bf16'}): use L divisible by {vec << lvl}")
        labels = None
        if self.num_classes is not None:
            assert tuple(torch.as_tensor(y).shape) == (B,)      # unet.py:531 (same assertion)
            labels = self.check_labels(y)
        self._sync_if_stale()                            # a torch optimizer updated the flat parameter in place: refresh the compute copies
        if self.training and self._wants_graph(x):
            return _UNetFn.apply(self, x, t, labels, self._flat_param(), context)
        return self._forward_native(x, t, labels, context)

    def check_context(self, context, B, L):
        """The context of a forward of B rows as a contiguous device float32 (rows, context_channels, L) tensor with B % rows == 0 (row b
        reads context row b % rows), or None: a context model then reads zeros.  Raises ValueError before anything is launched.  A model
        built without context_channels ignores the argument, as it always did (the reference's forward takes and ignores it too); the
        samplers and train steps, whose context keywords are new, refuse it there."""
        if context is None or not self.context_channels:
            return None
        if not torch.is_tensor(context) or context.dim() != 3 or tuple(context.shape[1:]) != (self.context_channels, L):
            raise ValueError(f"context must have shape (rows, {self.context_channels}, {L}), got "
                             f"{tuple(context.shape) if torch.is_tensor(context) else type(context).__name__}")
        if context.shape[0] < 1 or B % context.shape[0] != 0:
            raise ValueError(f"{context.shape[0]} context rows cannot be shared by a batch of {B} (B % rows != 0)")
        return context.detach().to(self.device, torch.float32).contiguous()

    def check_labels(self, y):
        """Class labels as a device int64 tensor; raises IndexError (as nn.Embedding does) before anything is launched when one lies
        outside [0, num_classes)."""
        y = torch.as_tensor(y)
        if y.dtype.is_floating_point or y.dtype == torch.bool:
            raise TypeError(f"class labels must be integers, got {y.dtype}")
        if y.numel():
            lo, hi = int(y.min()), int(y.max())
            if lo < 0 or hi >= self.num_classes:
                raise IndexError(f"class label {lo if lo < 0 else hi} is out of range for num_classes={self.num_classes}")
        return y.to(self.device, torch.int64).contiguous()

    def _forward_native(self, x, t, labels=None, context=None):
        B, _c, L = x.shape
        out = torch.empty(B, self.out_channels, L, device=self.device, dtype=torch.float32)
        if context is not None:                          # the handle keeps the pointer: set for this forward, cleared behind it
            check(lib.eegldm_unet_set_context(self.h, ptr(context), context.shape[0]))
        try:
            if self.num_classes is None:
                check(lib.eegldm_unet_forward(self.h, ptr(x), ptr(t), ptr(out), B, L, 1 if self.training else 0))
            else:
                check(lib.eegldm_unet_forward_cond(self.h, ptr(x), ptr(t), ptr(labels), ptr(out), B, L, 1 if self.training else 0))
        finally:
            if context is not None:
                check(lib.eegldm_unet_set_context(self.h, None, 0))
        self._bump_tape()                                # the executor's single tape now belongs to THIS call (eegldm.autograd)
        return out

    __call__ = forward

    def backward(self, dy, need_dx=False):
        dy = dy.to(self.device, torch.float32).contiguous()
        dx = torch.empty(dy.shape[0], self.x_channels, dy.shape[2], device=self.device) if need_dx else None      # (the context gets no gradient)
        check(lib.eegldm_unet_backward(self.h, ptr(dy), ptr(dx)))
        self._bump_tape()                                # consumed
        return dx

    def __del__(self):
        try:
            lib.eegldm_unet_destroy(self.h)
        except Exception:
            pass
