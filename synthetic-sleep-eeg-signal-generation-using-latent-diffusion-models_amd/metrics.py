"""Quality metrics of reconstructed / generated windows on the device, with the interfaces the reference's
evaluation code uses:

* `MultiScaleSSIMMetric(spatial_dims=1, data_range=1.0, kernel_size=7)(y_pred, y) -> (B, 1)`
  -- /root/reference/src/compute_mmds.py:297-408 (the reference's local 1-D adaptation of MONAI's metric), call site :487-503.
* `compute_psd(windows, sfreq=100, fmax=18) -> (psds (B, n_freqs), freqs)` and `mean_psd_db`
  -- mne `Epochs.compute_psd(fmax=18)` + average + 10 log10 as used at /root/reference/src/sample_trials.py:172-181
  (multitaper, DPSS half-bandwidth 4, low-bias tapers, normalization "length").  The DPSS tapers (a few KB, once per window
  length) come from scipy on the host; everything per window runs in libeegldm (eegldm_psd_multitaper).
* `band_powers`: integrates a PSD over the classical sleep-EEG bands.
* `stft_power`, `spectrogram`, `band_course_stats`, `spindle_so_coupling`: how the spectrum moves in time, and phase-amplitude coupling
  (csrc/tfr.hip; the section "time-frequency" below).
* `row_moments`, `hjorth`, `ordinal_counts`, `permutation_entropy`, `template_match_counts`, `sample_entropy`, `complexity_features`,
  `compare_features`: how regular a window is (csrc/complexity.hip; the section "signal complexity" below).
* `USleep(...)` (forward, `train_step`, `backward`, `predict`), `fid_features(model, windows)`, `FIDMetric()(y_pred, y)`, `FeatureMoments`
* `balanced_class_weights(labels, n_classes)`, `stage_report(pred, true)`: class weights and the scores of a sleep stager (host numpy)
  -- the FID of /root/reference/src/compute_fid.py:341-419: the U-Sleep feature extractor (/root/reference/src/models/usleep.py:101-287,
  same constructor kwargs, state_dict keys and forward return value) runs in libeegldm (csrc/usleep.hip), the features' mean and
  covariance are accumulated on the device in fp64 (eegldm_feature_moments), and the 302 x 302 trace-of-square-root is host linear
  algebra in fp64 -- where monai-generative's FIDMetric (scipy.linalg.sqrtm) does it too.
"""
import ctypes as C
import functools

import numpy as np
import torch

from ._lib import lib, check, ptr, default_context, USleepCfg

BANDS = {"delta": (0.5, 4.0), "theta": (4.0, 8.0), "alpha": (8.0, 13.0), "sigma": (11.0, 16.0), "beta": (13.0, 18.0)}


def gaussian_1d(kernel_size, sigma):
    """compute_mmds.py:185-195: exp(-(d/sigma)^2/2), d = -(k-1)/2 ... (k-1)/2, normalised to sum 1."""
    dist = np.arange((1 - kernel_size) / 2, (1 + kernel_size) / 2, 1.0, dtype=np.float32)
    g = np.exp(-np.power(dist / np.float32(sigma), 2) / 2).astype(np.float32)
    return g / g.sum()


class MultiScaleSSIMMetric:
    def __init__(self, spatial_dims=1, data_range=1.0, kernel_type="gaussian", kernel_size=11, kernel_sigma=1.5, k1=0.01, k2=0.03,
                 weights=(0.0448, 0.2856, 0.3001, 0.2363, 0.1333), reduction="mean", device=0, ctx=None):
        if spatial_dims != 1:
            raise NotImplementedError("the reference evaluates 1-D windows (compute_mmds.py:487)")
        ks = int(kernel_size[0] if isinstance(kernel_size, (tuple, list)) else kernel_size)
        sg = float(kernel_sigma[0] if isinstance(kernel_sigma, (tuple, list)) else kernel_sigma)
        if str(kernel_type).lower() == "gaussian":
            self.kernel = gaussian_1d(ks, sg)
        elif str(kernel_type).lower() == "uniform":
            self.kernel = np.full(ks, 1.0 / ks, np.float32)
        else:
            raise ValueError(kernel_type)
        self.data_range, self.k1, self.k2 = float(data_range), float(k1), float(k2)
        self.weights = np.asarray(weights, np.float32)
        self.ctx = ctx or default_context(device)
        self.device = torch.device("cuda", self.ctx.device)

    def __call__(self, y_pred, y):
        if y_pred.shape != y.shape:
            raise ValueError(f"y_pred and y should have same shapes, got {y_pred.shape} and {y.shape}.")
        if y_pred.dim() != 3:
            raise ValueError(f"y_pred should have 3 dimensions (batch, channel, length) when using 1 spatial dimension, got {y_pred.dim()}.")
        a = y_pred.to(self.device, torch.float32).contiguous(); b = y.to(self.device, torch.float32).contiguous()
        B, Cc, L = a.shape
        ks, ns = len(self.kernel), len(self.weights)
        div = max(1, ns - 1) ** 2
        if L // div <= ks - 1:
            raise ValueError(f"For a given number of `weights` parameters {ns} and kernel size {ks}, the image height must be larger than "
                             f"{(ks - 1) * div}.")
        if (L >> (ns - 1)) < ks:          # 6 to 8 scales: the guard above lets a last scale shorter than the kernel through
            raise ValueError(f"For {ns} scales the last scale has {L >> (ns - 1)} samples, fewer than the kernel size {ks}.")
        out = torch.empty(B, 1, device=self.device)
        if B:
            check(lib.eegldm_ms_ssim_1d(self.ctx.h, ptr(a), ptr(b), ptr(out), B, Cc, L, (C.c_float * ks)(*self.kernel.tolist()), ks,
                                        (C.c_float * ns)(*self.weights.tolist()), ns, self.data_range, self.k1, self.k2))
        return out


@functools.lru_cache(maxsize=8)
def dpss_tapers(n_times, half_nbw=4.0, low_bias=True):
    """Tapers and weights as mne's multitaper path builds them: scipy dpss(N, NW, Kmax = int(2 NW), sym=False, norm=2), keep the tapers
    whose concentration exceeds 0.9 (low_bias), weights = sqrt(concentration)."""
    from scipy.signal.windows import dpss
    tapers, ratios = dpss(n_times, half_nbw, int(2 * half_nbw), sym=False, norm=2, return_ratios=True)
    keep = ratios > 0.9 if low_bias else np.ones_like(ratios, bool)
    if not keep.any():
        keep = np.zeros_like(ratios, bool); keep[0] = True
    return np.ascontiguousarray(tapers[keep], np.float32), np.sqrt(ratios[keep]).astype(np.float32)


def compute_psd(windows, sfreq=100.0, fmin=0.0, fmax=18.0, bandwidth=None, low_bias=True, device=0, ctx=None):
    """windows (B, 1, L) or (B, L) -> (psds (B, n_freqs) device tensor [V^2/Hz], freqs numpy)."""
    ctx = ctx or default_context(device)
    dev = torch.device("cuda", ctx.device)
    x = windows.to(dev, torch.float32)
    if x.dim() == 3:
        if x.shape[1] != 1:
            raise ValueError("single-channel windows expected")
        x = x[:, 0]
    x = x.contiguous()
    B, L = x.shape
    half_nbw = 4.0 if bandwidth is None else float(bandwidth) * L / (2.0 * sfreq)
    tapers, w = dpss_tapers(L, half_nbw, low_bias)
    freqs = np.fft.rfftfreq(L, 1.0 / sfreq)
    n_bins = int(np.searchsorted(freqs, fmax, side="right"))
    k0 = int(np.searchsorted(freqs, fmin, side="left"))
    td = torch.from_numpy(tapers).to(dev)
    psd = torch.empty(B, n_bins, device=dev)
    if B:
        check(lib.eegldm_psd_multitaper(ctx.h, ptr(x), ptr(td), (C.c_float * len(w))(*w.tolist()), len(w), float(sfreq), n_bins, ptr(psd), B, L))
    return psd[:, k0:], freqs[k0:n_bins]


def mean_psd_db(psds):
    """sample_trials.py:176-181: average the epochs' spectra, then 10 log10."""
    return 10.0 * torch.log10(psds.mean(dim=0))


def band_powers(psds, freqs, bands=None):
    """Trapezoidal integral of each window's PSD over the bands -> {band: (B,) tensor}."""
    out = {}
    f = torch.as_tensor(freqs, device=psds.device, dtype=psds.dtype)
    for name, (lo, hi) in (bands or BANDS).items():
        m = (f >= lo) & (f <= hi)
        out[name] = torch.trapezoid(psds[:, m], f[m], dim=1) if int(m.sum()) > 1 else torch.zeros(psds.shape[0], device=psds.device)
    return out


# ---------------------------------------------------------------------------------------------------- FID on U-Sleep features
class USleep:
    """Host-side mirror of /root/reference/src/models/usleep.py::USleep (constructor kwargs, `forward(x) -> (y_pred, x, bottom)`,
    state_dict keys), executing on libeegldm: the forward, and the training step of the stager (`train_step`, `forward_train` / `backward`,
    `predict`; gradients in `flat_grad`).  `train()` / `eval()` select BatchNorm on batch or running statistics; a
    freshly constructed module is in TRAIN mode like any nn.Module -- /root/reference/src/compute_fid.py:357-386 never calls
    `.eval()`, so the reference's FID features are computed with batch statistics; `fid_features` below defaults to eval mode (the
    intended use of a trained stager) and takes `batch_stats=True` to reproduce the script literally."""

    def __init__(self, in_chans=2, sfreq=128, depth=12, n_time_filters=5, complexity_factor=1.67, with_skip_connection=True, n_classes=5,
                 input_size_s=30, time_conv_size_s=9 / 128, ensure_odd_conv_size=False, apply_softmax=False, device=0, ctx=None):
        k = int(np.round(time_conv_size_s * sfreq))
        if k % 2 == 0:
            if ensure_odd_conv_size:
                k += 1
            else:
                raise ValueError("time_conv_size must be an odd number to accomodate the upsampling step in the decoder blocks.")   # usleep.py:160-163
        self.in_chans, self.depth, self.n_classes, self.apply_softmax = in_chans, depth, n_classes, apply_softmax
        self.input_size = int(np.ceil(input_size_s * sfreq))
        self.with_skip_connection = bool(with_skip_connection)
        self.ctx = ctx or default_context(device if isinstance(device, int) else torch.device(device).index or 0)
        self.device = torch.device("cuda", self.ctx.device)
        cfg = USleepCfg(in_chans, depth, n_time_filters, n_classes, k, self.input_size, 1 if with_skip_connection else 0, float(complexity_factor))
        h = C.c_void_p()
        check(lib.eegldm_usleep_create(self.ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self.channels = [int(lib.eegldm_usleep_channel(h, i)) for i in range(depth + 2)]
        self.entries = {}                      # key -> (kind, offset, numel, shape), reference state_dict order
        name = C.create_string_buffer(256)
        kind, off, numel, ndim, shape = C.c_int(), C.c_long(), C.c_long(), C.c_int(), (C.c_int * 3)()
        for i in range(int(lib.eegldm_usleep_num_entries(h))):
            check(lib.eegldm_usleep_entry(h, i, name, 256, C.byref(kind), C.byref(off), C.byref(numel), C.byref(ndim), shape))
            self.entries[name.value.decode()] = (kind.value, off.value, numel.value, tuple(shape[j] for j in range(ndim.value)))
        self.flat = torch.zeros(int(lib.eegldm_usleep_num_params(h)), device=self.device)
        self.buffers = torch.zeros(int(lib.eegldm_usleep_num_buffers(h)), device=self.device)
        check(lib.eegldm_usleep_bind(h, ptr(self.flat), ptr(self.buffers)))
        self.flat_grad = torch.zeros_like(self.flat)
        check(lib.eegldm_usleep_bind_grads(h, ptr(self.flat_grad)))
        self.training = True
        self.load_state_dict(self._default_init())

    def _default_init(self, generator=None):
        sd = {}
        for k, (_kind, _o, _n, shape) in self.entries.items():
            leaf = k.split(".")[-1]
            if leaf == "running_var" or (leaf == "weight" and len(shape) == 1):
                sd[k] = torch.ones(shape)
            elif len(shape) == 3:          # nn.Conv1d default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                sd[k] = (torch.rand(shape, generator=generator) * 2 - 1) / float(np.sqrt(shape[1] * shape[2]))
            elif leaf == "bias" and k[:-4] + "weight" in self.entries and len(self.entries[k[:-4] + "weight"][3]) == 3:
                w = self.entries[k[:-4] + "weight"][3]
                sd[k] = (torch.rand(shape, generator=generator) * 2 - 1) / float(np.sqrt(w[1] * w[2]))
            else:
                sd[k] = torch.zeros(shape, dtype=torch.int64 if leaf == "num_batches_tracked" else torch.float32)
        return sd

    def _buf(self, kind):
        return self.flat if kind == 0 else self.buffers

    def state_dict(self):
        out = {}
        for k, (kind, o, n, shape) in self.entries.items():
            v = self._buf(kind)[o:o + n].clone()
            out[k] = v.reshape(shape) if shape else v.reshape(()).round().to(torch.int64)
        return out

    def load_state_dict(self, sd, strict=True):
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        missing = [k for k in self.entries if k not in sd]; extra = [k for k in sd if k not in self.entries]
        if strict and (missing or extra):
            raise KeyError(f"state_dict mismatch: missing {missing[:4]}, unexpected {extra[:4]}")
        for k, (kind, o, n, shape) in self.entries.items():
            if k not in sd:
                continue
            v = torch.as_tensor(sd[k]).detach().to(torch.float32)
            if tuple(v.shape) != tuple(shape):
                raise ValueError(f"{k}: shape {tuple(v.shape)} != {tuple(shape)}")
            self._buf(kind)[o:o + n].copy_(v.reshape(-1).to(self.device))

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, *a, **k):
        return self

    def _decoder_len(self, T):
        """Length of the decoder output: T with the skip connections (every block is cropped to its skip); without them nothing is cropped and
        it is the bottleneck length doubled `depth` times, longer than T unless T is a multiple of 2^depth."""
        if self.with_skip_connection:
            return T
        return usleep_bottleneck_length(T, self.depth) << self.depth

    def forward(self, x, features_only=False):
        """(B, C, T) or (B, S, C, T) -> (y_pred, decoder output, bottleneck) as usleep.py:249-287; `features_only` skips the decoder and
        returns (None, None, bottleneck)."""
        x = x.to(self.device, torch.float32)
        if x.dim() == 4:                              # (B, S, C, T) -> (B, C, S * T)
            x = x.permute(0, 2, 1, 3).flatten(start_dim=2)
        if x.dim() != 3 or x.shape[1] != self.in_chans:
            raise ValueError(f"USleep expects (B, {self.in_chans}, T) or (B, S, {self.in_chans}, T), got {tuple(x.shape)}")
        x = x.contiguous(); B, _c, T = x.shape
        Lb = T
        for _ in range(self.depth):
            Lb = (Lb + (2 if Lb % 2 else 0)) // 2
        bottom = torch.empty(B, self.channels[-1], Lb, device=self.device)
        if B == 0:
            return (None, None, bottom) if features_only else (torch.empty(0, self.n_classes, device=self.device), torch.empty(0, self.channels[1], T, device=self.device), bottom)
        if features_only:
            check(lib.eegldm_usleep_forward(self.h, ptr(x), None, None, ptr(bottom), B, T, 1 if self.training else 0))
            return None, None, bottom
        if T < self.input_size:
            raise ValueError(f"T={T} is shorter than input_size={self.input_size} (the classifier's AvgPool1d window)")
        Ld = self._decoder_len(T)
        S = Ld // self.input_size
        y = torch.empty(B, self.n_classes, S, device=self.device); dec = torch.empty(B, self.channels[1], Ld, device=self.device)
        check(lib.eegldm_usleep_forward(self.h, ptr(x), ptr(y), ptr(dec), ptr(bottom), B, T, 1 if self.training else 0))
        if self.apply_softmax:
            y = torch.softmax(y, dim=1)
        if S == 1:
            y = y[:, :, 0]
        return y, dec, bottom

    # ---- training (csrc/usleep_train.hip): fp32 gradients in `flat_grad`, laid out as `flat`; eegldm.training.Adam / EMA / GradScaler
    # work on this object as on the other models
    def zero_grad(self):
        self.flat_grad.zero_()

    def sync_weights(self):
        """fp32 model: the kernels read `flat` itself."""

    def grad_dict(self):
        return {k: self.flat_grad[o:o + n].reshape(shape) for k, (kind, o, n, shape) in self.entries.items() if kind == 0}

    def _train_input(self, x):
        x = x.to(self.device, torch.float32)
        if x.dim() == 4:
            x = x.permute(0, 2, 1, 3).flatten(start_dim=2)
        if x.dim() != 3 or x.shape[1] != self.in_chans:
            raise ValueError(f"USleep expects (B, {self.in_chans}, T) or (B, S, {self.in_chans}, T), got {tuple(x.shape)}")
        B, _c, T = x.shape
        check_train_shapes(B, T, self.depth, self.input_size)
        if self._decoder_len(T) != T:
            raise ValueError(f"training without skip connections needs T to be a multiple of 2^depth = {1 << self.depth} (the logits and dx are laid out "
                             f"for a decoder output of length T; T={T} gives {self._decoder_len(T)})")
        return x.contiguous(), B, T

    def forward_train(self, x):
        """Training forward that keeps the tape for `backward`: logits (B, n_classes, S), S = T // input_size (never squeezed)."""
        x, B, T = self._train_input(x)
        y = torch.empty(B, self.n_classes, T // self.input_size, device=self.device)
        check(lib.eegldm_usleep_forward_train(self.h, ptr(x), ptr(y), B, T))
        self._tape, self._tape_x = (B, T), x          # the first conv's weight gradient reads the input: the device copy lives as long as the tape
        return y

    def backward(self, dy_pred, need_dx=False):
        """Backward of the last `forward_train` from d(logits) (B, n_classes, S): accumulates into `flat_grad`, returns dx when asked.
        Raises when there is no tape, or any other forward on this model (`forward`, `fid_features`, `predict`) ran in between."""
        tape = getattr(self, "_tape", None)
        dy = dy_pred.to(self.device, torch.float32).contiguous()
        if tape is not None and tuple(dy.reshape(dy.shape[0], self.n_classes, -1).shape) != (tape[0], self.n_classes, tape[1] // self.input_size):
            raise ValueError(f"dy_pred {tuple(dy.shape)} does not match the logits of the taped forward")
        dx = torch.empty(tape[0], self.in_chans, tape[1], device=self.device) if (need_dx and tape is not None) else None
        check(lib.eegldm_usleep_backward(self.h, ptr(dy), ptr(dx)))
        return dx

    def train_step(self, x, labels, class_weight=None, grad_scale=1.0, loss_out=None, y_pred=None):
        """Training forward -> weighted stage cross-entropy (F.cross_entropy(weight=class_weight, ignore_index=any negative label), mean
        reduction) -> backward, accumulating into `flat_grad`; returns the device scalar loss.  labels: (B,) or (B, S) integers.  Labels
        given on the host are range-checked here; labels already on the device are checked by the loss kernel, which leaves an offending
        window out and raises a flag that `label_error()` reads."""
        x, B, T = self._train_input(x)
        S = T // self.input_size
        lab = check_stage_labels(labels, B, S, self.n_classes).to(self.device).contiguous()
        cw = None
        if class_weight is not None:
            cw = torch.as_tensor(class_weight, dtype=torch.float32)
            if tuple(cw.shape) != (self.n_classes,):
                raise ValueError(f"class_weight must have shape ({self.n_classes},), got {tuple(cw.shape)}")
            cw = cw.to(self.device).contiguous()
        if loss_out is None:
            loss_out = torch.zeros(1, device=self.device)
        if y_pred is not None and (tuple(y_pred.shape) != (B, self.n_classes, S) or y_pred.dtype != torch.float32 or not y_pred.is_contiguous()):
            raise ValueError(f"y_pred must be a contiguous float32 ({B}, {self.n_classes}, {S}) tensor")
        check(lib.eegldm_usleep_train_step(self.h, ptr(x), ptr(lab), ptr(cw), B, T, float(grad_scale), ptr(loss_out), ptr(y_pred)))
        self._tape, self._tape_x = (B, T), x
        return loss_out

    def label_error(self):
        """True when a train step since the last call met a label >= n_classes in device labels (waits for the stream)."""
        out = C.c_int(0)
        check(lib.eegldm_usleep_label_error(self.h, C.byref(out)))
        return bool(out.value)

    def last_launches(self):
        return int(lib.eegldm_usleep_last_launches(self.h))

    def predict(self, windows, batch_size=256):
        """Stages of single-channel windows (N, 1, T) as `fid_features` prepares them (36-sample pads of 3072-sample loader windows cropped,
        the EEG channel duplicated when in_chans == 2), in eval mode: (stages (N,) int64, logits (N, n_classes)) on the device."""
        was = self.training
        self.eval()
        try:
            outs = []
            for i in range(0, windows.shape[0], batch_size):
                y, _d, _b = self.forward(_stager_input(self, windows[i:i + batch_size]))
                outs.append(y.reshape(y.shape[0], self.n_classes, -1)[:, :, 0])
        finally:
            self.train(was)
        logits = torch.cat(outs) if outs else torch.empty(0, self.n_classes, device=self.device)
        return logits.argmax(1), logits

    __call__ = forward

    def __del__(self):
        try:
            lib.eegldm_usleep_destroy(self.h)
        except Exception:
            pass


def fid_features(model, windows, batch_stats=False):
    """compute_fid.py:373-384: windows (B, 1, 3072) from the loader (the 36-sample pads are cropped) or (B, 1, 3000) from the sampler's
    sample_{i}.npy files -> duplicate the EEG channel into U-Sleep's two inputs -> bottleneck activation with its length-1 time axis
    squeezed: (B, c_{depth+1}) = (B, 302) for the reference configuration."""
    w = windows.to(model.device, torch.float32)
    if w.dim() != 3 or w.shape[1] != 1:
        raise ValueError(f"single-channel windows (B, 1, T) expected, got {tuple(w.shape)}")
    if w.shape[-1] == 3072:
        w = w[:, :, 36:-36]
    was = model.training
    model.train(bool(batch_stats))
    try:
        _y, _d, bottom = model.forward(torch.cat([w, w], 1), features_only=True)
    finally:
        model.train(was)
    return bottom.squeeze(-1)


def _stager_input(model, windows):
    w = windows.to(model.device, torch.float32)
    if w.dim() != 3 or w.shape[1] != 1:
        raise ValueError(f"single-channel windows (B, 1, T) expected, got {tuple(w.shape)}")
    if w.shape[-1] == 3072:
        w = w[:, :, 36:-36]
    return torch.cat([w, w], 1) if model.in_chans == 2 else w


def usleep_bottleneck_length(T, depth):
    for _ in range(depth):
        T = (T + (2 if T % 2 else 0)) // 2
    return T


def check_train_shapes(B, T, depth, input_size):
    """What a U-Sleep training step refuses, decided on the host before anything is launched."""
    if B < 1:
        raise ValueError("empty batch")
    if T < input_size:
        raise ValueError(f"T={T} is shorter than input_size={input_size} (the classifier's AvgPool1d window)")
    Lb = usleep_bottleneck_length(T, depth)
    if B * Lb < 2:
        raise ValueError(f"train-mode BatchNorm needs more than one value per channel: B={B} x bottleneck length {Lb} (torch raises here too)")


def check_stage_labels(labels, B, S, n_classes):
    """labels (B,) or (B, S) integers -> (B, S) int64.  Host labels are range-checked (negative = ignored); device labels are left to the
    loss kernel's flag, since looking at them here would wait for the device."""
    lab = torch.as_tensor(labels)
    if lab.is_floating_point() or lab.dtype == torch.bool:
        raise ValueError(f"labels must be integers, got {lab.dtype}")
    if lab.dim() == 1 and S == 1:
        lab = lab.reshape(-1, 1)
    if tuple(lab.shape) != (B, S):
        raise ValueError(f"labels must have shape ({B}, {S}), got {tuple(lab.shape)}")
    if not lab.is_cuda and lab.numel() and int(lab.max()) >= n_classes:
        raise ValueError(f"label {int(lab.max())} is out of range for n_classes={n_classes}")
    return lab.to(torch.int64)


def balanced_class_weights(labels, n_classes):
    """sklearn's class_weight='balanced': n / (n_classes * count_k) over the non-negative labels; an absent class gets 0."""
    lab = np.asarray(torch.as_tensor(labels).cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
    lab = lab[lab >= 0]
    if lab.size and int(lab.max()) >= n_classes:
        raise ValueError(f"label {int(lab.max())} is out of range for n_classes={n_classes}")
    count = np.bincount(lab.astype(np.int64), minlength=n_classes).astype(np.float64)
    w = np.zeros(n_classes, dtype=np.float64)
    w[count > 0] = lab.size / (n_classes * count[count > 0])
    return w.astype(np.float32)


def stage_report(pred, true, n_classes=5):
    """Scores of a stager on the windows whose true label is non-negative (host numpy): confusion[t][p], accuracy, balanced accuracy (mean
    recall over the classes that occur), per-class precision / recall / F1 (0 where undefined), Cohen's kappa (0 when chance agreement is 1)."""
    p = np.asarray(torch.as_tensor(pred).cpu() if isinstance(pred, torch.Tensor) else pred).reshape(-1).astype(np.int64)
    t = np.asarray(torch.as_tensor(true).cpu() if isinstance(true, torch.Tensor) else true).reshape(-1).astype(np.int64)
    if p.shape != t.shape:
        raise ValueError(f"pred {p.shape} and true {t.shape} differ in length")
    keep = t >= 0
    p, t = p[keep], t[keep]
    if p.size and (int(t.max()) >= n_classes or int(p.max()) >= n_classes or int(p.min()) < 0):
        raise ValueError(f"stage outside [0, {n_classes})")
    cm = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(cm, (t, p), 1)
    n = int(cm.sum())
    tp = np.diag(cm).astype(np.float64); row = cm.sum(1).astype(np.float64); col = cm.sum(0).astype(np.float64)

    def ratio(a, b):
        return np.divide(a, b, out=np.zeros_like(a, dtype=np.float64), where=b > 0)

    prec, rec = ratio(tp, col), ratio(tp, row)
    f1 = ratio(2 * prec * rec, prec + rec)
    acc = float(tp.sum() / n) if n else 0.0
    bal = float(rec[row > 0].mean()) if n else 0.0
    pe = float((row * col).sum() / (n * n)) if n else 0.0
    kappa = (acc - pe) / (1.0 - pe) if n and pe < 1.0 else 0.0
    return {"n": n, "confusion": cm.tolist(), "accuracy": acc, "balanced_accuracy": bal, "precision": prec.tolist(), "recall": rec.tolist(),
            "f1": f1.tolist(), "kappa": float(kappa)}


class FeatureMoments:
    """Streaming mean / unbiased covariance of feature batches, accumulated on the device in fp64 (eegldm_feature_moments) -- the
    reference concatenates every batch's features in host memory first (compute_fid.py:371-388)."""

    def __init__(self, dim, device=0, ctx=None):
        self.ctx = ctx or default_context(device)
        self.dim, self.n = int(dim), 0
        dev = torch.device("cuda", self.ctx.device)
        self.sum = torch.zeros(self.dim, dtype=torch.float64, device=dev); self.outer = torch.zeros(self.dim, self.dim, dtype=torch.float64, device=dev)

    def update(self, feats):
        f = feats.to(self.sum.device, torch.float32).contiguous()
        if f.dim() != 2 or f.shape[1] != self.dim:
            raise ValueError("Inputs should have (number images, number of features) shape.")
        if f.shape[0]:
            check(lib.eegldm_feature_moments(self.ctx.h, ptr(f), f.shape[0], self.dim, ptr(self.sum), ptr(self.outer)))
            self.n += int(f.shape[0])
        return self

    def finalize(self):
        """(mean (D,), covariance (D, D)) as float64 numpy arrays."""
        if self.n < 2:
            raise ValueError("at least two feature vectors are needed for a covariance")
        s = self.sum.cpu().numpy(); o = self.outer.cpu().numpy()
        mu = s / self.n
        return mu, (o - self.n * np.outer(mu, mu)) / (self.n - 1)


def frechet_distance(mu_x, sigma_x, mu_y, sigma_y):
    """|mu_x - mu_y|^2 + tr(S_x) + tr(S_y) - 2 tr((S_x S_y)^(1/2)).  The trace of the square root is the sum of the square roots of the
    eigenvalues of S_x S_y, which are those of the SYMMETRIC positive semi-definite matrix S_x^(1/2) S_y S_x^(1/2): two `eigh` calls in
    fp64 instead of a general (complex, ill-conditioned for rank-deficient covariances: 64 synthetic windows against 302 features in
    compute_fid.py:405) matrix square root."""
    mu_x, mu_y = np.asarray(mu_x, np.float64), np.asarray(mu_y, np.float64)
    sx, sy = np.asarray(sigma_x, np.float64), np.asarray(sigma_y, np.float64)
    w, v = np.linalg.eigh((sx + sx.T) / 2)
    root = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    m = root @ ((sy + sy.T) / 2) @ root
    ev = np.linalg.eigvalsh((m + m.T) / 2)
    d = mu_x - mu_y
    return float(d @ d + np.trace(sx) + np.trace(sy) - 2.0 * np.sqrt(np.clip(ev, 0.0, None)).sum())


class FIDMetric:
    """monai-generative's `FIDMetric()(y_pred, y)` as compute_fid.py:412-414 calls it: (N, D) feature tensors -> scalar tensor."""

    def __init__(self, device=0, ctx=None):
        self.ctx = ctx or default_context(device)

    def __call__(self, y_pred, y):
        if y_pred.dim() > 2 or y.dim() > 2:
            raise ValueError("Inputs should have (number images, number of features) shape.")
        a = FeatureMoments(y_pred.shape[1], ctx=self.ctx).update(y_pred).finalize()
        b = FeatureMoments(y.shape[1], ctx=self.ctx).update(y).finalize()
        return torch.tensor(frechet_distance(a[0], a[1], b[0], b[1]), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------- nearest neighbours on the device
# k nearest neighbours of query rows in a corpus streamed chunk by chunk (csrc/knn.hip): the memorisation audit of generated windows and
# precision / recall (Kynkaanniemi et al. 2019) / coverage (Naeem et al. 2020) on the features the FID already extracts.  Everything that
# refuses an argument does so before the device is touched.
MAX_NEIGHBOURS = 32
KNN_METRICS = ("sqeuclidean", "correlation")


def _rows2d(t, name):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    if t.dim() != 2:
        raise ValueError(f"{name}: a 2-D (rows, features) tensor is expected, got shape {tuple(t.shape)}")
    return t


def _check_k(k):
    if int(k) != k or not 1 <= int(k) <= MAX_NEIGHBOURS:
        raise ValueError(f"k must be an integer in 1..{MAX_NEIGHBOURS}, got {k!r}")
    return int(k)


def _check_dim(a, b, what):
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"{what}: feature dimensions differ ({a.shape[1]} and {b.shape[1]})")


def _dev_rows(t, dev):
    """fp32 on the device with a unit inner stride; a row stride >= D is kept, so a crop of a window stays a view."""
    t = t.to(dev, torch.float32)
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _ld(t):
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


def rows_sqnorm(x, ctx=None):
    """|x_n|^2 of the rows of a device tensor (eegldm_rows_sqnorm: fixed summation order)."""
    ctx = ctx or default_context(0)
    out = torch.empty(x.shape[0], device=x.device)
    if x.shape[0]:
        check(lib.eegldm_rows_sqnorm(ctx.h, ptr(x), _ld(x), x.shape[0], x.shape[1], ptr(out)))
    return out


def rows_standardize(x, ctx=None):
    """Rows with their mean removed and divided by their L2 norm (eegldm_rows_standardize); a constant row becomes zeros."""
    ctx = ctx or default_context(0)
    out = torch.empty(x.shape[0], x.shape[1], device=x.device)
    if x.shape[0]:
        check(lib.eegldm_rows_standardize(ctx.h, ptr(x), _ld(x), x.shape[0], x.shape[1], ptr(out), x.shape[1]))
    return out


class NearestNeighbours:
    """Running k nearest corpus rows of every query row.  `update` merges one corpus chunk (eegldm_knn_update: f32 MFMA scores with a top-k
    epilogue; no Nq x Nc matrix exists), `result` returns (dist (Nq, k) fp32, idx (Nq, k) int64), nearest first, ties by index; slots
    beyond the rows seen hold inf / -1.  metric "sqeuclidean": squared Euclidean distance; "correlation": 1 - Pearson r (both sides are
    standardised on the device).  `exclude_self_base=b`: query i is corpus row b + i and is not its own neighbour.  The result does not
    depend on how the corpus is cut into chunks, bit for bit."""

    def __init__(self, queries, k, metric="sqeuclidean", exclude_self_base=None, ctx=None):
        q = _rows2d(queries, "queries")
        self.k = _check_k(k)
        if metric not in KNN_METRICS:
            raise ValueError(f"metric must be one of {KNN_METRICS}, got {metric!r}")
        if q.shape[0] == 0 or q.shape[1] == 0:
            raise ValueError(f"empty queries: shape {tuple(q.shape)}")
        if exclude_self_base is not None and int(exclude_self_base) < 0:
            raise ValueError("exclude_self_base must be >= 0")
        self.metric, self.self_base = metric, -1 if exclude_self_base is None else int(exclude_self_base)
        self.ctx = ctx or default_context(0)
        self.device = torch.device("cuda", self.ctx.device)
        q = _dev_rows(q, self.device)
        self.nq, self.dim = int(q.shape[0]), int(q.shape[1])
        if metric == "correlation":
            self.q, self.query_sqnorm = rows_standardize(q, self.ctx), None
        else:
            self.q, self.query_sqnorm = q, rows_sqnorm(q, self.ctx)
        self.best_s = torch.full((self.nq, self.k), float("inf"), device=self.device)
        self.best_i = torch.full((self.nq, self.k), -1, dtype=torch.int64, device=self.device)
        self.seen = 0

    def _prepare(self, chunk, radius2=None):
        """-> (rows as the kernel scores them, xbias or None)"""
        x = _dev_rows(chunk, self.device)
        if self.metric == "correlation":
            return rows_standardize(x, self.ctx), None
        xb = rows_sqnorm(x, self.ctx)
        if radius2 is not None:
            xb = xb - radius2.to(self.device, torch.float32)
        return x, xb

    def _update_prepared(self, x, xbias, index_base):
        check(lib.eegldm_knn_update(self.ctx.h, ptr(self.q), _ld(self.q), ptr(x), _ld(x), ptr(xbias), self.nq, x.shape[0], self.dim, self.k,
                                    int(index_base), self.self_base, ptr(self.best_s), ptr(self.best_i)))

    def update(self, corpus_chunk, index_base=None, radius2=None):
        """Merge a chunk whose row j carries index index_base + j (default: the count of rows seen so far).  `radius2` (one value per row)
        turns the rows into balls: the score becomes d^2 - radius^2 (see `margins`)."""
        x = _rows2d(corpus_chunk, "corpus_chunk")
        if x.shape[1] != self.dim:
            raise ValueError(f"corpus_chunk has {x.shape[1]} features, the queries have {self.dim}")
        if radius2 is not None and (self.metric != "sqeuclidean" or tuple(radius2.shape) != (x.shape[0],)):
            raise ValueError("radius2 needs the sqeuclidean metric and one value per corpus row")
        base = self.seen if index_base is None else int(index_base)
        if base < 0:
            raise ValueError("index_base must be >= 0")
        if x.shape[0]:
            xs, xb = self._prepare(x, radius2)
            self._update_prepared(xs, xb, base)
        self.seen += int(x.shape[0])
        return self

    def margins(self):
        """|q_i|^2 + s: with `radius2` given to every update, d^2 - radius^2 of the nearest ball (<= 0: inside some ball)."""
        return self.query_sqnorm[:, None] + self.best_s

    def result(self, rescore=None):
        """(dist, idx).  `rescore=chunk` (index_base 0), `(chunk, index_base)` or a list of such pairs replaces the distance of every
        neighbour that lies in one of the chunks by the direct form sum (q - x)^2 (no cancellation: an exact copy gets 0) and re-sorts."""
        if self.metric == "correlation":
            dist = (1.0 + 0.5 * self.best_s).clamp_min(0.0)
        else:
            dist = self.margins().clamp_min(0.0)
        idx = self.best_i.clone()
        if rescore is None:
            return dist, idx
        pairs = rescore if isinstance(rescore, list) else [rescore if isinstance(rescore, tuple) else (rescore, 0)]
        half = self.metric == "correlation"           # standardised rows: sum (zq - zx)^2 = 2 - 2 r
        out = (2.0 * dist if half else dist).contiguous()
        for chunk, base in pairs:
            x = _rows2d(chunk, "rescore chunk")
            if x.shape[1] != self.dim:
                raise ValueError(f"rescore chunk has {x.shape[1]} features, the queries have {self.dim}")
            if x.shape[0]:
                xs, _ = self._prepare(x)
                check(lib.eegldm_knn_rescore(self.ctx.h, ptr(self.q), _ld(self.q), ptr(xs), _ld(xs), self.nq, self.dim, self.k, int(base),
                                             xs.shape[0], ptr(idx), ptr(out)))
        return _sort_pairs(0.5 * out if half else out, idx)


def _sort_pairs(dist, idx):
    """Rows re-sorted by (distance, index); empty slots (inf, -1) stay last."""
    by_index = torch.argsort(idx, dim=1, stable=True)
    dist, idx = torch.gather(dist, 1, by_index), torch.gather(idx, 1, by_index)
    by_dist = torch.argsort(dist, dim=1, stable=True)
    return torch.gather(dist, 1, by_dist), torch.gather(idx, 1, by_dist)


def knn(queries, corpus, k, metric="sqeuclidean", chunk=65536, exclude_self=False, rescore=False):
    """One-shot form: (dist, idx) of the k nearest rows of `corpus` for every row of `queries`; host tensors are streamed to the device
    `chunk` rows at a time.  `exclude_self`: queries and corpus are the same set and a row is not its own neighbour.  `rescore`: a second
    pass over the chunks replaces the distances by their direct form."""
    q, x = _rows2d(queries, "queries"), _rows2d(corpus, "corpus")
    _check_k(k)
    _check_dim(q, x, "queries / corpus")
    if exclude_self and q.shape[0] != x.shape[0]:
        raise ValueError(f"exclude_self needs the same set on both sides, got {q.shape[0]} and {x.shape[0]} rows")
    if int(chunk) < 1:
        raise ValueError("chunk must be >= 1")
    nn = NearestNeighbours(q, k, metric, exclude_self_base=0 if exclude_self else None)
    for s in range(0, x.shape[0], int(chunk)):
        nn.update(x[s:s + int(chunk)], s)
    c = int(chunk)
    return nn.result(rescore=[(x[s:s + c], s) for s in range(0, x.shape[0], c)] if rescore else None)


def kth_radius(feats, k=3, squared=False, chunk=65536):
    """Distance from every row to its k-th nearest neighbour in its own set, the row itself excluded (direct-form distances)."""
    f = _rows2d(feats, "feats")
    _check_k(k)
    if f.shape[0] <= int(k):
        raise ValueError(f"kth_radius with k = {k} needs more than {k} rows, got {f.shape[0]}")
    d2, _ = knn(f, f, k, "sqeuclidean", chunk=chunk, exclude_self=True, rescore=True)
    r2 = d2[:, int(k) - 1].contiguous()
    return r2 if squared else torch.sqrt(r2)


def prc_from_tables(fake_margin, real_margin, real_nn_d2, real_r2):
    """The three shares from the neighbour tables: fake_margin[i] = d^2 - radius^2 of the nearest real ball around fake row i (<= 0: inside),
    real_margin likewise for real rows and fake balls, real_nn_d2[j] = squared distance from real row j to its nearest fake row,
    real_r2[j] = its own squared radius."""
    fm, rm = np.asarray(fake_margin, np.float64).reshape(-1), np.asarray(real_margin, np.float64).reshape(-1)
    d2, r2 = np.asarray(real_nn_d2, np.float64).reshape(-1), np.asarray(real_r2, np.float64).reshape(-1)
    if not len(fm) or not len(rm) or len(rm) != len(d2) or len(d2) != len(r2):
        raise ValueError("neighbour tables of mismatched or zero length")
    return {"precision": float(np.mean(fm <= 0.0)), "recall": float(np.mean(rm <= 0.0)), "coverage": float(np.mean(d2 <= r2)),
            "n_real": int(len(rm)), "n_fake": int(len(fm))}


def _ball_margins(queries, corpus, radius2, chunk):
    nn = NearestNeighbours(queries, 1)
    for s in range(0, corpus.shape[0], chunk):
        nn.update(corpus[s:s + chunk], s, radius2=radius2[s:s + chunk])
    return nn.margins()[:, 0]


def precision_recall_coverage(real_feats, fake_feats, k=3, chunk=65536):
    """precision = share of fake rows inside some real ball, recall = share of real rows inside some fake ball (balls: radius = distance to
    the k-th neighbour in the own set), coverage = share of real rows whose nearest fake row lies within their own radius."""
    real, fake = _rows2d(real_feats, "real_feats"), _rows2d(fake_feats, "fake_feats")
    k = _check_k(k)
    _check_dim(real, fake, "real_feats / fake_feats")
    if real.shape[0] <= k or fake.shape[0] <= k:
        raise ValueError(f"k = {k} needs more than {k} rows on both sides, got {real.shape[0]} and {fake.shape[0]}")
    r2_real, r2_fake = kth_radius(real, k, squared=True, chunk=chunk), kth_radius(fake, k, squared=True, chunk=chunk)
    fake_margin = _ball_margins(fake, real, r2_real, chunk)
    real_margin = _ball_margins(real, fake, r2_fake, chunk)
    d2, _ = knn(real, fake, 1, "sqeuclidean", chunk=chunk, rescore=True)
    out = prc_from_tables(fake_margin.cpu().numpy(), real_margin.cpu().numpy(), d2[:, 0].cpu().numpy(), r2_real.cpu().numpy())
    out["k"] = k
    return out


# ---------------------------------------------------------------------------------------------------- memorisation audit
HOLDOUT_QUANTILES = (0.0, 0.001, 0.01, 0.05, 0.25, 0.5, 0.75, 1.0)


def lag_crops(length, lags):
    """Sample ranges of the lagged comparison: for the largest |lag| g the corpus is the centre crop [g, length - g) and a query
    contributes, per lag l, the crop [g + l, length - g + l) -> (g, (lo, hi), {lag: (lo, hi)})."""
    lags = tuple(int(l) for l in lags)
    if not lags:
        raise ValueError("at least one lag is needed (0 = no shift)")
    g = max(abs(l) for l in lags)
    if int(length) - 2 * g < 1:
        raise ValueError(f"a lag of {g} samples leaves no samples of a window of {length}")
    return g, (g, int(length) - g), {l: (g + l, int(length) - g + l) for l in lags}


def merge_lag_tables(dists, idxs, k):
    """Per query the k nearest (distance, index) pairs over all lags; an index found at several lags keeps its smallest distance."""
    d, i = np.concatenate(dists, 1), np.concatenate(idxs, 1)
    out_d, out_i = np.full((d.shape[0], k), np.inf, np.float32), np.full((d.shape[0], k), -1, np.int64)
    for r in range(d.shape[0]):
        order = np.lexsort((i[r], d[r]))
        seen, n = set(), 0
        for o in order:
            if i[r, o] < 0 or int(i[r, o]) in seen:
                continue
            seen.add(int(i[r, o])); out_d[r, n], out_i[r, n] = d[r, o], i[r, o]; n += 1
            if n == k:
                break
    return out_d, out_i


def audit_summary(syn_dist, syn_idx, holdout_dist, quantile=0.01):
    """The audit's record from the neighbour tables (numpy, (N, k)): threshold = the `quantile` of the held-out windows' nearest training
    distance, flagged = the synthetic windows nearer to a training window than that.  `holdout_rank` is the share of held-out windows that
    are nearer to the training set than the synthetic window.  No claim about what a flag means."""
    if not 0.0 <= float(quantile) <= 1.0:
        raise ValueError(f"quantile must lie in [0, 1], got {quantile}")
    sd, si, hd = np.asarray(syn_dist, np.float64), np.asarray(syn_idx, np.int64), np.asarray(holdout_dist, np.float64)
    if sd.ndim != 2 or hd.ndim != 2 or sd.shape != si.shape or not len(hd) or not len(sd):
        raise ValueError("neighbour tables must be 2-D, non-empty and of equal shape")
    h = np.sort(hd[:, 0])
    thr = float(np.quantile(h, float(quantile)))
    return {"nearest_distance": sd.tolist(), "nearest_index": si.tolist(),
            "holdout_rank": (np.searchsorted(h, sd[:, 0], side="left") / len(h)).tolist(),
            "holdout_quantiles": {str(p): float(np.quantile(h, p)) for p in HOLDOUT_QUANTILES},
            "quantile": float(quantile), "threshold": thr, "flagged": np.nonzero(sd[:, 0] < thr)[0].tolist(),
            "n_synthetic": int(len(sd)), "n_holdout": int(len(hd))}


def _windows2d(w, name):
    """(N, L) or (N, 1, L) -> (N, L); the loader's 3072-sample windows lose their 36-sample zero pads (as in fid_features)."""
    if not torch.is_tensor(w):
        w = torch.as_tensor(np.asarray(w))
    if w.dim() == 3 and w.shape[1] == 1:
        w = w[:, 0]
    if w.dim() != 2:
        raise ValueError(f"{name}: windows (N, L) or (N, 1, L) expected, got shape {tuple(w.shape)}")
    if w.shape[1] == 3072:
        w = w[:, 36:-36]
    return w


def memorisation_audit(synthetic, train_chunks, holdout, space="signal", k=1, lags=(0,), quantile=0.01, usleep=None, batch_size=256):
    """Where do the synthetic windows sit, by their distance to the nearest training window, in the distribution of that same distance
    for held-out real windows?  `train_chunks`: an iterable of window batches (the training set is streamed once).  space "signal":
    1 - Pearson r on the samples, minimum over the sample offsets `lags`; "features": squared Euclidean distance on `fid_features` of
    `usleep`.  Returns `audit_summary`'s dict plus the settings."""
    syn, hold = _windows2d(synthetic, "synthetic"), _windows2d(holdout, "holdout")
    k = _check_k(k)
    if space not in ("signal", "features"):
        raise ValueError(f"space must be 'signal' or 'features', got {space!r}")
    if syn.shape[0] == 0 or hold.shape[0] == 0:
        raise ValueError("empty queries: the audit needs synthetic and held-out windows")
    _check_dim(syn, hold, "synthetic / holdout")
    if not 0.0 <= float(quantile) <= 1.0:
        raise ValueError(f"quantile must lie in [0, 1], got {quantile}")
    _g, (c_lo, c_hi), crops = lag_crops(syn.shape[1], lags)
    if space == "features":
        if tuple(crops) != (0,):
            raise ValueError("lags apply to space='signal' only")
        if usleep is None:
            raise ValueError("space='features' needs the U-Sleep feature extractor (usleep=)")
    ns = int(syn.shape[0])
    if space == "signal":
        dev = torch.device("cuda", default_context(0).device)
        queries = torch.cat([syn.to(dev, torch.float32), hold.to(dev, torch.float32)], 0)
        searches = {l: NearestNeighbours(queries[:, lo:hi], k, "correlation") for l, (lo, hi) in crops.items()}
        base = 0
        for chunk in train_chunks:
            x = _windows2d(chunk, "train chunk")
            _check_dim(syn, x, "synthetic / train chunk")
            if not x.shape[0]:
                continue
            xs = rows_standardize(_dev_rows(x.to(dev, torch.float32)[:, c_lo:c_hi], dev))
            for nn in searches.values():
                nn._update_prepared(xs, None, base)
            base += int(x.shape[0])
        tables = [nn.result() for nn in searches.values()]
        if len(tables) == 1:
            dist, idx = tables[0][0].cpu().numpy(), tables[0][1].cpu().numpy()
        else:
            dist, idx = merge_lag_tables([t[0].cpu().numpy() for t in tables], [t[1].cpu().numpy() for t in tables], k)
    else:
        def feats(w):
            return torch.cat([fid_features(usleep, w[s:s + batch_size].unsqueeze(1)) for s in range(0, w.shape[0], batch_size)], 0)
        nn = NearestNeighbours(torch.cat([feats(syn), feats(hold)], 0), k, "sqeuclidean")
        for chunk in train_chunks:
            x = _windows2d(chunk, "train chunk")
            _check_dim(syn, x, "synthetic / train chunk")
            if x.shape[0]:
                nn.update(feats(x))
        base = nn.seen
        dist, idx = (t.cpu().numpy() for t in nn.result())
    if base == 0:
        raise ValueError("no training windows were given")
    out = audit_summary(dist[:ns], idx[:ns], dist[ns:], quantile)
    out.update({"space": space, "metric": "1 - pearson r" if space == "signal" else "squared euclidean distance of U-Sleep features",
                "k": k, "lags": [int(l) for l in crops], "n_train": int(base)})
    return out


# ---------------------------------------------------------------------------------------------------- kernel two-sample statistics
# MMD^2 (Gretton et al. 2012), KID (Binkowski et al. 2018: the unbiased MMD^2 under the cubic kernel (<a, b> / D + 1)^3), a permutation
# p-value and the MMD witness function, all as float64 algebra on R = K(A, B) V (csrc/kmm.hip, eegldm_kernel_matmul): the kernel matrix
# never exists, the weights V are indicator columns.  The functions that turn R into statistics take R as input and run anywhere;
# everything that refuses an argument does so before the device is touched.
KMM_NO_DIAG = -(1 << 63)
KMM_MAX_COLS, KMM_MAX_SIGMAS = 64, 8
KMM_KERNELS = ("poly", "rbf")


def rbf_betas(sigmas):
    """beta = 1 / (2 sigma^2) as the fp32 values the kernel multiplies by."""
    s = np.asarray(sigmas, np.float64).reshape(-1)
    if not 1 <= s.size <= KMM_MAX_SIGMAS:
        raise ValueError(f"sigmas must hold 1..{KMM_MAX_SIGMAS} bandwidths, got {s.size}")
    if not np.all(s > 0):                  # a NaN fails too
        raise ValueError(f"sigmas must be positive, got {s.tolist()}")
    return (1.0 / (2.0 * s * s)).astype(np.float32)


def _check_kernel(kernel, degree, sigmas):
    if kernel not in KMM_KERNELS:
        raise ValueError(f"kernel must be one of {KMM_KERNELS}, got {kernel!r}")
    if kernel == "poly" and (int(degree) != degree or not 1 <= int(degree) <= 4):
        raise ValueError(f"degree must be an integer in 1..4, got {degree!r}")
    if kernel == "rbf" and sigmas is not None:
        rbf_betas(sigmas)


def _check_two_sets(x, y, names=("x", "y"), min_rows=2):
    x, y = _rows2d(x, names[0]), _rows2d(y, names[1])
    _check_dim(x, y, " / ".join(names))
    if x.shape[1] < 1:
        raise ValueError("rows without features")
    for t, n in zip((x, y), names):
        if t.shape[0] < min_rows:
            raise ValueError(f"{n}: at least {min_rows} rows are needed, got {t.shape[0]}")
    return x, y


def median_bandwidth(x, y, max_rows=1024, seed=0, ctx=None):
    """Median pairwise Euclidean distance of a seeded subsample of the pooled rows (torch on the device): the usual scale of an rbf kernel."""
    x, y = _check_two_sets(x, y, min_rows=1)
    if int(max_rows) < 2:
        raise ValueError("max_rows must be >= 2")
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    n, m = int(x.shape[0]), int(y.shape[0])
    pick = np.sort(np.random.default_rng(seed).choice(n + m, min(n + m, int(max_rows)), replace=False))
    z = torch.cat([x[torch.from_numpy(pick[pick < n])].to(dev, torch.float32), y[torch.from_numpy(pick[pick >= n] - n)].to(dev, torch.float32)], 0)
    if z.shape[0] < 2:
        raise ValueError("a bandwidth needs at least two rows")
    d = torch.cdist(z.double(), z.double())
    iu = torch.triu_indices(z.shape[0], z.shape[0], 1, device=dev)
    return float(d[iu[0], iu[1]].median())


def _default_sigmas(kernel, sigmas, x, y, ctx):
    if kernel != "rbf" or sigmas is not None:
        return sigmas
    med = median_bandwidth(x, y, ctx=ctx)
    if not med > 0.0:
        raise ValueError("the median pairwise distance is zero: give sigmas")
    return (0.5 * med, med, 2.0 * med)


def kernel_matmul(a, b, v, kernel="poly", degree=3, gamma=None, coef0=1.0, sigmas=None, diag_off=None, chunk=65536, ctx=None):
    """R = K(a, b) v as (Na, P) float64 on the device, any P (columns go to the device 64 at a time), b and v streamed `chunk` rows at a
    time.  poly: k = (gamma <a, b> + coef0)^degree, gamma None = 1 / D; rbf: the mean over `sigmas` of exp(-|a - b|^2 / (2 sigma^2)),
    sigmas None = (0.5, 1, 2) x `median_bandwidth(a, b)`.  `diag_off=d` leaves the pairs with j - i == d out (0: a set against itself
    without its diagonal)."""
    a, b = _check_two_sets(a, b, ("a", "b"), min_rows=0)
    v = _rows2d(v, "v")
    if v.shape[0] != b.shape[0]:
        raise ValueError(f"v has {v.shape[0]} rows, b has {b.shape[0]}")
    if a.shape[0] < 1 or v.shape[1] < 1:
        raise ValueError(f"empty problem: a {tuple(a.shape)}, v {tuple(v.shape)}")
    _check_kernel(kernel, degree, sigmas)
    if int(chunk) < 1:
        raise ValueError("chunk must be >= 1")
    chunk = int(chunk)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    sigmas = _default_sigmas(kernel, sigmas, a, b, ctx)
    na, nb, d, ptot = int(a.shape[0]), int(b.shape[0]), int(a.shape[1]), int(v.shape[1])
    rbf = kernel == "rbf"
    betas = rbf_betas(sigmas) if rbf else np.zeros(1, np.float32)
    betas_c = (C.c_float * len(betas))(*betas.tolist())
    g = 1.0 / d if gamma is None else float(gamma)
    ad = _dev_rows(a, dev)
    asq = rows_sqnorm(ad, ctx) if rbf else None
    out = torch.zeros(na, ptot, dtype=torch.float64, device=dev)
    for s in range(0, nb, chunk):
        bd, vd = _dev_rows(b[s:s + chunk], dev), _dev_rows(v[s:s + chunk], dev)
        bsq = rows_sqnorm(bd, ctx) if rbf else None
        off = KMM_NO_DIAG if diag_off is None else int(diag_off) - s
        for c in range(0, ptot, KMM_MAX_COLS):
            vc, oc = vd[:, c:c + KMM_MAX_COLS], out[:, c:c + KMM_MAX_COLS]
            check(lib.eegldm_kernel_matmul(ctx.h, ptr(ad), _ld(ad), ptr(asq), ptr(bd), _ld(bd), ptr(bsq), ptr(vc), _ld(vd), na, int(bd.shape[0]), d,
                                           int(vc.shape[1]), 1 if rbf else 0, int(degree), g, float(coef0), betas_c, len(betas), off,
                                           1 if s else 0, ptr(oc), ptot))
    return out


def subset_indicators(n, size, count, rng):
    """(n, count) fp32 0/1 columns, each with `size` ones drawn without replacement from `rng`."""
    if not 1 <= int(size) <= int(n):
        raise ValueError(f"a subset of {size} rows out of {n}")
    out = np.zeros((int(n), int(count)), np.float32)
    for c in range(int(count)):
        out[rng.choice(int(n), int(size), replace=False), c] = 1.0
    return out


def permutation_indicators(n, m, n_perm, seed=0):
    """(n + m, n_perm + 2) fp32: column 0 marks the first n pooled rows (the observed split), columns 1..n_perm the first n entries of
    seeded permutations of the pool, the last column is all ones."""
    if int(n_perm) < 1:
        raise ValueError(f"n_perm must be >= 1, got {n_perm}")
    if n < 2 or m < 2:
        raise ValueError("at least 2 rows per set are needed")
    rng = np.random.default_rng(seed)
    out = np.zeros((n + m, int(n_perm) + 2), np.float32)
    out[:n, 0] = 1.0
    for c in range(1, int(n_perm) + 1):
        out[rng.permutation(n + m)[:n], c] = 1.0
    out[:, -1] = 1.0
    return out


def mmd2_from_sums(sxx, syy, sxy, n, m, unbiased=True):
    """sxx / syy: the sums of k over the pairs inside each set (unbiased: without the diagonal; biased: with it), sxy: over all cross pairs."""
    kxx = float(sxx) / (n * (n - 1) if unbiased else n * n)
    kyy = float(syy) / (m * (m - 1) if unbiased else m * m)
    kxy = float(sxy) / (n * m)
    return {"mmd2": kxx + kyy - 2.0 * kxy, "kxx": kxx, "kyy": kyy, "kxy": kxy, "n": int(n), "m": int(m)}


def kid_from_r(ind_x, ind_y, r_xx, r_yy, r_xy):
    """Per-subset unbiased MMD^2 from r_xx = K°(x, x) ind_x, r_yy = K°(y, y) ind_y, r_xy = K(x, y) ind_y (K°: zero diagonal)."""
    ax, ay = np.asarray(ind_x, np.float64), np.asarray(ind_y, np.float64)
    kx, ky = ax.sum(0), ay.sum(0)
    sxx = (ax * np.asarray(r_xx, np.float64)).sum(0); syy = (ay * np.asarray(r_yy, np.float64)).sum(0)
    sxy = (ax * np.asarray(r_xy, np.float64)).sum(0)
    return sxx / (kx * (kx - 1)) + syy / (ky * (ky - 1)) - 2.0 * sxy / (kx * ky)


def permutation_stats_from_r(ind, r, n, m):
    """Unbiased MMD^2 of every split in `ind` (`permutation_indicators`) from r = K°(z, z) ind, z = [x; y]: with a a column and 1 the last,
    a^T K° a = sum a_i r_i, a^T K° b = a^T K° 1 - a^T K° a, b^T K° b = 1^T K° 1 - 2 a^T K° 1 + a^T K° a -> (n_perm + 1,), observed first."""
    a, r = np.asarray(ind, np.float64)[:, :-1], np.asarray(r, np.float64)
    aka = (a * r[:, :-1]).sum(0)
    ak1 = (a * r[:, -1:]).sum(0)
    k11 = r[:, -1].sum()
    akb = ak1 - aka
    bkb = k11 - 2.0 * ak1 + aka
    return aka / (n * (n - 1)) + bkb / (m * (m - 1)) - 2.0 * akb / (n * m)


def permutation_p_value(observed, null):
    """(1 + #{null >= observed}) / (1 + n_perm): never 0, valid at any n_perm (Phipson & Smyth 2010)."""
    null = np.asarray(null, np.float64).reshape(-1)
    return (1.0 + float(np.sum(null >= observed))) / (1.0 + null.size)


def mmd2(x, y, kernel="poly", degree=3, gamma=None, coef0=1.0, sigmas=None, unbiased=True, chunk=65536, ctx=None):
    """MMD^2 between the row sets -> {"mmd2", "kxx", "kyy", "kxy", "n", "m"}.  unbiased: the within-set means leave the diagonal out in the
    kernel (`diag_off`); it is never summed and subtracted."""
    x, y = _check_two_sets(x, y)
    _check_kernel(kernel, degree, sigmas)
    ctx = ctx or default_context(0)
    sigmas = _default_sigmas(kernel, sigmas, x, y, ctx)
    kw = dict(kernel=kernel, degree=degree, gamma=gamma, coef0=coef0, sigmas=sigmas, chunk=chunk, ctx=ctx)
    n, m = int(x.shape[0]), int(y.shape[0])
    ones_n, ones_m = torch.ones(n, 1), torch.ones(m, 1)
    d = 0 if unbiased else None
    sxx = kernel_matmul(x, x, ones_n, diag_off=d, **kw).sum().item()
    syy = kernel_matmul(y, y, ones_m, diag_off=d, **kw).sum().item()
    sxy = kernel_matmul(x, y, ones_m, **kw).sum().item()
    return mmd2_from_sums(sxx, syy, sxy, n, m, unbiased)


def kid(real, fake, subsets=100, subset_size=1000, seed=0, chunk=65536, ctx=None):
    """Kernel inception distance: mean and standard deviation of the unbiased cubic-kernel MMD^2 over `subsets` seeded subsets of
    min(subset_size, n, m) rows of each set -> {"kid_mean", "kid_std", "per_subset", "subset_size"}."""
    x, y = _check_two_sets(real, fake, ("real", "fake"))
    if int(subsets) < 1 or int(subset_size) < 2:
        raise ValueError(f"subsets must be >= 1 and subset_size >= 2, got {subsets} and {subset_size}")
    size = min(int(subset_size), int(x.shape[0]), int(y.shape[0]))
    rng = np.random.default_rng(seed)
    ix, iy = subset_indicators(x.shape[0], size, subsets, rng), subset_indicators(y.shape[0], size, subsets, rng)
    kw = dict(kernel="poly", degree=3, gamma=None, coef0=1.0, chunk=chunk, ctx=ctx)
    r_xx = kernel_matmul(x, x, torch.from_numpy(ix), diag_off=0, **kw).cpu().numpy()
    r_yy = kernel_matmul(y, y, torch.from_numpy(iy), diag_off=0, **kw).cpu().numpy()
    r_xy = kernel_matmul(x, y, torch.from_numpy(iy), **kw).cpu().numpy()
    per = kid_from_r(ix, iy, r_xx, r_yy, r_xy)
    return {"kid_mean": float(per.mean()), "kid_std": float(per.std()), "per_subset": per.tolist(), "subset_size": size}


def mmd_permutation_test(x, y, n_perm=1000, seed=0, kernel="poly", degree=3, gamma=None, coef0=1.0, sigmas=None, chunk=65536, ctx=None):
    """Kernel two-sample test: the unbiased MMD^2 of (x, y) against its values under `n_perm` seeded relabellings of the pooled rows
    -> {"mmd2", "p_value", "null", "n_perm"}.  A large p-value is not evidence that the sets are equal."""
    x, y = _check_two_sets(x, y)
    _check_kernel(kernel, degree, sigmas)
    n, m = int(x.shape[0]), int(y.shape[0])
    ind = permutation_indicators(n, m, n_perm, seed)
    ctx = ctx or default_context(0)
    sigmas = _default_sigmas(kernel, sigmas, x, y, ctx)
    z = torch.cat([x.to(torch.float32).cpu(), y.to(torch.float32).cpu()], 0) if not (x.is_cuda and y.is_cuda) else torch.cat([x.float(), y.float()], 0)
    r = kernel_matmul(z, z, torch.from_numpy(ind), kernel=kernel, degree=degree, gamma=gamma, coef0=coef0, sigmas=sigmas, diag_off=0,
                      chunk=chunk, ctx=ctx).cpu().numpy()
    stats = permutation_stats_from_r(ind, r, n, m)
    return {"mmd2": float(stats[0]), "p_value": permutation_p_value(stats[0], stats[1:]), "null": stats[1:].tolist(), "n_perm": int(n_perm)}


def witness_from_r(r_x, r_y, n, m):
    return np.asarray(r_x, np.float64).reshape(-1) / n - np.asarray(r_y, np.float64).reshape(-1) / m


def mmd_witness(points, x, y, kernel="poly", degree=3, gamma=None, coef0=1.0, sigmas=None, chunk=65536, ctx=None):
    """MMD witness function at `points`: mean_j k(p, x_j) - mean_j k(p, y_j) as (N,) float64 numpy; negative where a point looks more like
    y than like x."""
    x, y = _check_two_sets(x, y)
    p, _x = _check_two_sets(points, x, ("points", "x"), min_rows=1)
    _check_kernel(kernel, degree, sigmas)
    ctx = ctx or default_context(0)
    sigmas = _default_sigmas(kernel, sigmas, x, y, ctx)
    kw = dict(kernel=kernel, degree=degree, gamma=gamma, coef0=coef0, sigmas=sigmas, chunk=chunk, ctx=ctx)
    n, m = int(x.shape[0]), int(y.shape[0])
    r_x = kernel_matmul(p, x, torch.ones(n, 1), **kw).cpu().numpy()
    r_y = kernel_matmul(p, y, torch.ones(m, 1), **kw).cpu().numpy()
    return witness_from_r(r_x, r_y, n, m)


# ---------------------------------------------------------------------------------------------------- sleep micro-structure
# Spindles (band-pass, RMS envelope, threshold, duration gate) and slow waves (low-pass, zero-crossing half-waves, duration and amplitude
# gate) on two device primitives (csrc/events.hip): eegldm_fir_same, a zero-phase FIR filter over rows of windows, and
# eegldm_threshold_events, the runs of a row above a threshold with per-event features.  Everything that is not a pass over the windows is
# float64 numpy in functions that take tables as input; everything that refuses an argument does so before the device is touched.
# THE DETECTOR DEFAULTS ARE THE LITERATURE'S FOR SCALP EEG; NOBODY HAS VALIDATED THEM ON THIS PROJECT'S 18-Hz-LOW-PASSED DATA.
FIR_MAX_TAPS, FIR_MAX_LEN, EVENTS_MAX = 2049, 4096, 64
FIR_EDGES = {"zero": 0, "reflect": 1}
EVENT_INT_FIELDS = ("start", "length", "argmax", "n_up", "n_raw", "flags")
EVENT_FLOAT_FIELDS = ("peak", "sum", "aux_max", "aux_min")
SUMMARY_FEATURES = ("duration_s", "amplitude", "freq_hz")


def fir_length(sfreq, trans_hz):
    """Taps of a Hamming-windowed sinc with transition width trans_hz: the smallest odd integer >= 3.3 sfreq / trans_hz."""
    if not (sfreq > 0 and trans_hz > 0):                     # a NaN fails too
        raise ValueError(f"sfreq and trans_hz must be positive, got {sfreq} and {trans_hz}")
    m = int(np.ceil(3.3 * float(sfreq) / float(trans_hz)))
    return m + 1 - m % 2


def fir_design(sfreq, lo=None, hi=None, trans_hz=2.0):
    """(M,) float64 taps of a zero-phase (symmetric, odd-length) windowed-sinc filter with a Hamming window: low-pass (hi), high-pass (lo) or
    band-pass (lo, hi), cut-offs in Hz at the half-amplitude points, scaled to unit gain at DC (low-pass), at the band centre (band-pass) or
    at Nyquist (high-pass): scipy.signal.firwin(M, ..., window="hamming", fs=sfreq) in plain numpy."""
    m = fir_length(sfreq, trans_hz)
    nyq = 0.5 * float(sfreq)
    if lo is None and hi is None:
        raise ValueError("give lo (high-pass), hi (low-pass) or both (band-pass)")
    for name, f in (("lo", lo), ("hi", hi)):
        if f is not None and not 0.0 < float(f) < nyq:
            raise ValueError(f"{name} = {f} Hz must lie strictly between 0 and sfreq / 2 = {nyq}")
    if lo is not None and hi is not None and not float(lo) < float(hi):
        raise ValueError(f"band ({lo}, {hi}) Hz: lo must be below hi")
    if m > FIR_MAX_TAPS:
        raise ValueError(f"trans_hz = {trans_hz} at sfreq = {sfreq} needs {m} taps, eegldm_fir_same takes at most {FIR_MAX_TAPS}")
    left = 0.0 if lo is None else float(lo) / nyq
    right = 1.0 if hi is None else float(hi) / nyq
    k = np.arange(m, dtype=np.float64) - 0.5 * (m - 1)
    h = (right * np.sinc(right * k) - left * np.sinc(left * k)) * np.hamming(m)
    centre = 0.0 if left == 0.0 else (1.0 if right == 1.0 else 0.5 * (left + right))
    return h / np.sum(h * np.cos(np.pi * k * centre))


def _check_taps(taps, length, edge):
    t = np.asarray(taps, np.float64).reshape(-1)
    if edge not in FIR_EDGES:
        raise ValueError(f"edge must be one of {tuple(FIR_EDGES)}, got {edge!r}")
    if not 1 <= t.size <= FIR_MAX_TAPS or t.size % 2 == 0:
        raise ValueError(f"an odd number of taps in 1..{FIR_MAX_TAPS} is needed, got {t.size}")
    with np.errstate(over="ignore"):
        finite = np.all(np.isfinite(t.astype(np.float32)))          # as uploaded: a float64 tap beyond fp32's range is an inf on the device
    if not finite:
        raise ValueError("non-finite taps (as fp32)")
    if not 1 <= int(length) <= FIR_MAX_LEN:
        raise ValueError(f"windows of 1..{FIR_MAX_LEN} samples are taken, got {length}")
    if edge == "reflect" and (t.size - 1) // 2 > int(length) - 1:
        raise ValueError(f"reflect needs (M - 1) / 2 <= L - 1, got {t.size} taps for windows of {length} samples")
    return t


def _rows_any_length(w, name):
    """(N, L) or (N, 1, L) -> (N, L), nothing cropped."""
    if not torch.is_tensor(w):
        w = torch.as_tensor(np.asarray(w))
    if w.dim() == 3 and w.shape[1] == 1:
        w = w[:, 0]
    if w.dim() != 2:
        raise ValueError(f"{name}: windows (N, L) or (N, 1, L) expected, got shape {tuple(w.shape)}")
    return w


def fir_filter(windows, taps, edge="zero", rms=False, ctx=None):
    """Zero-phase FIR over every window: (N, L) fp32 on the device.  y[n] = sum_k taps[k] xe[n + k - (M - 1) / 2], xe the window extended by
    zeros ("zero") or by whole-sample reflection ("reflect"); rms=True squares every sample on the way in and returns sqrt(max(sum, 0)): with
    box taps 1 / W the moving RMS.  Windows (N, L) or (N, 1, L), L <= 4096, are filtered as they are (no pad is cropped)."""
    w = _rows_any_length(windows, "windows")
    t = _check_taps(taps, w.shape[1], edge)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    x = _dev_rows(w, dev)
    out = torch.empty(x.shape[0], x.shape[1], device=dev)
    if x.shape[0]:
        td = torch.from_numpy(t.astype(np.float32)).to(dev)
        check(lib.eegldm_fir_same(ctx.h, ptr(x), _ld(x), ptr(td), int(t.size), ptr(out), int(x.shape[1]), int(x.shape[0]), int(x.shape[1]),
                                  FIR_EDGES[edge], 1 if rms else 0))
    return out


def rms_box(rms_s, sfreq):
    """Box taps of the moving RMS: W = round(rms_s sfreq) samples, made odd by adding one, gain 1 / W."""
    w = int(round(float(rms_s) * float(sfreq)))
    if w < 1:
        raise ValueError(f"rms_s = {rms_s} s is shorter than a sample at sfreq = {sfreq}")
    w += 1 - w % 2
    return np.full(w, 1.0 / w)


def band_envelope(windows, lo, hi, sfreq=100.0, rms_s=0.2, trans_hz=2.0, ctx=None):
    """(band, env): the windows band-passed to (lo, hi) Hz and the moving RMS of that over rms_s seconds, both (N, L) fp32 on the device,
    edges by reflection.  The loader's 3072-sample windows lose their zero pads first."""
    w = _windows2d(windows, "windows")
    taps, box = fir_design(sfreq, lo, hi, trans_hz), rms_box(rms_s, sfreq)
    _check_taps(taps, w.shape[1], "reflect"); _check_taps(box, w.shape[1], "reflect")
    band = fir_filter(w, taps, "reflect", ctx=ctx)
    return band, fir_filter(band, box, "reflect", rms=True, ctx=ctx)


def _check_events_args(length, min_len, max_len, merge_gap, max_events):
    if not 1 <= int(length) <= FIR_MAX_LEN:
        raise ValueError(f"rows of 1..{FIR_MAX_LEN} samples are taken, got {length}")
    if int(max_events) != max_events or not 1 <= int(max_events) <= EVENTS_MAX:
        raise ValueError(f"max_events must be an integer in 1..{EVENTS_MAX}, got {max_events!r}")
    if int(min_len) < 1 or int(max_len) < int(min_len) or int(merge_gap) < 0:
        raise ValueError(f"need 1 <= min_len <= max_len and merge_gap >= 0, got {min_len}, {max_len}, {merge_gap}")


def threshold_events(s, thr, aux=None, min_len=1, max_len=None, merge_gap=0, drop_edge=False, max_events=32, ctx=None):
    """Runs of every row of s (N, L) above thr (a float or (N,)) after closing gaps of at most merge_gap samples, kept when min_len <= length
    <= max_len (and, with drop_edge, when they touch no row end), with features (eegldm_threshold_events; include/eegldm.h has the
    definition).  Returns numpy tables: n_events (N,) all kept events, n_raw_runs (N,), stored (N, E) bool, and per stored event (N, E)
    start, length, argmax, n_up, n_raw, flags (int32), peak, sum, aux_max, aux_min (fp32); slots past the stored events are zero."""
    s = _rows_any_length(s, "s")
    n, length = int(s.shape[0]), int(s.shape[1])
    max_len = length if max_len is None else max_len
    _check_events_args(length, min_len, max_len, merge_gap, max_events)
    if aux is not None:
        aux = _rows_any_length(aux, "aux")
        if tuple(aux.shape) != tuple(s.shape):
            raise ValueError(f"aux {tuple(aux.shape)} does not match s {tuple(s.shape)}")
    thr_a = np.asarray(thr.detach().cpu().numpy() if torch.is_tensor(thr) else thr, np.float32)
    if thr_a.ndim == 0:
        thr_a = np.full(n, thr_a, np.float32)
    if thr_a.shape != (n,):
        raise ValueError(f"thr must be a float or ({n},), got shape {thr_a.shape}")
    e = int(max_events)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    sd = _dev_rows(s, dev)
    ad = None if aux is None else _dev_rows(aux, dev)
    counts = torch.zeros(n, 2, dtype=torch.int32, device=dev)
    ev_i = torch.zeros(n, e, 6, dtype=torch.int32, device=dev)
    ev_f = torch.zeros(n, e, 4, dtype=torch.float32, device=dev)
    if n:
        td = torch.from_numpy(thr_a).to(dev)
        check(lib.eegldm_threshold_events(ctx.h, ptr(sd), _ld(sd), ptr(ad), _ld(ad) if ad is not None else 0, ptr(td), n, length, int(min_len),
                                          int(max_len), int(merge_gap), 1 if drop_edge else 0, e, ptr(counts), ptr(ev_i), ptr(ev_f)))
    return events_from_tables(counts.cpu().numpy(), ev_i.cpu().numpy(), ev_f.cpu().numpy())


def events_from_tables(counts, ev_i, ev_f):
    """The export's three tables as a dict of named numpy tables (see `threshold_events`)."""
    counts, ev_i, ev_f = np.asarray(counts), np.asarray(ev_i), np.asarray(ev_f)
    e = ev_i.shape[1]
    out = {"n_events": counts[:, 0].copy(), "n_raw_runs": counts[:, 1].copy(),
           "stored": np.arange(e)[None, :] < np.minimum(counts[:, :1], e)}
    for k, name in enumerate(EVENT_INT_FIELDS):
        out[name] = ev_i[:, :, k].copy()
    for k, name in enumerate(EVENT_FLOAT_FIELDS):
        out[name] = ev_f[:, :, k].copy()
    return out


def event_table(ev, sfreq=100.0):
    """One row per stored event, in window order then start order: window, the export's fields, duration_s and mid_s (the run's midpoint);
    `truncated` counts the windows that had more events than slots."""
    win, slot = np.nonzero(ev["stored"])
    t = {"window": win.astype(np.int64)}
    for name in EVENT_INT_FIELDS + EVENT_FLOAT_FIELDS:
        t[name] = ev[name][win, slot]
    t["duration_s"] = t["length"].astype(np.float64) / float(sfreq)
    t["mid_s"] = (t["start"].astype(np.float64) + 0.5 * t["length"]) / float(sfreq)
    t["sfreq"] = float(sfreq)
    t["n_windows"] = int(ev["stored"].shape[0])
    t["truncated"] = int(np.sum(ev["n_events"] > ev["stored"].shape[1]))
    return t


def _seconds_to_samples(sfreq, **kw):
    out = {}
    for k, v in kw.items():
        if not (v >= 0):
            raise ValueError(f"{k} = {v} s must be non-negative")
        out[k] = int(round(float(v) * float(sfreq)))
    return out


def envelope_threshold(real_windows, factor=1.5, band=(11.0, 16.0), batch_size=4096, **band_kw):
    """ONE absolute threshold for the spindle detector: mean + factor * std (float64, population) of the band envelope over every sample of the
    REAL set.  It is taken from the real set and applied to both sets: a per-window threshold invents events in windows that have none.
    `band` defaults to `detect_spindles`' band; band_kw are `band_envelope`'s other keywords (sfreq, rms_s, trans_hz; lo / hi override band)."""
    if len(band) != 2:
        raise ValueError(f"band must be (lo, hi), got {band!r}")
    lo, hi = band_kw.pop("lo", band[0]), band_kw.pop("hi", band[1])
    w = _windows2d(real_windows, "real_windows")
    if w.shape[0] < 1:
        raise ValueError("no real windows")
    if not np.isfinite(factor):
        raise ValueError(f"factor must be finite, got {factor}")
    n, s1, s2 = 0, 0.0, 0.0
    for i in range(0, w.shape[0], int(batch_size)):
        env = band_envelope(w[i:i + int(batch_size)], lo, hi, **band_kw)[1].double()
        n += env.numel(); s1 += float(env.sum()); s2 += float((env * env).sum())
    mean = s1 / n
    return mean + float(factor) * float(np.sqrt(max(s2 / n - mean * mean, 0.0)))


def detect_spindles(windows, thr, sfreq=100.0, band=(11.0, 16.0), rms_s=0.2, min_s=0.5, max_s=3.0, merge_s=0.1, drop_edge=True, trans_hz=2.0,
                    max_events=32, ctx=None):
    """Sleep spindles by the classical amplitude criterion: band-pass to `band`, moving RMS over rms_s, runs of the envelope above the absolute
    threshold `thr` (see `envelope_threshold`), gaps up to merge_s closed, duration in [min_s, max_s].  Returns `event_table` plus freq_hz =
    upward zero crossings of the band signal per second of the run (n_up * sfreq / length) and amplitude = peak-to-peak of the band signal."""
    if len(band) != 2:
        raise ValueError(f"band must be (lo, hi), got {band!r}")
    n = _seconds_to_samples(sfreq, min_s=min_s, max_s=max_s, merge_s=merge_s)
    w = _windows2d(windows, "windows")
    _check_events_args(w.shape[1], max(n["min_s"], 1), n["max_s"], n["merge_s"], max_events)
    bd, env = band_envelope(w, band[0], band[1], sfreq, rms_s, trans_hz, ctx=ctx)
    ev = threshold_events(env, thr, aux=bd, min_len=max(n["min_s"], 1), max_len=n["max_s"], merge_gap=n["merge_s"], drop_edge=drop_edge,
                          max_events=max_events, ctx=ctx)
    t = event_table(ev, sfreq)
    t["freq_hz"] = t["n_up"].astype(np.float64) * float(sfreq) / np.maximum(t["length"], 1)
    t["amplitude"] = t["aux_max"].astype(np.float64) - t["aux_min"].astype(np.float64)
    return t


def detect_half_waves(windows, polarity=-1, sfreq=100.0, lowpass_hz=4.0, highpass_hz=None, min_s=0.3, max_s=1.0, min_amp=None, trans_hz=2.0,
                      max_events=64, ctx=None):
    """Half-waves of one polarity of the low-passed window (the building block of slow-wave detection): runs of polarity * filtered above 0
    with duration in [min_s, max_s].  The row mean is removed when there is no high-pass; the sign costs nothing, the taps are negated.
    `min_amp` gates the stored peak afterwards.  Returns `event_table` plus amplitude = the half-wave's peak magnitude and polarity."""
    if polarity not in (-1, 1):
        raise ValueError(f"polarity must be -1 or 1, got {polarity!r}")
    n = _seconds_to_samples(sfreq, min_s=min_s, max_s=max_s)
    w = _windows2d(windows, "windows")
    taps = fir_design(sfreq, highpass_hz, lowpass_hz, trans_hz) * float(polarity)
    _check_taps(taps, w.shape[1], "reflect")
    _check_events_args(w.shape[1], max(n["min_s"], 1), n["max_s"], 0, max_events)
    if min_amp is not None and not min_amp >= 0:
        raise ValueError(f"min_amp must be non-negative, got {min_amp}")
    ctx = ctx or default_context(0)
    x = w.to(torch.device("cuda", ctx.device), torch.float32)
    if highpass_hz is None:
        x = x - x.mean(1, keepdim=True)
    sig = fir_filter(x, taps, "reflect", ctx=ctx)
    ev = threshold_events(sig, 0.0, min_len=max(n["min_s"], 1), max_len=n["max_s"], merge_gap=0, drop_edge=False, max_events=max_events, ctx=ctx)
    t = event_table(ev, sfreq)
    t["amplitude"] = t["peak"].astype(np.float64)
    t["polarity"] = int(polarity)
    if min_amp is not None:
        keep = t["amplitude"] >= float(min_amp)
        t = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in t.items()}
    return t


def pair_half_waves(neg, pos):
    """Attach to each negative half-wave the positive one of the same window that starts where it ends (the negative-to-positive zero crossing);
    negative half-waves without one are left out.  Returns one row per pair: window, start, neg_length, pos_length, neg_peak, pos_peak,
    amplitude (peak to peak) and duration_s (both halves): the criteria of Massimini et al. 2004."""
    if neg["sfreq"] != pos["sfreq"] or neg["n_windows"] != pos["n_windows"]:
        raise ValueError("the two tables come from different sets")
    where = {(int(w), int(s)): i for i, (w, s) in enumerate(zip(pos["window"], pos["start"]))}
    pairs = [(i, where[(int(w), int(s + n))]) for i, (w, s, n) in enumerate(zip(neg["window"], neg["start"], neg["length"])) if (int(w), int(s + n)) in where]
    i = np.asarray([p[0] for p in pairs], np.int64); j = np.asarray([p[1] for p in pairs], np.int64)
    t = {"window": neg["window"][i], "start": neg["start"][i], "neg_length": neg["length"][i], "pos_length": pos["length"][j],
         "neg_peak": neg["peak"][i].astype(np.float64), "pos_peak": pos["peak"][j].astype(np.float64)}
    t["amplitude"] = t["neg_peak"] + t["pos_peak"]
    t["duration_s"] = (t["neg_length"] + t["pos_length"]).astype(np.float64) / neg["sfreq"]
    t["mid_s"] = (t["start"] + t["neg_length"]).astype(np.float64) / neg["sfreq"]
    t["sfreq"], t["n_windows"] = neg["sfreq"], neg["n_windows"]
    return t


def _feature_stats(v):
    v = np.asarray(v, np.float64)
    if v.size == 0:
        return {"n": 0, "mean": None, "sd": None, "q25": None, "median": None, "q75": None}
    q = np.quantile(v, [0.25, 0.5, 0.75])
    return {"n": int(v.size), "mean": float(v.mean()), "sd": float(v.std()), "q25": float(q[0]), "median": float(q[1]), "q75": float(q[2])}


def event_summary(table, n_windows, window_s, labels=None):
    """Density (events per minute of signal) and the mean, population sd and quartiles of duration_s, amplitude and freq_hz (those the table
    has) over the events of `table`.  With labels (n_windows,) the same per stage under "per_stage", keyed by the stage code."""
    n_windows = int(n_windows)
    if n_windows < 1 or not window_s > 0:
        raise ValueError(f"n_windows and window_s must be positive, got {n_windows} and {window_s}")
    win = np.asarray(table["window"], np.int64)
    if win.size and (win.min() < 0 or win.max() >= n_windows):
        raise ValueError(f"the table names window {int(win.max())}, n_windows is {n_windows}")

    def block(pick, nw):
        out = {"n_windows": int(nw), "n_events": int(pick.sum()), "density_per_min": float(pick.sum()) / (nw * float(window_s) / 60.0) if nw else None}
        for f in SUMMARY_FEATURES:
            if f in table:
                out[f] = _feature_stats(np.asarray(table[f])[pick])
        return out

    res = block(np.ones(win.size, bool), n_windows)
    if labels is not None:
        lab = np.asarray(labels).reshape(-1)
        if lab.size != n_windows:
            raise ValueError(f"{lab.size} labels for {n_windows} windows")
        res["per_stage"] = {str(int(c)): block(lab[win] == c, int(np.sum(lab == c))) for c in np.unique(lab)}
    return res


def ks_statistic(a, b):
    """Two-sample Kolmogorov-Smirnov statistic sup |F_a - F_b| from the sorted samples (float64)."""
    a, b = np.sort(np.asarray(a, np.float64)), np.sort(np.asarray(b, np.float64))
    z = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, z, side="right") / a.size - np.searchsorted(b, z, side="right") / b.size)))


def wasserstein_1d(a, b):
    """1-D Wasserstein-1 distance, the integral of |F_a - F_b| (float64)."""
    a, b = np.sort(np.asarray(a, np.float64)), np.sort(np.asarray(b, np.float64))
    z = np.sort(np.concatenate([a, b]))
    fa, fb = np.searchsorted(a, z[:-1], side="right") / a.size, np.searchsorted(b, z[:-1], side="right") / b.size
    return float(np.sum(np.abs(fa - fb) * np.diff(z)))


def compare_events(real, fake):
    """Per feature (duration_s, amplitude, freq_hz, where both tables have it): the two-sample KS statistic and the 1-D Wasserstein distance of
    the real against the synthetic events, with the sample sizes; None where a side has no events."""
    out = {}
    for f in SUMMARY_FEATURES:
        if f in real and f in fake:
            a, b = np.asarray(real[f], np.float64), np.asarray(fake[f], np.float64)
            ok = a.size > 0 and b.size > 0
            out[f] = {"n_real": int(a.size), "n_synthetic": int(b.size), "ks": ks_statistic(a, b) if ok else None,
                      "wasserstein": wasserstein_1d(a, b) if ok else None}
    return out


# ---------------------------------------------------------------------------------------------------- time-frequency
# How a window's (or a night's) spectrum moves in time, and whether spindles ride on the up-state of the slow oscillation, on two device
# primitives (csrc/tfr.hip): eegldm_stft_power, short-time multitaper power with optional band sums, and eegldm_pac_intervals, float64
# phase-amplitude sums over intervals.  As above: what is not a pass over the samples is float64 numpy in functions that take tables as
# input, and every refusal is a ValueError before the device is touched.
# THE DEFAULT BANDS, WINDOW LENGTHS AND THE SLOW-OSCILLATION BAND ARE THE LITERATURE'S; NOBODY HAS VALIDATED THEM ON THIS PROJECT'S
# 18-Hz-LOW-PASSED DATA, AND MATCHING STATISTICS ARE NOT EVIDENCE OF REALISM ON THEIR OWN.
STFT_NFFT = (64, 128, 256, 512, 1024, 2048, 4096)
STFT_MAX_TAPERS, STFT_MAX_BANDS = 8, 16
STFT_WINDOWS = ("dpss", "hann")
COURSE_FEATURES = ("mean", "cv", "lag1")


def stft_n_fft(n_win):
    """The smallest transform length eegldm_stft_power takes that holds a frame of n_win samples."""
    for n in STFT_NFFT:
        if n >= int(n_win) >= 1:
            return n
    raise ValueError(f"frames of 1..{STFT_NFFT[-1]} samples are taken, got {n_win}")


def stft_num_frames(length, n_win, hop, centre=True):
    """Frames of a row of `length` samples (eegldm_stft_num_frames: the rule lives in the library)."""
    f = int(lib.eegldm_stft_num_frames(int(length), int(n_win), int(hop), 1 if centre else 0))
    if f < 0:
        raise ValueError(f"need length >= 0, n_win >= 1 and hop >= 1, got {length}, {n_win}, {hop}")
    return f


def _bin_ranges(ranges, nbin, what):
    r = np.asarray(ranges, np.int64).reshape(-1, 2) if len(ranges) else np.zeros((0, 2), np.int64)
    if np.any(np.asarray(ranges, np.float64).reshape(-1, 2) != r):
        raise ValueError(f"{what}: bin ranges must be integers, got {ranges!r}")
    if np.any(r[:, 0] < 0) or np.any(r[:, 0] >= r[:, 1]) or np.any(r[:, 1] > nbin):
        raise ValueError(f"{what}: need 0 <= lo < hi <= {nbin}, got {r.tolist()}")
    return r


def stft_power(x, tapers, weights=None, n_fft=None, hop=None, centre=True, edge="reflect", detrend=True, scale=1.0, onesided=True, bins=None,
               bands=None, ctx=None):
    """Short-time multitaper power of every row (eegldm_stft_power; include/eegldm.h has the definition): P[b][f][k] = scale c_k sum_t
    weights[t]^2 |FFT_n_fft(tapers[t] (frame - mean))[k]|^2.  x (B, L) or (B, 1, L), any L; tapers (K, n_win) or (n_win,), K <= 8; n_fft
    defaults to the next listed size >= n_win, hop to n_win // 2.  bins = (k0, k1) picks the stored bins (None: all n_fft / 2 + 1; False: no
    spectrogram); bands = [(lo, hi), ...] are up to 16 bin ranges summed per frame (None: none).  Returns {"power": (B, F, k1 - k0) or None,
    "bands": (B, F, NB) or None, "n_frames": F}, fp32 tensors on the device."""
    x = _rows_any_length(x, "x")
    tp = np.asarray(tapers.detach().cpu().numpy() if torch.is_tensor(tapers) else tapers, np.float32)
    if tp.ndim == 1:
        tp = tp[None]
    if tp.ndim != 2 or not 1 <= tp.shape[0] <= STFT_MAX_TAPERS or tp.shape[1] < 1:
        raise ValueError(f"tapers (K, n_win) with K in 1..{STFT_MAX_TAPERS} expected, got shape {tp.shape}")
    if not np.all(np.isfinite(tp)):
        raise ValueError("non-finite tapers (as fp32)")
    k, n_win = int(tp.shape[0]), int(tp.shape[1])
    n_fft = stft_n_fft(n_win) if n_fft is None else n_fft
    if n_fft not in STFT_NFFT:
        raise ValueError(f"n_fft must be one of {STFT_NFFT}, got {n_fft!r}")
    if n_win > n_fft:
        raise ValueError(f"n_win {n_win} exceeds n_fft {n_fft}")
    hop = max(1, n_win // 2) if hop is None else hop
    if int(hop) != hop or hop < 1:
        raise ValueError(f"hop must be an integer >= 1, got {hop!r}")
    if edge not in FIR_EDGES:
        raise ValueError(f"edge must be one of {tuple(FIR_EDGES)}, got {edge!r}")
    w = np.ones(k) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    with np.errstate(over="ignore"):
        w2 = (w * w).astype(np.float32)
    if w.size != k or not np.all(np.isfinite(w2)):
        raise ValueError(f"{k} finite weights expected, got {w!r}")
    with np.errstate(over="ignore"):
        scale_ok = np.isfinite(np.float32(scale))
    if not scale_ok:
        raise ValueError(f"scale must be finite as fp32, got {scale!r}")
    nbin = n_fft // 2 + 1
    want_power = bins is not False
    k0, k1 = (0, nbin) if bins is None or bins is False else (int(v) for v in _bin_ranges([bins], nbin, "bins")[0])
    br = None if bands is None else _bin_ranges(list(bands), nbin, "bands")
    if br is not None and not 1 <= len(br) <= STFT_MAX_BANDS:
        raise ValueError(f"1..{STFT_MAX_BANDS} bands are taken, got {len(br)}")
    if not want_power and br is None:
        raise ValueError("nothing to compute: bins=False and bands=None")
    b, length = int(x.shape[0]), int(x.shape[1])
    if centre and edge == "reflect" and length >= 1 and n_win // 2 > length - 1:
        raise ValueError(f"reflect needs n_win // 2 <= L - 1, got n_win {n_win} for rows of {length} samples")
    f = stft_num_frames(length, n_win, int(hop), centre)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    power = torch.empty(b, f, k1 - k0, device=dev) if want_power else None
    bsum = torch.empty(b, f, len(br), device=dev) if br is not None else None
    if b and f:
        xd = _dev_rows(x, dev)
        td = torch.from_numpy(np.ascontiguousarray(tp)).to(dev)
        nb = 0 if br is None else len(br)
        bh = (C.c_int * max(2 * nb, 1))(*([int(v) for v in br.reshape(-1)] if nb else [0]))
        check(lib.eegldm_stft_power(ctx.h, ptr(xd), _ld(xd), b, length, ptr(td), (C.c_float * k)(*w2.tolist()), k, n_win, int(n_fft), int(hop),
                                    1 if centre else 0, FIR_EDGES[edge], 1 if detrend else 0, 1 if onesided else 0, float(scale), k0, k1,
                                    ptr(power), bh if nb else None, nb, ptr(bsum)))
    return {"power": power, "bands": bsum, "n_frames": f}


def spectrogram_tapers(n_win, window="dpss", half_nbw=2.0, n_tapers=None):
    """(tapers (K, n_win) float64 of unit energy, weights (K,) of ones): K = 2 half_nbw - 1 DPSS tapers from scipy (as `dpss_tapers` gets
    them), or the one periodic Hann window."""
    n_win = int(n_win)
    if n_win < 1:
        raise ValueError(f"n_win must be >= 1, got {n_win}")
    if window == "hann":
        if n_tapers not in (None, 1):
            raise ValueError("the Hann window is one taper")
        t = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_win) / n_win))[None] if n_win > 1 else np.ones((1, 1))
    elif window == "dpss":
        k = int(round(2.0 * float(half_nbw) - 1.0)) if n_tapers is None else n_tapers
        if int(k) != k or not 1 <= k <= STFT_MAX_TAPERS or not half_nbw > 0:
            raise ValueError(f"1..{STFT_MAX_TAPERS} tapers and half_nbw > 0 are needed, got n_tapers {k!r}, half_nbw {half_nbw!r}")
        if n_win < 2 * int(k):
            raise ValueError(f"{k} DPSS tapers need frames of at least {2 * int(k)} samples, got {n_win}")
        from scipy.signal.windows import dpss
        t = np.atleast_2d(dpss(n_win, float(half_nbw), int(k), sym=False, norm=2)).astype(np.float64)
    else:
        raise ValueError(f"window must be one of {STFT_WINDOWS}, got {window!r}")
    t = t / np.sqrt(np.sum(t * t, axis=1, keepdims=True))
    return t, np.ones(t.shape[0])


def band_bin_ranges(bands, sfreq, n_fft):
    """{name: (lo, hi) Hz} -> (names, [(k_lo, k_hi)]): the bins with lo <= k df < hi, df = sfreq / n_fft."""
    df = float(sfreq) / int(n_fft)
    freqs = np.arange(int(n_fft) // 2 + 1) * df
    names, ranges = [], []
    for name, (lo, hi) in bands.items():
        k_lo, k_hi = int(np.searchsorted(freqs, lo, side="left")), int(np.searchsorted(freqs, hi, side="left"))
        if not k_lo < k_hi:
            raise ValueError(f"band {name!r} = ({lo}, {hi}) Hz holds no bin at df = {df:g} Hz")
        names.append(name); ranges.append((k_lo, k_hi))
    return names, ranges


def spectrogram(x, sfreq=100.0, win_s=2.0, step_s=0.5, window="dpss", half_nbw=2.0, n_tapers=None, fmin=0.0, fmax=None, bands=None, keep_power=True,
                centre=True, edge="reflect", detrend=True, ctx=None):
    """Multitaper (or Hann) spectrogram of every row as a power density in V^2/Hz, with the time course of the power in each band.
    Frames of win_s seconds every step_s seconds; tapers of unit energy, unit weights, n_fft the next listed size >= the frame, scale = 1 /
    (sfreq sum w^2), one-sided.  bands {name: (lo, hi) Hz} (default: the module's BANDS) become bin ranges lo <= f < hi; band_power is their
    sum times df (V^2), float64 on the device.  keep_power=False never writes the spectrogram: a night's band courses cost F x NB floats.
    Returns {"power" (B, F, n_freqs) or None, "freqs", "times" (frame centres, s), "band_power" (B, F, NB), "band_names", "df", "n_fft",
    "n_frames"}.  The default bands and window lengths are the literature's; they have not been validated on this 18-Hz-low-passed data."""
    if not (sfreq > 0 and win_s > 0 and step_s > 0):
        raise ValueError(f"sfreq, win_s and step_s must be positive, got {sfreq}, {win_s}, {step_s}")
    n_win, hop = int(round(float(win_s) * float(sfreq))), int(round(float(step_s) * float(sfreq)))
    if n_win < 1 or hop < 1:
        raise ValueError(f"win_s = {win_s} s or step_s = {step_s} s is shorter than a sample at sfreq = {sfreq}")
    n_fft = stft_n_fft(n_win)
    tapers, w = spectrogram_tapers(n_win, window, half_nbw, n_tapers)
    df = float(sfreq) / n_fft
    freqs = np.arange(n_fft // 2 + 1) * df
    fmax = 0.5 * float(sfreq) if fmax is None else fmax
    k0, k1 = int(np.searchsorted(freqs, fmin, side="left")), int(np.searchsorted(freqs, fmax, side="right"))
    if not k0 < k1:
        raise ValueError(f"no bin in [{fmin}, {fmax}] Hz at df = {df:g} Hz")
    names, ranges = band_bin_ranges(BANDS if bands is None else bands, sfreq, n_fft)
    res = stft_power(x, tapers, w, n_fft=n_fft, hop=hop, centre=centre, edge=edge, detrend=detrend, scale=1.0 / (float(sfreq) * float(np.sum(w * w))),
                     onesided=True, bins=(k0, k1) if keep_power else False, bands=ranges, ctx=ctx)
    f = res["n_frames"]
    times = (np.arange(f) * hop + (0.0 if centre else 0.5 * n_win)) / float(sfreq)
    return {"power": res["power"], "freqs": freqs[k0:k1], "times": times, "band_power": res["bands"].double() * df, "band_names": names, "df": df,
            "n_fft": n_fft, "n_frames": f}


def band_course_stats(band_power):
    """What an average PSD cannot say about a band: per window and band, over the frames, the temporal mean, the coefficient of variation
    (population sd / mean) and the lag-1 autocorrelation of log power.  band_power (B, F, NB) -> {"mean", "cv", "lag1"}, (B, NB) float64;
    NaN where undefined (fewer than two frames, a zero mean, a non-positive power, no variance)."""
    p = band_power.detach().cpu().numpy() if torch.is_tensor(band_power) else band_power
    p = np.asarray(p, np.float64)
    if p.ndim != 3:
        raise ValueError(f"band_power (B, F, NB) expected, got shape {p.shape}")
    b, f, nb = p.shape
    nan = np.full((b, nb), np.nan)
    if f == 0:
        return {"mean": nan, "cv": nan.copy(), "lag1": nan.copy()}
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = p.mean(axis=1)
        cv = np.where(mean != 0, p.std(axis=1) / mean, np.nan)
        y = np.where(p > 0, np.log(np.where(p > 0, p, 1.0)), np.nan)
        d = y - y.mean(axis=1, keepdims=True)
        den = np.sum(d * d, axis=1)
        lag1 = np.where(den > 0, np.sum(d[:, :-1] * d[:, 1:], axis=1) / np.where(den > 0, den, 1.0), np.nan) if f >= 2 else nan.copy()
    return {"mean": mean, "cv": cv, "lag1": lag1}


def compare_band_courses(real, fake, names=None):
    """Per band and feature of `band_course_stats` (mean, cv, lag1): the KS statistic and the Wasserstein distance of the real against the
    synthetic windows (the finite values of each), with the sample sizes; None where a side has none."""
    nb = np.asarray(real["mean"]).shape[1]
    names = [str(i) for i in range(nb)] if names is None else list(names)
    out = {}
    for j, name in enumerate(names):
        out[name] = {}
        for feat in COURSE_FEATURES:
            a, c = np.asarray(real[feat], np.float64)[:, j], np.asarray(fake[feat], np.float64)[:, j]
            a, c = a[np.isfinite(a)], c[np.isfinite(c)]
            ok = a.size > 0 and c.size > 0
            out[name][feat] = {"n_real": int(a.size), "n_synthetic": int(c.size), "ks": ks_statistic(a, c) if ok else None,
                               "wasserstein": wasserstein_1d(a, c) if ok else None}
    return out


def fir_design_analytic(sfreq, lo, hi, trans_hz=2.0):
    """(re_taps, im_taps), float64: the low-pass prototype h = fir_design(sfreq, hi=(hi - lo) / 2, trans_hz) shifted to the band centre,
    re = 2 h cos(w0 m), im = -2 h sin(w0 m), m = n - (M - 1) / 2, w0 = 2 pi (lo + hi) / (2 sfreq).  Under `fir_filter`'s correlation form
    y[n] = sum_m g[m] x[n + m] the pair passes e^{+i w n} in the band and rejects its mirror: a real cos(w0 n) comes out as e^{i w0 n}."""
    if lo is None or hi is None or not 0.0 <= float(lo) < float(hi) < 0.5 * float(sfreq):
        raise ValueError(f"band ({lo}, {hi}) Hz: need 0 <= lo < hi < sfreq / 2 = {0.5 * float(sfreq)}")
    h = fir_design(sfreq, hi=0.5 * (float(hi) - float(lo)), trans_hz=trans_hz)
    m = np.arange(h.size, dtype=np.float64) - 0.5 * (h.size - 1)
    w0 = 2.0 * np.pi * (float(lo) + float(hi)) / (2.0 * float(sfreq))
    return 2.0 * h * np.cos(w0 * m), -2.0 * h * np.sin(w0 * m)


def analytic_band(windows, lo, hi, sfreq=100.0, trans_hz=2.0, edge="reflect", ctx=None):
    """(re, im): the analytic signal of the windows' (lo, hi) Hz band, two passes of `fir_filter` with the taps of `fir_design_analytic`;
    (N, L) fp32 on the device, L <= 4096.  The loader's 3072-sample windows lose their zero pads first."""
    w = _windows2d(windows, "windows")
    re_t, im_t = fir_design_analytic(sfreq, lo, hi, trans_hz)
    _check_taps(re_t, w.shape[1], edge)
    return fir_filter(w, re_t, edge, ctx=ctx), fir_filter(w, im_t, edge, ctx=ctx)


def pac_from_out(out):
    """eegldm_pac_intervals' table (NI, 4) = (n, sum a, c, s) -> {"n" int64, "sum_a", "mvl" = hypot(c, s) / sum a, "phase" = atan2(s, c)}, float64;
    mvl and phase are NaN where no sample took part (n <= 0; n = -1 marks an interval outside its row) or sum a is not positive."""
    o = np.asarray(out, np.float64).reshape(-1, 4)
    ok = (o[:, 0] > 0) & (o[:, 1] > 0)
    safe = np.where(ok, o[:, 1], 1.0)
    return {"n": o[:, 0].astype(np.int64), "sum_a": o[:, 1].copy(), "mvl": np.where(ok, np.hypot(o[:, 2], o[:, 3]) / safe, np.nan),
            "phase": np.where(ok, np.arctan2(o[:, 3], o[:, 2]), np.nan)}


def phase_amplitude_coupling(phase_re, phase_im, amp, intervals=None, ctx=None):
    """Amplitude-weighted mean vector of the phase signal (phase_re, phase_im) over intervals (eegldm_pac_intervals, float64 sums on the device):
    rows (B, L) fp32; intervals (NI, 3) int = (row, start, length), or None for one interval per row.  Returns `pac_from_out`'s dict."""
    pr, pi, am = (_rows_any_length(t, n) for t, n in ((phase_re, "phase_re"), (phase_im, "phase_im"), (amp, "amp")))
    if not tuple(pr.shape) == tuple(pi.shape) == tuple(am.shape):
        raise ValueError(f"shapes differ: {tuple(pr.shape)}, {tuple(pi.shape)}, {tuple(am.shape)}")
    b, length = int(pr.shape[0]), int(pr.shape[1])
    if length < 1:
        raise ValueError("rows of at least one sample are needed")
    iv = None
    if intervals is not None:
        iv = np.asarray(intervals)
        if iv.ndim != 2 or iv.shape[1] != 3 or not np.issubdtype(iv.dtype, np.integer) or (iv.size and np.abs(iv).max() > 0x7fffffff):
            raise ValueError(f"intervals (NI, 3) int32 = (row, start, length) expected, got shape {iv.shape} dtype {iv.dtype}")
        iv = np.ascontiguousarray(iv, np.int32)
    ni = b if iv is None else int(iv.shape[0])
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    out = torch.empty(ni, 4, dtype=torch.float64, device=dev)
    if ni:
        prd, pid, amd = _dev_rows(pr, dev), _dev_rows(pi, dev), _dev_rows(am, dev)
        ivd = None if iv is None else torch.from_numpy(iv).to(dev)
        check(lib.eegldm_pac_intervals(ctx.h, ptr(prd), _ld(prd), ptr(pid), _ld(pid), ptr(amd), _ld(amd), b, length, ptr(ivd), ni, ptr(out)))
    return pac_from_out(out.cpu().numpy())


def rayleigh_p(n, r):
    """p-value of the Rayleigh test of uniformity for n angles with resultant length r: z = n r^2, p = exp(-z) (1 + (2 z - z^2) / (4 n) -
    (24 z - 132 z^2 + 76 z^3 - 9 z^4) / (288 n^2)) (Zar, Biostatistical Analysis, eq. 27.4), clipped to [0, 1]."""
    z = n * r * r
    p = np.exp(-z) * (1.0 + (2.0 * z - z * z) / (4.0 * n) - (24.0 * z - 132.0 * z ** 2 + 76.0 * z ** 3 - 9.0 * z ** 4) / (288.0 * n * n))
    return float(min(max(p, 0.0), 1.0))


def circular_summary(phases):
    """{"n", "mean" (rad, in (-pi, pi]), "R" (resultant length), "z" = n R^2, "p" (Rayleigh)} of the finite angles; None fields when there are none."""
    a = np.asarray(phases, np.float64).reshape(-1)
    a = a[np.isfinite(a)]
    if a.size == 0:
        return {"n": 0, "mean": None, "R": None, "z": None, "p": None}
    c, s = np.mean(np.cos(a)), np.mean(np.sin(a))
    r = float(np.hypot(c, s))
    return {"n": int(a.size), "mean": float(np.arctan2(s, c)), "R": r, "z": float(a.size * r * r), "p": rayleigh_p(a.size, r)}


def circular_distance(a, b):
    """|a - b| on the circle, in [0, pi]; None when either is None."""
    if a is None or b is None:
        return None
    return float(abs(np.angle(np.exp(1j * (float(a) - float(b))))))


def spindle_so_coupling(windows, spindles, sfreq=100.0, so_band=(0.5, 1.25), so_trans_hz=0.5, sigma_band=(11.0, 16.0), half_s=0.5, sigma_trans_hz=2.0,
                        ctx=None):
    """Do the spindles of `spindles` (a `detect_spindles` table of these windows) ride on a preferred phase of the slow oscillation?  The SO
    phase is the analytic so_band signal, the spindle amplitude the modulus of the analytic sigma_band signal.  Per event: the SO phase at the
    envelope peak (`argmax`), and the mean vector length and preferred phase of the amplitude-weighted SO phase over peak +- half_s; events
    whose interval leaves the window are dropped and counted.  Per set: `circular_summary` of the peak phases and of the preferred phases.
    Phase 0 is the SO's positive peak.  The SO band is the literature's; it has not been validated on this 18-Hz-low-passed data."""
    if len(so_band) != 2 or len(sigma_band) != 2:
        raise ValueError(f"bands must be (lo, hi), got {so_band!r} and {sigma_band!r}")
    half = _seconds_to_samples(sfreq, half_s=half_s)["half_s"]
    w = _windows2d(windows, "windows")
    n_win, length = int(w.shape[0]), int(w.shape[1])
    win, peak = np.asarray(spindles["window"], np.int64), np.asarray(spindles["argmax"], np.int64)
    if win.shape != peak.shape or (win.size and (win.min() < 0 or win.max() >= n_win or peak.min() < 0 or peak.max() >= length)):
        raise ValueError("the spindle table does not belong to these windows")
    for band, trans in ((so_band, so_trans_hz), (sigma_band, sigma_trans_hz)):
        _check_taps(fir_design_analytic(sfreq, band[0], band[1], trans)[0], length, "reflect")
    keep = (peak - half >= 0) & (peak + half + 1 <= length)
    win, peak = win[keep], peak[keep]
    res = {"n_events": int(win.size), "n_dropped": int(np.sum(~keep)), "window": win, "peak": peak}
    if win.size == 0:
        res.update(peak_phase=np.zeros(0), mvl=np.zeros(0), phase=np.zeros(0))
    else:
        so_r, so_i = analytic_band(w, so_band[0], so_band[1], sfreq, so_trans_hz, ctx=ctx)
        sg_r, sg_i = analytic_band(w, sigma_band[0], sigma_band[1], sfreq, sigma_trans_hz, ctx=ctx)
        amp = torch.hypot(sg_r, sg_i)
        wi, pk = torch.from_numpy(win).to(so_r.device), torch.from_numpy(peak).to(so_r.device)
        res["peak_phase"] = np.arctan2(so_i[wi, pk].double().cpu().numpy(), so_r[wi, pk].double().cpu().numpy())
        pac = phase_amplitude_coupling(so_r, so_i, amp, np.stack([win, peak - half, np.full_like(win, 2 * half + 1)], axis=1), ctx=ctx)
        res["mvl"], res["phase"] = pac["mvl"], pac["phase"]
    res["peak_phase_stats"] = circular_summary(res["peak_phase"])
    res["preferred_phase_stats"] = circular_summary(res["phase"])
    return res


def compare_coupling(real, fake):
    """Two `spindle_so_coupling` results side by side: both sets' circular summaries, the circular distance of their mean phases (peak and
    preferred), and the KS statistic and Wasserstein distance of the per-event mean vector lengths (None where a side has no events)."""
    out = {}
    for side, r in (("real", real), ("synthetic", fake)):
        out[side] = {"n_events": int(r["n_events"]), "n_dropped": int(r["n_dropped"]), "peak_phase": r["peak_phase_stats"],
                     "preferred_phase": r["preferred_phase_stats"]}
    out["peak_phase_distance"] = circular_distance(real["peak_phase_stats"]["mean"], fake["peak_phase_stats"]["mean"])
    out["preferred_phase_distance"] = circular_distance(real["preferred_phase_stats"]["mean"], fake["preferred_phase_stats"]["mean"])
    a, b = (np.asarray(r["mvl"], np.float64)[np.isfinite(np.asarray(r["mvl"], np.float64))] for r in (real, fake))
    ok = a.size > 0 and b.size > 0
    out["mvl"] = {"n_real": int(a.size), "n_synthetic": int(b.size), "ks": ks_statistic(a, b) if ok else None,
                  "wasserstein": wasserstein_1d(a, b) if ok else None}
    return out


# ---------------------------------------------------------------------------------------------------- signal complexity
# How REGULAR a window is: Hjorth parameters, permutation entropy and (multiscale) sample entropy, on three device primitives
# (csrc/complexity.hip): eegldm_row_moments, float64 two-pass moments of a row and of its first and second differences;
# eegldm_ordinal_counts, the histogram of ordinal patterns; eegldm_template_matches, the O(L^2) pair counts of sample entropy with the
# coarse-graining of the multiscale variant fused in.  As above: what is not a pass over the samples is float64 numpy in functions that take
# tables as input, and every refusal is a ValueError before the device is touched.  The loader's 3072-sample windows lose their zero pads first.
# NOBODY HAS MEASURED WHAT THESE FEATURES SHOW ON THIS PROJECT'S 18-Hz-LOW-PASSED DATA: they are offered as distributions to compare, not as
# detectors of stages or of bad samples.
CX_MAX_LEN, CX_MIN_ORDER, CX_MAX_ORDER, CX_MAX_M, CX_MAX_SCALE = 4096, 2, 6, 4, 64
MOMENT_FIELDS = ("mean", "m2_x", "m2_d1", "m2_d2", "line_length", "sign_changes", "min", "max")
R_MODES = ("sd", "abs")


def _as_int(v, name):
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def _cx_rows(windows, name="windows", min_len=1):
    w = _windows2d(windows, name)
    if not min_len <= int(w.shape[1]) <= CX_MAX_LEN:
        raise ValueError(f"{name}: rows of {min_len}..{CX_MAX_LEN} samples are taken, got {int(w.shape[1])}")
    return w


def _check_ordinal_args(length, order, delay):
    order, delay = _as_int(order, "order"), _as_int(delay, "delay")
    if not CX_MIN_ORDER <= order <= CX_MAX_ORDER:
        raise ValueError(f"order must lie in {CX_MIN_ORDER}..{CX_MAX_ORDER}, got {order}")
    if delay < 1:
        raise ValueError(f"delay must be >= 1, got {delay}")
    if (order - 1) * delay >= int(length):
        raise ValueError(f"(order - 1) * delay = {(order - 1) * delay} leaves no position in a row of {length} samples")
    return order, delay


def _check_template_args(length, m, scale):
    m, scale = _as_int(m, "m"), _as_int(scale, "scale")
    if not 1 <= m <= CX_MAX_M:
        raise ValueError(f"m must lie in 1..{CX_MAX_M}, got {m}")
    if not 1 <= scale <= CX_MAX_SCALE:
        raise ValueError(f"scale must lie in 1..{CX_MAX_SCALE}, got {scale}")
    if int(length) // scale - m < 2:
        raise ValueError(f"a row of {length} samples at scale {scale} has {int(length) // scale} points: m = {m} needs at least {m + 2}")
    return m, scale


def _check_r(r, n=None):
    """A positive finite tolerance, or one per row: (n,) float32."""
    a = np.asarray(r.detach().cpu().numpy() if torch.is_tensor(r) else r, np.float64)
    if a.ndim > 1 or (a.ndim == 1 and n is not None and a.shape != (n,)) or (a.ndim == 1 and n is None):
        raise ValueError(f"r must be a float{'' if n is None else f' or ({n},)'}, got shape {a.shape}")
    with np.errstate(over="ignore"):
        a32 = a.astype(np.float32)                              # as uploaded
    if not (np.all(np.isfinite(a32)) and np.all(a32 > 0)):
        raise ValueError("r must be positive and finite (as fp32)")
    return a32


def _moments_dev(x, ctx):
    out = torch.empty(x.shape[0], 8, dtype=torch.float64, device=x.device)
    if x.shape[0]:
        check(lib.eegldm_row_moments(ctx.h, ptr(x), _ld(x), int(x.shape[0]), int(x.shape[1]), ptr(out)))
    return out


def row_moments(windows, ctx=None):
    """(N, 8) float64 numpy, columns MOMENT_FIELDS: mean, the central sums of squares of the row, of its first and of its second differences
    (two passes, float64), line length sum |d1|, sign changes of x - mean, min, max (eegldm_row_moments; include/eegldm.h has the definition)."""
    w = _cx_rows(windows)
    ctx = ctx or default_context(0)
    return _moments_dev(_dev_rows(w, torch.device("cuda", ctx.device)), ctx).cpu().numpy()


def hjorth_from_moments(table, length):
    """(N, 3) float64 = (activity, mobility, complexity) from `row_moments`' table of rows of `length` >= 3 samples: activity = var x, mobility =
    sqrt(var d1 / var x), complexity = sqrt(var d2 / var d1) / mobility, population variances m2 / count.  A constant row gives NaN (0 / 0)."""
    t = np.asarray(table, np.float64).reshape(-1, 8)
    n = _as_int(length, "length")
    if n < 3:
        raise ValueError(f"Hjorth parameters need rows of at least 3 samples, got {n}")
    with np.errstate(divide="ignore", invalid="ignore"):
        v0, v1, v2 = t[:, 1] / n, t[:, 2] / (n - 1), t[:, 3] / (n - 2)
        mob = np.sqrt(v1 / v0)
        return np.stack([v0, mob, np.sqrt(v2 / v1) / mob], 1)


def hjorth(windows, ctx=None):
    """Hjorth activity, mobility and complexity of every window: (N, 3) float64 numpy (`row_moments` + `hjorth_from_moments`)."""
    w = _cx_rows(windows, min_len=3)
    return hjorth_from_moments(row_moments(w, ctx=ctx), int(w.shape[1]))


def ordinal_counts(windows, order=3, delay=1, ctx=None):
    """(counts (N, order!) int32, skipped (N,) int32) numpy: how often each ordinal pattern of `order` samples `delay` apart occurs in a window
    (index = Lehmer code, ties rank by position), and the positions left out because they hold a NaN or an infinity (eegldm_ordinal_counts)."""
    w = _cx_rows(windows)
    order, delay = _check_ordinal_args(w.shape[1], order, delay)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    x = _dev_rows(w, dev)
    nb = int(np.prod(np.arange(1, order + 1)))
    counts = torch.empty(x.shape[0], nb, dtype=torch.int32, device=dev)
    skipped = torch.empty(x.shape[0], dtype=torch.int32, device=dev)
    if x.shape[0]:
        check(lib.eegldm_ordinal_counts(ctx.h, ptr(x), _ld(x), int(x.shape[0]), int(x.shape[1]), order, delay, ptr(counts), ptr(skipped)))
    return counts.cpu().numpy(), skipped.cpu().numpy()


def permutation_entropy_from_counts(counts, normalize=True):
    """-sum p ln p of every row of a pattern histogram (N, order!), p = counts / their sum, 0 ln 0 = 0; divided by ln(order!) when normalize.
    A row without a counted position gives NaN."""
    c = np.asarray(counts, np.float64)
    if c.ndim != 2 or c.shape[1] < 2:
        raise ValueError(f"counts (N, order!) expected, got shape {c.shape}")
    tot = c.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = c / tot
        h = -np.sum(np.where(c > 0, p * np.log(np.where(c > 0, p, 1.0)), 0.0), 1)
    h = np.where(tot[:, 0] > 0, h, np.nan)
    return h / np.log(c.shape[1]) if normalize else h


def permutation_entropy(windows, order=3, delay=1, normalize=True, ctx=None):
    """Permutation entropy (Bandt and Pompe 2002) of every window: (N,) float64, in [0, 1] when normalize."""
    return permutation_entropy_from_counts(ordinal_counts(windows, order, delay, ctx=ctx)[0], normalize)


def _template_counts_dev(x, r_dev, m, scale, ctx):
    counts = torch.empty(x.shape[0], 2, dtype=torch.int64, device=x.device)
    if x.shape[0]:
        check(lib.eegldm_template_matches(ctx.h, ptr(x), _ld(x), int(x.shape[0]), int(x.shape[1]), m, scale, ptr(r_dev), ptr(counts)))
    return counts


def template_match_counts(windows, m=2, r=None, scale=1, ctx=None):
    """(N, 2) int64 numpy = (B, A): the pairs of templates i < j of the window coarse-grained by `scale` that match within the absolute
    tolerance r (a float or (N,)) at length m and at length m + 1, over the same N / scale - m templates (eegldm_template_matches)."""
    w = _cx_rows(windows)
    m, scale = _check_template_args(w.shape[1], m, scale)
    if r is None:
        raise ValueError("r, the absolute tolerance (a float or one per window), is needed")
    r32 = _check_r(r, int(w.shape[0]))
    if r32.ndim == 0:
        r32 = np.full(int(w.shape[0]), r32, np.float32)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    return _template_counts_dev(_dev_rows(w, dev), torch.from_numpy(r32).to(dev), m, scale, ctx).cpu().numpy()


def sample_entropy_from_counts(counts):
    """SampEn = -ln(A / B) of (..., 2) = (B, A) pair counts, float64: NaN where B == 0 (nothing to condition on), +inf where A == 0 < B."""
    c = np.asarray(counts, np.float64)
    if c.shape[-1] != 2:
        raise ValueError(f"counts (..., 2) expected, got shape {c.shape}")
    b, a = c[..., 0], c[..., 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b > 0, -np.log(np.where(b > 0, a / np.where(b > 0, b, 1.0), 1.0)), np.nan)


def _check_scales(length, m, scales):
    s = tuple(scales) if np.ndim(scales) else (scales,)
    if not s:
        raise ValueError("at least one scale is needed")
    return tuple(_check_template_args(length, m, v)[1] for v in s)


def sample_entropy(windows, m=2, r=0.2, r_mode="sd", scales=(1,), ctx=None):
    """(Multiscale) sample entropy (Richman and Moorman 2000; Costa et al. 2002) of every window: (N, len(scales)) float64 numpy.  r_mode "sd":
    the tolerance is r times the population standard deviation of the RAW window at every scale (Costa's convention), taken on the device from
    the moments table; "abs": r is the tolerance itself."""
    w = _cx_rows(windows)
    if r_mode not in R_MODES:
        raise ValueError(f"r_mode must be one of {R_MODES}, got {r_mode!r}")
    m = _check_template_args(w.shape[1], m, 1)[0]
    scales = _check_scales(w.shape[1], m, scales)
    _check_r(r)
    ctx = ctx or default_context(0)
    dev = torch.device("cuda", ctx.device)
    x = _dev_rows(w, dev)
    if r_mode == "sd":                                          # float64 on the device, one rounding to the fp32 the kernel compares with
        r_dev = (float(r) * torch.sqrt(_moments_dev(x, ctx)[:, 1] / float(x.shape[1]))).float()
    else:
        r_dev = torch.full((x.shape[0],), float(r), dtype=torch.float32, device=dev)
    counts = torch.stack([_template_counts_dev(x, r_dev, m, s, ctx) for s in scales], 1)
    return sample_entropy_from_counts(counts.cpu().numpy())


def complexity_feature_names(orders=(3, 4, 5), scales=(1, 2, 5, 10, 20)):
    return (["activity", "mobility", "complexity", "sign_change_rate", "line_length_per_sample"] + [f"perm_entropy_o{int(o)}" for o in orders]
            + [f"sample_entropy_s{int(s)}" for s in scales])


def complexity_features(windows, orders=(3, 4, 5), delay=1, m=2, r=0.2, r_mode="sd", scales=(1, 2, 5, 10, 20), ctx=None):
    """(features (N, F) float64 numpy, names): Hjorth activity, mobility and complexity, sign changes of x - mean and line length per
    difference (both / (L - 1)), normalised permutation entropy at `orders`, sample entropy at `scales`.  Rows are windows: the matrix goes
    into `mmd2`, `kid`, `knn` and `precision_recall_coverage` as it is (drop non-finite rows first), a column into `compare_features`."""
    w = _cx_rows(windows, min_len=3)
    length = int(w.shape[1])
    orders = tuple(orders) if np.ndim(orders) else (orders,)
    orders = tuple(_check_ordinal_args(length, o, delay)[0] for o in orders)
    delay = _as_int(delay, "delay")
    if r_mode not in R_MODES:
        raise ValueError(f"r_mode must be one of {R_MODES}, got {r_mode!r}")
    m = _check_template_args(length, m, 1)[0]
    scales = _check_scales(length, m, scales)
    _check_r(r)
    ctx = ctx or default_context(0)
    w = _dev_rows(w, torch.device("cuda", ctx.device))
    mom = row_moments(w, ctx=ctx)
    cols = [hjorth_from_moments(mom, length), mom[:, 5:6] / (length - 1), mom[:, 4:5] / (length - 1)]
    cols += [permutation_entropy(w, o, delay, True, ctx=ctx)[:, None] for o in orders]
    if scales:
        cols.append(sample_entropy(w, m, r, r_mode, scales, ctx=ctx))
    return np.concatenate(cols, 1), complexity_feature_names(orders, scales)


def compare_features(real, fake, names):
    """Per column of two feature matrices (N_real, F) and (N_fake, F): the two-sample KS statistic and the 1-D Wasserstein distance over the
    FINITE values of each side (None where a side has none), with the counts of finite and of non-finite values beside them."""
    a, b = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    names = list(names)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != len(names) or b.shape[1] != len(names):
        raise ValueError(f"feature matrices (N, {len(names)}) expected, got {a.shape} and {b.shape}")
    out = {}
    for k, name in enumerate(names):
        u, v = a[:, k][np.isfinite(a[:, k])], b[:, k][np.isfinite(b[:, k])]
        ok = u.size > 0 and v.size > 0
        out[name] = {"n_real": int(u.size), "n_synthetic": int(v.size), "n_real_nonfinite": int(a.shape[0] - u.size),
                     "n_synthetic_nonfinite": int(b.shape[0] - v.size), "ks": ks_statistic(u, v) if ok else None,
                     "wasserstein": wasserstein_1d(u, v) if ok else None}
    return out
