"""Device-resident window bank: the recordings of a loader in ONE flat fp32 device buffer, normalised there (eegldm_bank_normalise), and
training batches cropped, padded and labelled by one launch each (eegldm_window_batch) -- no per-item Python, no upload per batch.

The sampling policy lives in the SEGMENT TABLES built here once per bank in plain int64 numpy (`segment_tables`); the kernel knows nothing of
epochs or stages.  A segment is a run of consecutive valid crop starts of one recording that share a label; a uniform draw over a table is
one uniform draw over every valid start it lists, which is the distribution the host loader's rejection loop (entry/common.py:
WindowLoader._item) produces -- in one draw, with no retry limit.  Only the DISTRIBUTION is the host loader's: crops come from the device
Philox stream, not from the loader's numpy Generator, so the two loaders do not draw the same windows from the same seed."""
import numpy as np
import torch

from ._lib import check, default_context, lib, ptr
from .entry.common import BORDER, EPOCH, WINDOW

BANK_CHUNK = 16384                       # EEGLDM_BANK_CHUNK of include/eegldm.h
CLASS_KEY = 0x9E3779B97F4A7C15           # xor-ed into the seed for the class draw of "balanced": a Philox key of its own, same counters
SAMPLINGS = ("recording", "uniform", "balanced")


class SegmentTable:
    """seg_first / seg_cum / seg_label / group_bounds as include/eegldm.h describes them (host int64 / int32 arrays), plus what only the
    host needs: seg_rec (the recording of every segment) and group_keys (the recording index or the label each group stands for)."""

    def __init__(self, seg_first, seg_count, seg_label, seg_rec, group_bounds, group_keys):
        self.seg_first = np.ascontiguousarray(seg_first, np.int64)
        self.seg_cum = np.concatenate([[0], np.cumsum(np.asarray(seg_count, np.int64))]).astype(np.int64)
        self.seg_label = np.ascontiguousarray(seg_label, np.int32)
        self.seg_rec = np.ascontiguousarray(seg_rec, np.int64)
        self.group_bounds = np.ascontiguousarray(group_bounds, np.int64)
        self.group_keys = np.ascontiguousarray(group_keys, np.int64)

    n_seg = property(lambda self: len(self.seg_first))
    n_group = property(lambda self: len(self.group_bounds) - 1)
    total = property(lambda self: int(self.seg_cum[-1]))

    def group_range(self, g):
        """[lo, hi): the table indices of group g."""
        return int(self.seg_cum[self.group_bounds[g]]), int(self.seg_cum[self.group_bounds[g + 1]])

    def lookup(self, idx):
        """Table indices -> (src, label, recording): the host restatement of steps 4 and 5 of eegldm_window_batch."""
        idx = np.asarray(idx, np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= self.total):
            raise IndexError(f"table index outside [0, {self.total})")
        j = np.searchsorted(self.seg_cum, idx, side="right") - 1
        return self.seg_first[j] + idx - self.seg_cum[j], self.seg_label[j].astype(np.int64), self.seg_rec[j]


def _check_stages(st, name):
    st = np.asarray(st)
    if st.ndim != 1 or not np.issubdtype(st.dtype, np.integer):
        raise ValueError(f"{name}: stage codes must be a 1-D integer array, got {st.dtype} {st.shape}")
    return st.astype(np.int64)


def segment_tables(lengths, stages=None, window=WINDOW, names=None):
    """lengths: samples per recording; stages: None or one 1-D integer array per recording (one code per EPOCH samples from sample 0,
    negative = unscored) -> (table_a, table_b, row_off).

    Without stages a recording is one segment, starts 0 .. L - window, label -1.  With stages, epoch e with code c >= 0 gives the starts
    whose window centre s + window // 2 lies in it, clipped to the valid starts: max(0, EPOCH e - window // 2) .. min(L - window,
    EPOCH e + EPOCH - 1 - window // 2) -- exactly the starts for which centre_label returns c; empty runs are dropped.
    table_a is ordered by (recording, epoch) and grouped by recording (every recording has a group, possibly empty); table_b holds the
    same segments ordered by (label, recording, epoch) and grouped by label (the labels present, ascending)."""
    lengths = np.asarray(lengths, np.int64)
    n_rec = len(lengths)
    names = names or [f"recording {r}" for r in range(n_rec)]
    if n_rec < 1:
        raise ValueError("a bank needs at least one recording")
    if window < 1:
        raise ValueError(f"window {window} must be >= 1")
    for r in range(n_rec):
        if lengths[r] < window:
            raise ValueError(f"{names[r]}: {int(lengths[r])} samples, need at least {window}")
    if stages is not None and len(stages) != n_rec:
        raise ValueError(f"{len(stages)} stage arrays for {n_rec} recordings")
    row_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    half = window // 2
    first, count, label, rec, bounds = [], [], [], [], [0]
    for r in range(n_rec):
        last = int(lengths[r]) - window                  # the last valid start
        if stages is None:
            s0, s1, lab = np.zeros(1, np.int64), np.full(1, last, np.int64), np.full(1, -1, np.int64)
        else:
            st = _check_stages(stages[r], names[r])
            e = np.arange(min(len(st), (last + half) // EPOCH + 1), dtype=np.int64)
            s0 = np.maximum(0, EPOCH * e - half); s1 = np.minimum(last, EPOCH * e + (EPOCH - 1 - half)); lab = st[:len(e)]
            keep = (lab >= 0) & (s1 >= s0)
            s0, s1, lab = s0[keep], s1[keep], lab[keep]
        first.append(row_off[r] + s0); count.append(s1 - s0 + 1); label.append(lab); rec.append(np.full(len(s0), r, np.int64))
        bounds.append(bounds[-1] + len(s0))
    first, count, label, rec = (np.concatenate(v).astype(np.int64) for v in (first, count, label, rec))
    a = SegmentTable(first, count, label, rec, bounds, np.arange(n_rec))
    order = np.argsort(label, kind="stable")             # (label, recording, epoch): a stable sort of the (recording, epoch) order
    keys, starts = np.unique(label[order], return_index=True)
    b = SegmentTable(first[order], count[order], label[order], rec[order], np.concatenate([starts, [len(order)]]), keys)
    b.order = order                                       # b's segment j is a's segment order[j]
    return a, b, row_off


def draw_indices(table, words, group=None):
    """The draw rule of eegldm_window_batch on the host: words = the uint64 values (r0 << 32) | r1 of Philox(seed, offset + b), group =
    None (the whole table) or one group per window -> table indices lo + v % (hi - lo)."""
    words = np.asarray(words, np.uint64)
    if group is None:
        lo, hi = np.zeros(len(words), np.int64), np.full(len(words), table.total, np.int64)
    else:
        group = np.asarray(group, np.int64)
        lo, hi = table.seg_cum[table.group_bounds[group]], table.seg_cum[table.group_bounds[group + 1]]
    if np.any(hi <= lo):
        raise ValueError("draw from an empty range")
    return lo + (words % (hi - lo).astype(np.uint64)).astype(np.int64)


class WindowBank:
    """Reads `files` (.npy recordings, flattened to one channel as normalise_recording flattens them), uploads them into one device buffer,
    normalises it there and builds both segment tables.  `stage_files`: one hypnogram per recording (WindowLoader's rules: 1-D integer
    array, one code per 30-s epoch, negative = unscored).  upload=False builds the host side only (lengths, tables): planning and tests.

    Raises ValueError naming the file for a recording shorter than `window`, a bad stage array, and a recording whose scaled minimum or
    maximum is not finite (a NaN or an infinity in the data, or an overflow of x * (1 + 1e6)); MemoryError, before anything is allocated,
    when the bank does not fit the free device memory."""

    def __init__(self, files, stage_files=None, window=WINDOW, border=BORDER, device=None, upload=True, ctx=None):
        self.files = list(files)
        self.stage_files = list(stage_files) if stage_files is not None else None
        self.window, self.border = int(window), int(border)
        if self.border < 0:
            raise ValueError(f"border {border} must be >= 0")
        if not self.files:
            raise ValueError("a bank needs at least one recording")
        if self.stage_files is not None and len(self.stage_files) != len(self.files):
            raise ValueError(f"{len(self.stage_files)} stage files for {len(self.files)} recordings")
        arrays = [np.load(f, mmap_mode="r") for f in self.files]
        lengths = [int(np.prod(a.shape)) for a in arrays]
        stages = None
        if self.stage_files is not None:
            stages = [_check_stages(np.load(f), f) for f in self.stage_files]
        self.table_a, self.table_b, self.row_off = segment_tables(lengths, stages, self.window, names=self.files)
        self.lengths = np.asarray(lengths, np.int64)
        self.has_stages = stages is not None
        self.classes = [int(k) for k in self.table_b.group_keys] if self.has_stages else []      # the labels present, ascending
        self.n_rec, self.total = len(self.files), int(self.row_off[-1])
        self.uploaded = False
        if upload:
            self._upload(arrays, device, ctx)

    # ---- device side
    def _upload(self, arrays, device, ctx):
        if not torch.cuda.is_available():
            raise RuntimeError("WindowBank needs an MI355X (gfx950) GPU: no HIP device is visible; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"device {device!r}: the bank lives in device memory")
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.device, self.ctx = torch.device("cuda", index), ctx or default_context(index)
        ws_floats = 2 * (self.total // BANK_CHUNK + self.n_rec + 1)
        tables = sum(t.n_seg * 20 + 8 * (t.n_group + 2) for t in (self.table_a, self.table_b))
        need = 4 * self.total + 4 * ws_floats + 16 * self.n_rec + tables + 8 * self.n_rec
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free:
            raise MemoryError(f"the bank needs {need / 2**30:.2f} GiB of device memory ({self.n_rec} recordings, {self.total} samples) and "
                              f"{free / 2**30:.2f} GiB are free: shard the file list or bank fewer recordings")
        self.bank = torch.empty(self.total, dtype=torch.float32, device=self.device)
        for r, a in enumerate(arrays):
            row = np.array(a, dtype=np.float32).reshape(-1)      # (a copy: the memory map is read-only)
            self.bank[int(self.row_off[r]):int(self.row_off[r + 1])].copy_(torch.from_numpy(row))
        self.row_off_dev = torch.from_numpy(self.row_off).to(self.device)
        self.lohi_dev = torch.empty(self.n_rec, 2, dtype=torch.float32, device=self.device)
        ws = torch.empty(ws_floats, dtype=torch.float32, device=self.device)
        check(lib.eegldm_bank_normalise(self.ctx.h, ptr(self.bank), ptr(self.row_off_dev), self.row_off.ctypes.data, self.n_rec,
                                        ptr(self.lohi_dev), ptr(ws), ws_floats))
        self.lohi = self.lohi_dev.cpu().numpy()
        bad = np.flatnonzero(~np.isfinite(self.lohi).all(axis=1))
        if len(bad):
            r = int(bad[0])
            raise ValueError(f"{self.files[r]}: scaled minimum {self.lohi[r, 0]} / maximum {self.lohi[r, 1]} is not finite "
                             "(a NaN or an infinity in the recording, or x * (1 + 1e6) overflows float32)")
        self._dev = {name: self._table_to_device(t) for name, t in (("a", self.table_a), ("b", self.table_b))}
        self.uploaded = True

    def _table_to_device(self, t):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        return {"seg_first": up(t.seg_first), "seg_cum": up(t.seg_cum), "seg_label": up(t.seg_label), "group_bounds": up(t.group_bounds)}

    def table(self, which):
        return {"recording": self.table_a, "a": self.table_a, "label": self.table_b, "b": self.table_b}[which]

    # ---- host translations
    def locate(self, src):
        """Bank index -> (recording, start)."""
        src = int(src)
        if not 0 <= src < self.total:
            raise IndexError(f"bank index {src} outside [0, {self.total})")
        r = int(np.searchsorted(self.row_off, src, side="right") - 1)
        return r, src - int(self.row_off[r])

    def index_of(self, rec, start, table="recording"):
        """(recording, start) -> the index of that crop in the table ordered by "recording" (table A) or by "label" (table B); ValueError
        when `start` is no valid start of the recording or its window's centre is unscored."""
        rec, start = int(rec), int(start)
        if not 0 <= rec < self.n_rec or not 0 <= start <= int(self.lengths[rec]) - self.window:
            raise ValueError(f"({rec}, {start}) is not a valid crop start")
        a, src = self.table_a, int(self.row_off[rec]) + start
        j = int(np.searchsorted(a.seg_first, src, side="right") - 1)      # table A's seg_first ascends
        if j < 0 or a.seg_rec[j] != rec or src >= a.seg_first[j] + (a.seg_cum[j + 1] - a.seg_cum[j]):
            raise ValueError(f"the window at ({rec}, {start}) has an unscored centre: it is in no segment")
        if self.table(table) is a:
            return int(a.seg_cum[j]) + src - int(a.seg_first[j])
        b = self.table_b
        jb = int(np.flatnonzero(b.order == j)[0])
        return int(b.seg_cum[jb]) + src - int(b.seg_first[jb])

    # ---- one batch
    def batch(self, B, table="recording", group=None, idx=None, seed=0, offset=0, out=None, want_src=False):
        """One eegldm_window_batch launch -> (eeg (B, 1, window + 2 border) fp32, labels (B,) int64, src (B,) int64 or None).  group / idx:
        device int64 tensors of length B, or None."""
        if not self.uploaded:
            raise RuntimeError("this bank was built with upload=False: it has no device side")
        t, d = self.table(table), self._dev["a" if self.table(table) is self.table_a else "b"]
        W = self.window + 2 * self.border
        if out is None:
            out = torch.empty(B, 1, W, dtype=torch.float32, device=self.device)
        labels = torch.empty(B, dtype=torch.int64, device=self.device)
        src = torch.empty(B, dtype=torch.int64, device=self.device) if want_src else None
        for name, v in (("group", group), ("idx", idx)):
            if v is not None and (v.dtype != torch.int64 or v.numel() != B or not v.is_cuda or not v.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous device int64 tensor of {B} elements")
        check(lib.eegldm_window_batch(self.ctx.h, ptr(self.bank), self.total, ptr(d["seg_first"]), ptr(d["seg_cum"]), ptr(d["seg_label"]),
                                      t.n_seg, ptr(d["group_bounds"]), t.n_group, ptr(group), ptr(idx), int(seed), int(offset),
                                      self.window, self.border, ptr(out), out.stride(0), ptr(labels), ptr(src), B))
        return out, labels, src


class DeviceWindowLoader:
    """Iterable of {"eeg": (B, 1, window + 2 border) device fp32, "label": (B,) device int64 (banks with stages only)} over a WindowBank.

    sampling  "recording": the host loader's epoch -- every recording `windows_per_recording` times, in an order permuted by numpy
              (Generator seeded by (seed, epoch); one int64 array uploaded per epoch), the crop drawn on the device within the recording;
              "uniform": every window drawn over all valid starts of the bank (long recordings are seen in proportion to their length);
              "balanced": the class drawn first -- eegldm_randint over the classes present, or from `class_probs` (one probability per
              class present, in ascending label order, or a {label: probability} dict) -- then the start uniformly within the class.
    An epoch is len(files) * windows_per_recording windows in every mode.  Window number n of the run (counted over epochs) takes its crop
    from Philox(seed, n) and its class from Philox(seed ^ CLASS_KEY, n): a batch is a function of (seed, position), and state_dict() /
    load_state_dict() make a resumed run draw what the uninterrupted one would.  with_src=True adds "src": (B,) device int64, the bank index
    of every window's first sample (bank.locate translates it to (recording, start))."""

    def __init__(self, bank, batch_size, seed, sampling="recording", windows_per_recording=1, class_probs=None, drop_last=False, shuffle=True,
                 with_src=False):
        if sampling not in SAMPLINGS:
            raise ValueError(f"sampling {sampling!r}: one of {SAMPLINGS}")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size {batch_size} must be >= 1")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed {seed} must fit 64 unsigned bits")
        if class_probs is not None and sampling != "balanced":
            raise ValueError("class_probs goes with sampling='balanced'")
        self.bank, self.batch_size, self.seed, self.sampling = bank, int(batch_size), int(seed), sampling
        self.wpr, self.drop_last, self.shuffle, self.with_src = max(1, int(windows_per_recording)), drop_last, shuffle, bool(with_src)
        self.n = bank.n_rec * self.wpr
        self.cum_probs = None
        if sampling == "recording":
            a = bank.table_a
            empty = np.flatnonzero(a.group_bounds[1:] == a.group_bounds[:-1])
            if len(empty):
                raise ValueError(f"{bank.files[int(empty[0])]}: no scored epoch under any window centre; sampling='recording' visits every "
                                 "recording (use 'uniform' or 'balanced', or drop the file)")
        elif bank.table_a.total < 1:
            raise ValueError("the bank has no valid crop start with a scored centre")
        if sampling == "balanced":
            if not bank.has_stages:
                raise ValueError("sampling='balanced' needs stages")
            if class_probs is not None:
                if isinstance(class_probs, dict):
                    unknown = sorted(set(class_probs) - set(bank.classes))
                    if unknown:
                        raise ValueError(f"class_probs names classes {unknown} that the bank does not hold (present: {bank.classes})")
                    class_probs = [class_probs.get(c, 0.0) for c in bank.classes]
                p = np.asarray(class_probs, np.float64)
                if p.shape != (len(bank.classes),) or not np.all(np.isfinite(p)) or np.any(p < 0) or abs(p.sum() - 1.0) > 1e-6:
                    raise ValueError(f"class_probs must be {len(bank.classes)} probabilities summing to 1 (classes present: {bank.classes}), got {class_probs}")
                self.cum_probs = np.cumsum(p) / p.sum()
        self.epoch, self.batch, self.drawn, self._resume = 0, 0, 0, False
        self._cum_dev = None

    def __len__(self):
        return self.n // self.batch_size if self.drop_last else -(-self.n // self.batch_size)

    def state_dict(self):
        return {"epoch": self.epoch, "batch": self.batch, "drawn": self.drawn, "seed": self.seed, "sampling": self.sampling, "n": self.n,
                "batch_size": self.batch_size}

    def load_state_dict(self, sd):
        for k in ("seed", "sampling", "n", "batch_size"):
            if sd[k] != getattr(self, k):
                raise ValueError(f"the saved loader state has {k} = {sd[k]}, this loader {getattr(self, k)}: the runs would not draw alike")
        self.epoch, self.batch, self.drawn = int(sd["epoch"]), int(sd["batch"]), int(sd["drawn"])
        self._resume = self.batch > 0

    def order(self, epoch):
        """The recording of every window of `epoch` under "recording" sampling (host int64)."""
        order = np.random.default_rng([self.seed, int(epoch)]).permutation(self.n) if self.shuffle else np.arange(self.n)
        return (order // self.wpr).astype(np.int64)

    def classes_drawn(self, b, offset):
        """The group (index into bank.classes) of windows offset .. offset + b under "balanced" sampling: a device int64 tensor."""
        bank = self.bank
        out = torch.empty(b, dtype=torch.int64, device=bank.device)
        key = self.seed ^ CLASS_KEY
        if self.cum_probs is None:
            check(lib.eegldm_randint(bank.ctx.h, ptr(out), b, len(bank.classes), key, offset))
            return out
        check(lib.eegldm_randint(bank.ctx.h, ptr(out), b, 1 << 53, key, offset))
        if self._cum_dev is None:
            self._cum_dev = torch.from_numpy(self.cum_probs).to(bank.device)
        u = out.to(torch.float64) * (2.0 ** -53)                                  # exact: [0, 1) on a 2^-53 grid
        return torch.searchsorted(self._cum_dev, u, right=True).clamp_(max=len(bank.classes) - 1)

    def __iter__(self):
        bank = self.bank
        if not bank.uploaded:
            raise RuntimeError("this bank was built with upload=False: it has no device side")
        if self.batch and not self._resume:          # the last pass was abandoned mid-epoch: the next one is a new epoch
            self.epoch, self.batch = self.epoch + 1, 0
        self._resume = False
        order = torch.from_numpy(self.order(self.epoch)).to(bank.device) if self.sampling == "recording" else None
        while self.batch < len(self):
            k = self.batch
            b = min(self.batch_size, self.n - k * self.batch_size)
            if self.sampling == "recording":
                eeg, labels, src = bank.batch(b, "recording", group=order[k * self.batch_size:k * self.batch_size + b], seed=self.seed, offset=self.drawn,
                                              want_src=self.with_src)
            elif self.sampling == "uniform":
                eeg, labels, src = bank.batch(b, "recording", seed=self.seed, offset=self.drawn, want_src=self.with_src)
            else:
                eeg, labels, src = bank.batch(b, "label", group=self.classes_drawn(b, self.drawn), seed=self.seed, offset=self.drawn, want_src=self.with_src)
            # the state moves BEFORE the yield: a state_dict() taken by the consumer of batch k describes "batch k + 1 is next"
            self.drawn += b; self.batch += 1
            last = self.batch >= len(self)
            if last:
                self.epoch, self.batch = self.epoch + 1, 0
            item = {"eeg": eeg, "label": labels} if bank.has_stages else {"eeg": eeg}
            if self.with_src:
                item["src"] = src
            yield item
            if last:
                return
