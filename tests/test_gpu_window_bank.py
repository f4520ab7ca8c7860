"""-m gpu: the device-resident window bank.  eegldm_bank_normalise against numpy's normalise_recording byte for byte over ragged rows;
eegldm_window_batch against crop_and_pad / centre_label byte for byte with injected indices, and against the restated draw rule with the
draw taken from eegldm_randint itself; the DeviceWindowLoader's epoch, resume and class draw; the training scripts with --device_loader."""
import os

import numpy as np
import pytest
import torch
import yaml

import gpu_util as G
from eegldm.data import BANK_CHUNK, DeviceWindowLoader, WindowBank
from eegldm.entry.common import BORDER, EPOCH, WINDOW, centre_label, crop_and_pad, normalise_recording

pytestmark = pytest.mark.gpu
lib, ptr = G.lib, G.ptr
INT64_MIN = -2 ** 63
E = EPOCH


def last_error():
    return lib.eegldm_last_error().decode()


def raw_row(rng, n):
    """EEG-like volts: the scaled values are of order 10 and their minimum is not a zero."""
    return (rng.standard_normal(n) * 1e-5 + 3e-6 * np.sin(np.arange(n) / 50.0)).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(G.DEV)


# ------------------------------------------------------------------------------------------------------------------ normalise
def normalise(rows, lead=0):
    """rows at [lead, ...) of one flat device buffer -> (bank tensor after the call, lohi (n, 2) numpy, row_off)."""
    row_off = lead + np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = np.full(int(row_off[-1]) + 3, 7.0, np.float32)            # sentinels ahead of the first and behind the last row
    for r, row in enumerate(rows):
        flat[row_off[r]:row_off[r + 1]] = row
    bank, lohi = dev(flat), torch.full((len(rows), 2), 5.0, device=G.DEV)
    nws = 2 * (int(row_off[-1]) // BANK_CHUNK + len(rows) + 1)
    ws = torch.full((nws,), float("nan"), device=G.DEV)              # "contents irrelevant"
    G.check(lib.eegldm_bank_normalise(G.ctx().h, ptr(bank), ptr(dev(row_off)), row_off.ctypes.data, len(rows), ptr(lohi), ptr(ws), nws))
    torch.cuda.synchronize()
    out = bank.cpu().numpy()
    assert (out[:lead] == 7.0).all() and (out[row_off[-1]:] == 7.0).all(), "wrote outside the rows"
    return out, lohi.cpu().numpy(), row_off


def assert_rows_equal_numpy(rows, out, lohi, row_off):
    for r, row in enumerate(rows):
        want = normalise_recording(row)
        a = row * np.float32(1.0 + 1e6)
        got = out[row_off[r]:row_off[r + 1]]
        assert got.tobytes() == want.tobytes(), f"row {r} ({len(row)} samples at offset {row_off[r]}): {int((got != want).sum())} elements differ"
        assert lohi[r].tobytes() == np.array([a.min(), a.max()], np.float32).tobytes()


def test_normalise_row_lengths_bytes_equal_numpy():
    """One row shorter than a chunk, chunk - 1 / chunk / chunk + 1 samples, several chunks with a ragged last one; the rows follow each other
    in one bank, so they also start at offsets 0, 0, 1, 0, 0, 1 mod 4."""
    rng = np.random.default_rng(1)
    rows = [raw_row(rng, n) for n in (3000, 3001, 16383, 16384, 16385, 100003)]
    out, lohi, row_off = normalise(rows)
    assert_rows_equal_numpy(rows, out, lohi, row_off)
    out2, lohi2, _ = normalise(rows)
    assert out.tobytes() == out2.tobytes() and lohi.tobytes() == lohi2.tobytes()          # two runs agree


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_normalise_ragged_rows_on_every_alignment(lead):
    """3001, 7001 and 16385 samples: the four row boundaries fall on offsets 0, 1, 2, 3 mod 4 (shifted by `lead`)."""
    rng = np.random.default_rng(2)
    rows = [raw_row(rng, n) for n in (3001, 7001, 16385)]
    out, lohi, row_off = normalise(rows, lead)
    assert sorted((row_off % 4).tolist()) == [0, 1, 2, 3]
    assert_rows_equal_numpy(rows, out, lohi, row_off)


def test_normalise_constant_and_nan_rows():
    rng = np.random.default_rng(3)
    nan_row = raw_row(rng, 40001); nan_row[33333] = np.nan          # in the third chunk of the row
    rows = [raw_row(rng, 3003), np.full(5001, 2.5e-5, np.float32), raw_row(rng, 3002), nan_row, raw_row(rng, 20001)]
    out, lohi, row_off = normalise(rows)
    seg = lambda r: out[row_off[r]:row_off[r + 1]]
    assert (seg(1).view(np.int32) == 0).all()                       # constant -> exact +0
    assert lohi[1, 0] == lohi[1, 1] == np.float32(2.5e-5) * np.float32(1.0 + 1e6)
    assert np.isnan(seg(3)).all() and np.isnan(lohi[3]).all()       # as numpy: min / max keep the NaN
    assert np.isnan(normalise_recording(nan_row)).all()
    for r in (0, 2, 4):                                             # the neighbours keep numpy's bytes
        assert seg(r).tobytes() == normalise_recording(rows[r]).tobytes()
        assert np.isfinite(lohi[r]).all()


def test_normalise_refusals_leave_everything_untouched():
    rows = [np.arange(3000, dtype=np.float32), np.arange(3000, dtype=np.float32)]
    row_off = np.array([0, 3000, 6000], np.int64)
    bank, lohi, ws = dev(np.concatenate(rows)), torch.full((2, 2), 5.0, device=G.DEV), torch.zeros(64, device=G.DEV)
    ro = dev(row_off)
    h = G.ctx().h
    cases = [
        (lambda: lib.eegldm_bank_normalise(h, None, ptr(ro), row_off.ctypes.data, 2, ptr(lohi), ptr(ws), 64), "null"),
        (lambda: lib.eegldm_bank_normalise(h, ptr(bank), ptr(ro), None, 2, ptr(lohi), ptr(ws), 64), "null"),
        (lambda: lib.eegldm_bank_normalise(h, ptr(bank), ptr(ro), row_off.ctypes.data, 0, ptr(lohi), ptr(ws), 64), "n_rec"),
        (lambda: lib.eegldm_bank_normalise(h, ptr(bank), ptr(ro), row_off.ctypes.data, 2, ptr(lohi), ptr(ws), 5), "workspace"),
    ]
    bad_off = np.array([0, 3000, 3000], np.int64)
    cases.append((lambda: lib.eegldm_bank_normalise(h, ptr(bank), ptr(ro), bad_off.ctypes.data, 2, ptr(lohi), ptr(ws), 64), "row 1 has 0 samples"))
    for call, msg in cases:
        assert call() != 0 and msg in last_error(), (msg, last_error())
    torch.cuda.synchronize()
    assert bank.cpu().numpy().tobytes() == np.concatenate(rows).tobytes() and (lohi == 5.0).all()


def test_bank_refuses_a_non_finite_recording_by_name(tmp_path):
    rng = np.random.default_rng(4)
    good, bad = raw_row(rng, 3500), raw_row(rng, 3200); bad[17] = np.inf
    f0, f1 = str(tmp_path / "good.npy"), str(tmp_path / "bad.npy")
    np.save(f0, good); np.save(f1, bad)
    with pytest.raises(ValueError, match=r"bad\.npy: scaled minimum .* is not finite"):
        WindowBank([f0, f1])
    big = (good.astype(np.float64) * 1e38).astype(np.float32)      # about 1e33: finite in the file, x * (1 + 1e6) = 1e39 overflows float32
    with np.errstate(over="ignore"):
        assert np.isfinite(big).all() and not np.isfinite(big * np.float32(1.0 + 1e6)).all()
    np.save(f1, big)
    with pytest.raises(ValueError, match=r"bad\.npy: scaled minimum .* is not finite"):
        WindowBank([f0, f1])


# ------------------------------------------------------------------------------------------------------------------ the banks of the batch tests
LENGTHS = (4 * E, 4 * E + 1, 4 * E + 2, 4 * E + 3)                # 4 epochs each; rows start at offsets 0, 0, 1, 3 mod 4
STAGES = (np.array([0, 1, -1, 2]), np.array([3, -1, 1, 1]), np.array([2, 2, 0, 4]), np.array([1, 0, 3, 2, 2]))


class Banked:
    pass


@pytest.fixture(scope="module")
def banked(tmp_path_factory):
    """Four tiny recordings on disk, banked with and without stages; the numpy references are computed once and never modified."""
    root = tmp_path_factory.mktemp("bank")
    rng = np.random.default_rng(5)
    b = Banked()
    b.root, b.files, b.sfiles, b.raw = str(root), [], [], []
    for r, L in enumerate(LENGTHS):
        f, s = str(root / f"rec{r}.npy"), str(root / f"rec{r}.stages.npy")
        raw = raw_row(rng, L)
        np.save(f, raw.reshape(1, L)); np.save(s, STAGES[r])       # (1, L): the bank flattens as normalise_recording does
        b.files.append(f); b.sfiles.append(s); b.raw.append(raw)
    b.recs = [normalise_recording(x) for x in b.raw]
    for x in b.recs:
        x.setflags(write=False)
    b.plain, b.staged = WindowBank(b.files), WindowBank(b.files, b.sfiles)
    with open(str(root / "ids.csv"), "w") as f:
        f.write("FILE_NAME_EEG\n" + "".join(f"rec{r}\n" for r in range(len(LENGTHS))))
    with open(str(root / "ids8.csv"), "w") as f:      # every recording twice: a batch of 8
        f.write("FILE_NAME_EEG\n" + "".join(f"rec{r % 4}\n" for r in range(8)))
    return b


def reference_rows(b, bank, src, window=WINDOW, border=BORDER):
    """numpy rows and labels for bank indices `src` (crop_and_pad / centre_label for the loader's window)."""
    rows, labs = [], []
    for s in np.asarray(src):
        r, start = bank.locate(int(s))
        if (window, border) == (WINDOW, BORDER):
            rows.append(crop_and_pad(b.recs[r], start)[0])
        else:
            w = np.zeros(window + 2 * border, np.float32); w[border:border + window] = b.recs[r][start:start + window]; rows.append(w)
        labs.append(centre_label(STAGES[r], start) if bank.has_stages else -1)
    return np.stack(rows), np.asarray(labs, np.int64)


def test_bank_bytes_equal_numpy(banked):
    for bank in (banked.plain, banked.staged):
        flat = bank.bank.cpu().numpy()
        assert flat.shape == (sum(LENGTHS),)                        # sized exactly: the last window ends at the last element
        for r in range(len(LENGTHS)):
            assert flat[bank.row_off[r]:bank.row_off[r + 1]].tobytes() == banked.recs[r].tobytes()
            a = banked.raw[r] * np.float32(1.0 + 1e6)
            assert bank.lohi[r].tolist() == [a.min(), a.max()]


@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("staged", [False, True])
def test_batch_with_injected_indices(banked, B, staged):
    bank = banked.staged if staged else banked.plain
    t = bank.table_a
    rng = np.random.default_rng(B)
    idx = rng.integers(0, t.total, B)
    # the corners: first and last valid start of the first and the last recording, and starts 0..3 (src % 4 = 0..3) of recording 0
    corners = [bank.index_of(0, 0), bank.index_of(0, LENGTHS[0] - WINDOW), bank.index_of(3, 0), bank.index_of(3, LENGTHS[3] - WINDOW)]
    corners += [bank.index_of(0, s) for s in (1, 2, 3)]
    idx[:min(B, len(corners))] = corners[:B] if B < len(corners) else corners
    if B == 1:
        idx[0] = corners[3]                                         # the window that ends at the bank's last element
    eeg, labels, src = bank.batch(B, idx=dev(idx), want_src=True)
    torch.cuda.synchronize()
    want_src = t.lookup(idx)[0]
    assert np.array_equal(src.cpu().numpy(), want_src)
    if B >= 7:
        assert sorted(set((want_src[:7] % 4).tolist())) == [0, 1, 2, 3]
    rows, labs = reference_rows(banked, bank, want_src)
    got = eeg.cpu().numpy()
    assert got.shape == (B, 1, WINDOW + 2 * BORDER) and got[:, 0].tobytes() == rows.tobytes()
    assert (got[:, 0, :BORDER].view(np.int32) == 0).all() and (got[:, 0, -BORDER:].view(np.int32) == 0).all()      # +0, not -0
    assert np.array_equal(labels.cpu().numpy(), labs)
    if staged:
        assert (labs >= 0).all()
        # the same windows through table B: other indices, the same bytes
        idx_b = np.array([bank.index_of(*bank.locate(int(s)), table="label") for s in want_src[:16]])
        eeg_b, labels_b, src_b = bank.batch(len(idx_b), table="label", idx=dev(idx_b), want_src=True)
        assert torch.equal(eeg_b, eeg[:16]) and torch.equal(labels_b, labels[:16]) and torch.equal(src_b, src[:16])


def raw_batch(bank, t, d, B, out, ld, idx=None, group=None, window=None, border=None, seed=0, offset=0, labels=None, src=None, bank_ptr=True,
              first=True, bounds=True):
    """eegldm_window_batch itself, argument by argument (d: the bank's device copy of table t)."""
    return lib.eegldm_window_batch(G.ctx().h, ptr(bank.bank) if bank_ptr else None, bank.total, ptr(d["seg_first"]) if first else None,
                                   ptr(d["seg_cum"]), ptr(d["seg_label"]), t.n_seg, ptr(d["group_bounds"]) if bounds else None, t.n_group,
                                   ptr(group), ptr(idx), seed, offset, bank.window if window is None else window,
                                   bank.border if border is None else border, ptr(out), ld, ptr(labels), ptr(src), B)


@pytest.mark.parametrize("ld", [3072, 3080, 3073])
def test_leading_dimension_and_gutters(banked, ld):
    """ld = 3080: rows stay 16-byte aligned and carry a gutter; ld = 3073: three rows of four start off a 16-byte line (the scalar stores)."""
    bank, B = banked.staged, 6
    t, d = bank.table_a, bank._dev["a"]
    idx = np.random.default_rng(ld).integers(0, t.total, B)
    out = torch.full((B, ld), float("nan"), device=G.DEV)
    labels = torch.zeros(B, dtype=torch.int64, device=G.DEV)
    G.check(raw_batch(bank, t, d, B, out, ld, idx=dev(idx), labels=labels))      # src_out NULL
    got = out.cpu().numpy()
    rows, labs = reference_rows(banked, bank, t.lookup(idx)[0])
    assert got[:, :3072].tobytes() == rows.tobytes() and np.isnan(got[:, 3072:]).all()
    assert np.array_equal(labels.cpu().numpy(), labs)


def test_border_zero_and_labels_null(banked):
    bank, B = banked.plain, 5
    t, d = bank.table_a, bank._dev["a"]
    idx = np.array([0, 1, 2, 3, t.total - 1])
    out = torch.full((B, WINDOW), float("nan"), device=G.DEV)
    G.check(raw_batch(bank, t, d, B, out, WINDOW, idx=dev(idx), border=0))
    rows, _ = reference_rows(banked, bank, t.lookup(idx)[0], WINDOW, 0)
    assert out.cpu().numpy().tobytes() == rows.tobytes()


def test_toy_bank_window_7_border_1(tmp_path):
    """Rows of 9 floats: no row but the first of every four starts on a 16-byte line, windows straddle every group of four."""
    rng = np.random.default_rng(6)
    raws = [raw_row(rng, 23), raw_row(rng, 10)]
    files = []
    for r, x in enumerate(raws):
        files.append(str(tmp_path / f"toy{r}.npy")); np.save(files[-1], x)
    bank = WindowBank(files, window=7, border=1)
    recs = [normalise_recording(x) for x in raws]
    t = bank.table_a
    assert t.total == 17 + 4
    idx = np.arange(t.total)
    eeg, labels, src = bank.batch(t.total, idx=dev(idx), want_src=True)
    got, src = eeg.cpu().numpy()[:, 0], src.cpu().numpy()
    for i in range(t.total):
        r, s = bank.locate(int(src[i]))
        assert (r, s) == ((0, i) if i < 17 else (1, i - 17))
        want = np.zeros(9, np.float32); want[1:8] = recs[r][s:s + 7]
        assert got[i].tobytes() == want.tobytes()
    assert (labels == -1).all()


def test_device_side_errors_give_nan_rows(banked, tmp_path):
    bank, B = banked.staged, 5
    t = bank.table_a
    idx = np.array([7, t.total, 11, -1, t.total - 1])
    eeg, labels, src = bank.batch(B, idx=dev(idx), want_src=True)
    got, lab = eeg.cpu().numpy()[:, 0], labels.cpu().numpy()
    assert np.isnan(got[[1, 3]]).all() and lab[[1, 3]].tolist() == [INT64_MIN, INT64_MIN] and src.cpu().numpy()[[1, 3]].tolist() == [-1, -1]
    rows, labs = reference_rows(banked, bank, t.lookup(idx[[0, 2, 4]])[0])
    assert got[[0, 2, 4]].tobytes() == rows.tobytes() and np.array_equal(lab[[0, 2, 4]], labs)
    # an index outside its group's range, and a group outside the table
    lo1, hi1 = t.group_range(1)
    grp, gidx = dev(np.array([1, 1, 1, 99, -3])), dev(np.array([lo1, hi1, lo1 - 1, lo1, lo1]))
    eeg, labels, _ = bank.batch(5, group=grp, idx=gidx)
    assert labels.cpu().numpy().tolist()[1:] == [INT64_MIN] * 4 and labels[0] >= 0 and torch.isnan(eeg[1:]).all() and not torch.isnan(eeg[0]).any()
    # an empty group: a recording without a scored epoch
    f, s = str(tmp_path / "unscored.npy"), str(tmp_path / "unscored.stages.npy")
    np.save(f, banked.raw[0][:2 * E]); np.save(s, np.array([-1, -1]))
    mixed = WindowBank([banked.files[0], f, banked.files[1]], [banked.sfiles[0], s, banked.sfiles[1]])
    assert mixed.table_a.group_range(1)[0] == mixed.table_a.group_range(1)[1]
    eeg, labels, src = mixed.batch(3, group=dev(np.array([0, 1, 2])), seed=9, want_src=True)
    assert torch.isnan(eeg[1]).all() and int(labels[1]) == INT64_MIN and not torch.isnan(eeg[[0, 2]]).any() and (labels[[0, 2]] >= 0).all()
    assert mixed.locate(int(src[0]))[0] == 0 and mixed.locate(int(src[2]))[0] == 2


def test_batch_refusals_leave_the_outputs_untouched(banked):
    bank, B, ld = banked.staged, 3, 3072
    t, d = bank.table_a, bank._dev["a"]
    out = torch.full((B, ld), 7.0, device=G.DEV)
    labels, src = torch.full((B,), 7, dtype=torch.int64, device=G.DEV), torch.full((B,), 7, dtype=torch.int64, device=G.DEV)
    idx, grp = dev(np.array([0, 1, 2])), dev(np.array([0, 1, 2]))
    kw = dict(idx=idx, labels=labels, src=src)
    cases = [
        (lambda: raw_batch(bank, t, d, B, out, ld, bank_ptr=False, **kw), "null"),
        (lambda: raw_batch(bank, t, d, B, out, ld, first=False, **kw), "null"),
        (lambda: raw_batch(bank, t, d, B, None, ld, **kw), "null"),
        (lambda: raw_batch(bank, t, d, B, out, ld, group=grp, bounds=False, **kw), "group needs group_bounds"),
        (lambda: raw_batch(bank, t, d, B, out, ld, window=0, **kw), "window (0) must be >= 1"),
        (lambda: raw_batch(bank, t, d, B, out, ld, border=-1, **kw), "border (-1) must be >= 0"),
        (lambda: raw_batch(bank, t, d, B, out, 3071, **kw), "ld (3071) is smaller"),
        (lambda: raw_batch(bank, t, d, 0, out, ld, **kw), "B (0) must be >= 1"),
    ]
    for call, msg in cases:
        rc = call()
        assert rc != 0 and msg in last_error(), (msg, rc, last_error())
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (labels == 7).all() and (src == 7).all()
    with pytest.raises(ValueError, match="contiguous device int64"):
        bank.batch(B, idx=torch.zeros(B, dtype=torch.int32, device=G.DEV))


# ------------------------------------------------------------------------------------------------------------------ drawn
def randint(n, high, seed, offset):
    out = torch.empty(n, dtype=torch.int64, device=G.DEV)
    G.check(lib.eegldm_randint(G.ctx().h, ptr(out), n, int(high), seed, offset))
    return out.cpu().numpy()


def restated_draw(t, B, seed, offset, group=None):
    """lo + eegldm_randint(high = hi - lo, seed, offset)[b], one eegldm_randint call of B values per distinct `high`."""
    if group is None:
        lo, hi = np.zeros(B, np.int64), np.full(B, t.total, np.int64)
    else:
        lo, hi = t.seg_cum[t.group_bounds[group]], t.seg_cum[t.group_bounds[group + 1]]
    idx = np.empty(B, np.int64)
    for high in np.unique(hi - lo):
        r = randint(B, high, seed, offset)
        m = (hi - lo) == high
        idx[m] = lo[m] + r[m]
    return idx


@pytest.mark.parametrize("mode", ["whole_table", "recording_groups", "label_groups"])
def test_drawn_windows_follow_the_restated_rule(banked, mode):
    bank, B, seed, offset = banked.staged, 300, 0xC0FFEE12345, 2 ** 33 + 5
    which = "label" if mode == "label_groups" else "recording"
    t = bank.table(which)
    group = None if mode == "whole_table" else np.random.default_rng(7).integers(0, t.n_group, B)
    eeg, labels, src = bank.batch(B, table=which, group=None if group is None else dev(group), seed=seed, offset=offset, want_src=True)
    idx = restated_draw(t, B, seed, offset, group)
    want_src, want_lab, want_rec = t.lookup(idx)
    assert np.array_equal(src.cpu().numpy(), want_src)
    rows, labs = reference_rows(banked, bank, want_src)
    assert eeg.cpu().numpy()[:, 0].tobytes() == rows.tobytes() and np.array_equal(labels.cpu().numpy(), labs) and np.array_equal(labs, want_lab)
    if mode == "recording_groups":
        assert np.array_equal(want_rec, group)
    if mode == "label_groups":
        assert np.array_equal(labs, t.group_keys[group])
    # offset = k: rows k .. of the offset-0 batch, where the groups agree
    k = 37
    base = bank.batch(B, table=which, group=None if group is None else dev(group), seed=seed, offset=0, want_src=True)
    shifted = bank.batch(B - k, table=which, group=None if group is None else dev(group[k:]), seed=seed, offset=k, want_src=True)
    for x, y in zip(base, shifted):
        assert torch.equal(x[k:], y)
    assert not torch.equal(base[2][:B - k], shifted[2])


# ------------------------------------------------------------------------------------------------------------------ loader
def collect(loader, n_batches=None):
    out = []
    for i, b in enumerate(loader):
        out.append({k: v.clone() for k, v in b.items()})
        if n_batches is not None and i + 1 == n_batches:
            break
    return out


def test_loader_recording_epoch(banked):
    bank = banked.staged
    ld = DeviceWindowLoader(bank, 5, seed=11, sampling="recording", windows_per_recording=3, with_src=True)
    assert len(ld) == 3
    orders = []
    for _epoch in range(2):
        bs = collect(ld)
        assert [b["eeg"].shape[0] for b in bs] == [5, 5, 2] and all(b["eeg"].shape[1:] == (1, 3072) and b["eeg"].is_cuda for b in bs)
        src = torch.cat([b["src"] for b in bs]).cpu().numpy(); lab = torch.cat([b["label"] for b in bs]).cpu().numpy()
        recs = np.array([bank.locate(int(s))[0] for s in src])
        assert np.bincount(recs, minlength=4).tolist() == [3, 3, 3, 3]            # every recording windows_per_recording times
        rows, labs = reference_rows(banked, bank, src)
        assert torch.cat([b["eeg"] for b in bs]).cpu().numpy()[:, 0].tobytes() == rows.tobytes() and np.array_equal(lab, labs)
        assert lab.dtype == np.int64 and (lab >= 0).all()
        orders.append(recs.tolist())
    assert orders[0] == ld.order(0).tolist() and orders[1] == ld.order(1).tolist() and ld.epoch == 2 and ld.drawn == 24
    plain = collect(DeviceWindowLoader(banked.plain, 4, seed=11, drop_last=True))
    assert len(plain) == 1 and set(plain[0]) == {"eeg"}                           # no stages: no "label"


@pytest.mark.parametrize("sampling", ["recording", "uniform", "balanced"])
def test_loader_state_dict_round_trip_mid_epoch(banked, sampling):
    make = lambda: DeviceWindowLoader(banked.staged, 3, seed=21, sampling=sampling, windows_per_recording=4, with_src=True)
    whole = make()
    full = collect(whole) + collect(whole)                                        # two epochs of 6 batches (16 windows: 5 x 3 + 1)
    assert len(full) == 12
    first = make()
    head = collect(first, 2)
    sd = first.state_dict()
    assert sd["batch"] == 2 and sd["drawn"] == 6 and sd["epoch"] == 0
    resumed = make()
    resumed.load_state_dict(sd)
    tail = collect(resumed) + collect(resumed)
    assert len(head) + len(tail) == 12
    for a, b in zip(full, head + tail):
        assert set(a) == set(b) == {"eeg", "label", "src"}
        for k in a:
            assert torch.equal(a[k], b[k]), k
    # a pass abandoned mid-epoch and not resumed: the next pass is the next epoch's, whole
    assert len(collect(first)) == 6 and first.epoch == 2


def test_loader_balanced_labels_are_the_drawn_classes(banked):
    bank = banked.staged
    assert bank.classes == [0, 1, 2, 3, 4]
    ld = DeviceWindowLoader(bank, 64, seed=31, sampling="balanced", windows_per_recording=32)
    assert len(ld) == 2
    off = 0
    for b in ld:
        n = b["label"].shape[0]
        cls = randint(n, 5, 31 ^ 0x9E3779B97F4A7C15, off)                          # the class key, the window's own counter
        assert np.array_equal(b["label"].cpu().numpy(), np.asarray(bank.classes)[cls])
        off += n
    assert off == 128
    # class_probs: the classes are those of the cumulative table at u = randint(2^53) / 2^53
    probs = {0: 0.5, 3: 0.25, 4: 0.25}
    ld = DeviceWindowLoader(bank, 200, seed=32, sampling="balanced", windows_per_recording=50, class_probs=probs)
    lab = next(iter(ld))["label"].cpu().numpy()
    u = randint(200, 2 ** 53, 32 ^ 0x9E3779B97F4A7C15, 0).astype(np.float64) * 2.0 ** -53
    want = np.searchsorted(np.cumsum([0.5, 0.0, 0.0, 0.25, 0.25]), u, side="right")
    assert np.array_equal(lab, np.asarray(bank.classes)[want]) and set(lab.tolist()) == {0, 3, 4}


# ------------------------------------------------------------------------------------------------------------------ through main
AEKL_YAML = {
    "train": {"seed": 2, "batch_size": 8, "n_epochs": 2, "val_interval": 1, "num_workers": 0, "drop_last": False,
              "output_dir": "OUT", "run_dir": "aekl_eeg", "experiment": "AEKL"},
    "models": {"optimizer_g_lr": 0.005, "optimizer_d_lr": 0.0005, "adv_weight": 0.01, "kl_weight": 1e-9, "spectral_weight": 1e4},
    "autoencoderkl": {"params": {"spatial_dims": 1, "in_channels": 1, "out_channels": 1, "num_res_blocks": 2, "norm_num_groups": 1,
                                 "attention_levels": [False, False, False], "with_encoder_nonlocal_attn": False,
                                 "with_decoder_nonlocal_attn": False, "num_channels": [8, 8, 16], "latent_channels": 1}},
    "patchdiscriminator": {"params": {"spatial_dims": 1, "num_layers_d": 3, "num_channels": 16, "in_channels": 1, "out_channels": 1,
                                      "kernel_size": 3, "norm": "BATCH", "bias": False, "padding": 1}},
}


def test_train_autoencoderkl_with_the_device_loader(banked, tmp_path, capsys):
    import math
    from eegldm.entry import train_autoencoderkl as TA
    cfg = dict(AEKL_YAML); cfg["train"] = dict(cfg["train"], output_dir=str(tmp_path))
    y = str(tmp_path / "aekl.yaml")
    yaml.safe_dump(cfg, open(y, "w"))
    ids = os.path.join(banked.root, "ids8.csv")
    run = TA.main(TA.parse_args(["--config_file", y, "--path_train_ids", ids, "--path_valid_ids", ids, "--path_pre_processed", banked.root,
                                 "--latent_channels", "1", "--device_loader", "--sampling", "uniform"]))
    assert TA.LAST_RUN["steps"] == 2 and math.isfinite(TA.LAST_RUN["ae_sum"]) and math.isfinite(TA.LAST_RUN["d_sum"])
    ck = torch.load(os.path.join(run, "checkpoint.pth"))
    assert math.isfinite(ck["best_loss"]) and tuple(ck["init_batch"].shape) == (8, 1, 3000)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and "nan" not in " ".join(lines).lower(), lines


def test_train_usleep_with_and_without_the_device_loader(banked, tmp_path):
    import math
    from eegldm.entry import train_usleep as TU
    ids = os.path.join(banked.root, "ids.csv")
    common = ["--path_train_ids", ids, "--path_valid_ids", ids, "--path_pre_processed", banked.root, "--depth", "4", "--batch_size", "8",
              "--windows_per_recording", "4", "--n_epochs", "2", "--seed", "0"]
    rep = TU.main(TU.parse_args(["--output_dir", str(tmp_path / "dev")] + common + ["--device_loader", "--sampling", "balanced", "--class_weights", "balanced"]))
    assert [h["steps"] for h in rep["history"]] == [2, 2] and all(math.isfinite(h["train_loss"]) for h in rep["history"])
    assert all(0.0 <= h["valid"]["balanced_accuracy"] <= 1.0 for h in rep["history"]) and len(rep["class_weight"]) == 5
    host = TU.main(TU.parse_args(["--output_dir", str(tmp_path / "host")] + common))
    assert [h["steps"] for h in host["history"]] == [2, 2] and all(math.isfinite(h["train_loss"]) for h in host["history"])
    assert host["args"]["device_loader"] is False
