"""CPU: the host side of the device-resident window bank (eegldm.data) -- the segment tables against a brute-force enumeration of every
crop start with centre_label, table B as a regrouping of table A, every refusal of the Python layer, and the draw rule restated with
tests/context_ref.philox4x32 (the generator the GPU tests pin to the device bit for bit): label frequencies of 20 000 draws against the
table's own proportions ("uniform") and against 1 / K' ("balanced")."""
import math
import os

import numpy as np
import pytest

import context_ref as R
from eegldm.data import CLASS_KEY, DeviceWindowLoader, SegmentTable, WindowBank, draw_indices, segment_tables
from eegldm.entry.common import EPOCH, WINDOW, centre_label

E = EPOCH


def brute_force(lengths, stages):
    """Every (recording, start) whose centre is scored, in (recording, start) order -> (bank index, label, recording) arrays."""
    src, lab, rec, off = [], [], [], 0
    for r, L in enumerate(lengths):
        for s in range(0, L - WINDOW + 1):
            c = centre_label(stages[r], s) if stages is not None else -1
            if stages is None or c >= 0:
                src.append(off + s); lab.append(c); rec.append(r)
        off += L
    return np.asarray(src, np.int64), np.asarray(lab, np.int64), np.asarray(rec, np.int64)


# hypnograms chosen for the edges of the rule: unscored first / middle / last epochs, a hypnogram shorter and longer than the recording,
# recordings of exactly one window, one window + 1, 1.5 epochs - 1, 1.5 epochs, 3 epochs + 17, and an all-unscored recording
CASES = {
    "unscored_first_middle_last": ([5 * E, 5 * E + 7], [np.array([-1, 0, -1, 2, -1]), np.array([1, 1, -2, 3, 4])]),
    "hypnogram_shorter": ([4 * E + 100], [np.array([2, 3])]),
    "hypnogram_longer": ([2 * E + 50], [np.array([0, 1, 2, 3, 4, 0, 1])]),
    "L_3000": ([3000], [np.array([4])]),
    "L_3001": ([3001], [np.array([4, 1])]),
    "L_4499": ([4499], [np.array([0, 1])]),
    "L_4500": ([4500], [np.array([0, 1])]),
    "L_3_epochs_17": ([3 * E + 17, 3000, 4500], [np.array([1, -1, 2, 0]), np.array([0]), np.array([3, 3])]),
    "one_all_unscored": ([2 * E, 2 * E + 1], [np.array([-1, -1]), np.array([0, 2])]),
    "int32_codes": ([2 * E], [np.array([1, 2], np.int32)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_against_brute_force(name):
    lengths, stages = CASES[name]
    src, lab, rec = brute_force(lengths, stages)
    a, b, row_off = segment_tables(lengths, stages)
    assert row_off.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert a.total == b.total == len(src)
    # table A in (recording, epoch) order IS the (recording, start) order: the ordered map idx -> (start, label) must be equal
    got_src, got_lab, got_rec = a.lookup(np.arange(a.total))
    assert np.array_equal(got_src, src) and np.array_equal(got_lab, lab) and np.array_equal(got_rec, rec)
    # groups of A are the recordings
    assert a.n_group == len(lengths)
    for r in range(len(lengths)):
        lo, hi = a.group_range(r)
        assert hi - lo == int((rec == r).sum()) and (hi == lo or (got_rec[lo:hi] == r).all())
    # table B: the same starts, grouped by label in ascending label order, (recording, start) order inside a label
    bs, bl, br = b.lookup(np.arange(b.total))
    assert sorted(bs.tolist()) == src.tolist() and len(set(bs.tolist())) == len(bs)
    assert b.group_keys.tolist() == sorted(set(lab.tolist()))
    for g, key in enumerate(b.group_keys):
        lo, hi = b.group_range(g)
        assert hi > lo and (bl[lo:hi] == key).all() and np.array_equal(bs[lo:hi], src[lab == key])
    assert b.group_range(b.n_group - 1)[1] == b.total and b.group_range(0)[0] == 0
    # no empty runs, no float anywhere
    for t in (a, b):
        assert (np.diff(t.seg_cum) > 0).all() and t.seg_first.dtype == t.seg_cum.dtype == t.group_bounds.dtype == np.int64
        assert t.seg_label.dtype == np.int32


def test_tables_without_stages():
    lengths = [3000, 3001, 10 * E + 123]
    src, lab, rec = brute_force(lengths, None)
    a, b, _ = segment_tables(lengths)
    assert a.n_seg == 3 and a.seg_label.tolist() == [-1, -1, -1] and a.total == len(src)
    assert np.array_equal(a.lookup(np.arange(a.total))[0], src)
    assert b.n_group == 1 and b.group_keys.tolist() == [-1] and np.array_equal(b.lookup(np.arange(b.total))[0], src)


def test_all_unscored_recording_has_an_empty_group():
    a, b, _ = segment_tables(*CASES["one_all_unscored"])
    assert a.group_range(0) == (0, 0) and a.group_range(1)[1] == a.total > 0
    with pytest.raises(ValueError, match="empty range"):
        draw_indices(a, np.array([5], np.uint64), group=np.array([0]))
    with pytest.raises(IndexError):
        a.lookup([a.total])


def test_other_window_lengths_follow_the_centre_rule():
    """window = 7 on a toy bank (the GPU test's shape): starts whose centre s + 3 lies in a scored epoch."""
    a, _b, _ = segment_tables([E + 20], [np.array([2, 0])], window=7)
    src, lab, _ = a.lookup(np.arange(a.total))
    want = [(s, [2, 0][(s + 3) // E]) for s in range(E + 20 - 7 + 1)]
    assert list(zip(src.tolist(), lab.tolist())) == want


# ------------------------------------------------------------------------------------------------------------------ refusals
def _write(tmp_path, lengths, stages=None, dtype=np.float32):
    files, sfiles = [], []
    rng = np.random.default_rng(0)
    for r, L in enumerate(lengths):
        f = os.path.join(tmp_path, f"rec{r}.npy"); np.save(f, (rng.standard_normal(L) * 1e-5).astype(dtype)); files.append(f)
        if stages is not None:
            s = os.path.join(tmp_path, f"rec{r}.stages.npy"); np.save(s, stages[r]); sfiles.append(s)
    return files, (sfiles if stages is not None else None)


def test_bank_refusals_name_the_file(tmp_path):
    files, _ = _write(str(tmp_path), [3000, 2999])
    with pytest.raises(ValueError, match=r"rec1\.npy: 2999 samples"):
        WindowBank(files, upload=False)
    files, sfiles = _write(str(tmp_path), [3000, 6000], [np.array([1]), np.array([0.0, 1.0])])
    with pytest.raises(ValueError, match=r"rec1\.stages\.npy: stage codes must be a 1-D integer array"):
        WindowBank(files, sfiles, upload=False)
    np.save(sfiles[1], np.array([[0, 1]]))
    with pytest.raises(ValueError, match=r"rec1\.stages\.npy"):
        WindowBank(files, sfiles, upload=False)
    with pytest.raises(ValueError, match="stage files for"):
        WindowBank(files, sfiles[:1], upload=False)
    with pytest.raises(ValueError, match="at least one recording"):
        WindowBank([], upload=False)
    with pytest.raises(ValueError, match="border"):
        WindowBank(files, border=-1, upload=False)


def test_host_translations(tmp_path):
    lengths, stages = CASES["L_3_epochs_17"]
    files, sfiles = _write(str(tmp_path), lengths, stages)
    bank = WindowBank(files, sfiles, upload=False)
    assert bank.classes == [0, 1, 2, 3] and bank.n_rec == 3 and bank.total == sum(lengths) and not bank.uploaded
    src, lab, rec = brute_force(lengths, stages)
    for i in (0, 1, 1499, 1500, len(src) - 1):
        r, s = bank.locate(src[i])
        assert r == rec[i] and bank.index_of(r, s) == i
        ib = bank.index_of(r, s, table="label")
        assert bank.table_b.lookup([ib])[0][0] == src[i] and bank.table_b.lookup([ib])[1][0] == lab[i]
    with pytest.raises(ValueError, match="unscored"):
        bank.index_of(0, 3000)            # centre 4500: epoch 1, unscored
    with pytest.raises(ValueError, match="not a valid crop start"):
        bank.index_of(0, lengths[0] - WINDOW + 1)
    with pytest.raises(IndexError):
        bank.locate(bank.total)
    with pytest.raises(RuntimeError, match="upload=False"):
        bank.batch(1)


def test_loader_refusals(tmp_path):
    files, sfiles = _write(str(tmp_path), *CASES["one_all_unscored"])
    bank = WindowBank(files, sfiles, upload=False)
    with pytest.raises(ValueError, match=r"rec0\.npy: no scored epoch"):
        DeviceWindowLoader(bank, 4, 0, sampling="recording")
    DeviceWindowLoader(bank, 4, 0, sampling="uniform"); DeviceWindowLoader(bank, 4, 0, sampling="balanced")
    plain = WindowBank(files, upload=False)
    with pytest.raises(ValueError, match="needs stages"):
        DeviceWindowLoader(plain, 4, 0, sampling="balanced")
    with pytest.raises(ValueError, match="one of"):
        DeviceWindowLoader(plain, 4, 0, sampling="stratified")
    with pytest.raises(ValueError, match="batch_size"):
        DeviceWindowLoader(plain, 0, 0)
    with pytest.raises(ValueError, match="seed"):
        DeviceWindowLoader(plain, 4, -1)
    with pytest.raises(ValueError, match="class_probs goes with"):
        DeviceWindowLoader(plain, 4, 0, class_probs=[1.0])
    for bad in ([0.5, 0.6], [1.0], [-0.5, 1.5], [float("nan"), 1.0], {7: 1.0}):
        with pytest.raises(ValueError, match="class_probs"):
            DeviceWindowLoader(bank, 4, 0, sampling="balanced", class_probs=bad)
    ok = DeviceWindowLoader(bank, 4, 0, sampling="balanced", class_probs={2: 1.0})
    assert ok.cum_probs.tolist() == [0.0, 1.0]
    ld = DeviceWindowLoader(plain, 4, 3, windows_per_recording=3)
    assert ld.n == 6 and len(ld) == 2 and len(DeviceWindowLoader(plain, 4, 3, windows_per_recording=3, drop_last=True)) == 1
    with pytest.raises(ValueError, match="seed"):
        ld.load_state_dict({**ld.state_dict(), "seed": 4})
    with pytest.raises(RuntimeError, match="upload=False"):
        next(iter(ld))
    # the epoch's order: every recording windows_per_recording times, another permutation per epoch, the same one for the same epoch
    assert sorted(ld.order(0).tolist()) == [0, 0, 0, 1, 1, 1] and ld.order(5).tolist() == ld.order(5).tolist()
    assert DeviceWindowLoader(plain, 4, 3, windows_per_recording=3, shuffle=False).order(1).tolist() == [0, 0, 0, 1, 1, 1]


def test_script_flags():
    from eegldm.entry import train_autoencoderkl, train_dm, train_ldm, train_usleep
    from eegldm.entry.common import window_loader
    for mod, base in ((train_autoencoderkl, ["--config_file", "x"]), (train_dm, ["--config_file", "x"]), (train_ldm, ["--config_file", "x", "--autoencoderkl_config_file_path", "y"]),
                      (train_usleep, ["--output_dir", "x"])):
        a = mod.parse_args(base)
        assert a.device_loader is False and a.sampling == "recording"
        a = mod.parse_args(base + ["--device_loader", "--sampling", "balanced"])
        assert a.device_loader is True and a.sampling == "balanced"
        with pytest.raises(SystemExit):
            mod.parse_args(base + ["--sampling", "stratified"])
    a = train_dm.parse_args(["--config_file", "x", "--sampling", "uniform"])
    with pytest.raises(ValueError, match="needs --device_loader"):
        window_loader(a, None, 4, 8, seed=1)
    a = train_dm.parse_args(["--config_file", "x", "--device_loader"])
    with pytest.raises(ValueError, match="not synthetic windows"):
        window_loader(a, None, 4, 8, seed=1)


# ------------------------------------------------------------------------------------------------------------------ the draw rule
def words(seed, offset, n):
    """(r0 << 32) | r1 of Philox(seed, offset + b), b < n: what eegldm_randint reduces modulo `high`."""
    w0, w1, _w2, _w3 = R.philox4x32(seed, np.uint64(offset) + np.arange(n, dtype=np.uint64))
    return (w0.astype(np.uint64) << np.uint64(32)) | w1.astype(np.uint64)


# three classes with unequal shares: 2, 5 and 1 scored epochs, one unscored, the last recording ending inside an epoch
DRAW_BANK = ([4 * E, 5 * E + 1200], [np.array([0, 1, 1, -1]), np.array([1, 0, 1, 2, 1, 1])])
N_DRAWS, SEED = 20000, 20240607
CHI2_DF2_Q = -2.0 * math.log(1e-6)          # the 1 - 1e-6 quantile of chi-square with 2 degrees of freedom (survival exp(-x / 2)): 27.63


def chi_square(counts, probs):
    exp = N_DRAWS * np.asarray(probs, np.float64)
    return float(((np.asarray(counts, np.float64) - exp) ** 2 / exp).sum())


def test_uniform_draws_follow_the_tables_proportions():
    a, _b, _ = segment_tables(*DRAW_BANK)
    v = words(SEED, 0, N_DRAWS)
    idx = (v % np.uint64(a.total)).astype(np.int64)                       # group NULL: lo = 0, hi = total
    assert np.array_equal(idx, draw_indices(a, v))
    _src, lab, _rec = a.lookup(idx)
    _s, all_lab, _r = a.lookup(np.arange(a.total))
    classes = [0, 1, 2]
    probs = [float((all_lab == c).mean()) for c in classes]
    assert len(set(probs)) == 3 and min(probs) > 0.05
    x2 = chi_square([(lab == c).sum() for c in classes], probs)
    assert x2 < CHI2_DF2_Q, x2
    # an offset is a shift of the stream
    assert np.array_equal(draw_indices(a, words(SEED, 77, 100)), idx[77:177])


def test_balanced_draws_are_uniform_over_the_classes_present():
    _a, b, _ = segment_tables(*DRAW_BANK)
    K = b.n_group
    assert K == 3
    cls = (words(SEED ^ CLASS_KEY, 0, N_DRAWS) % np.uint64(K)).astype(np.int64)      # eegldm_randint(K') on the class key
    v = words(SEED, 0, N_DRAWS)
    lo = b.seg_cum[b.group_bounds[cls]]; hi = b.seg_cum[b.group_bounds[cls + 1]]
    idx = lo + (v % (hi - lo).astype(np.uint64)).astype(np.int64)
    assert np.array_equal(idx, draw_indices(b, v, group=cls))
    _src, lab, _rec = b.lookup(idx)
    assert np.array_equal(lab, b.group_keys[cls])                          # the label IS the drawn class
    x2 = chi_square([(lab == c).sum() for c in b.group_keys], [1.0 / K] * K)
    assert x2 < CHI2_DF2_Q, x2
    # within a class the starts are uniform too: halves of the largest class's range are hit equally often (1 degree of freedom:
    # the 1 - 1e-6 quantile is 23.93)
    g = int(np.argmax(np.diff(b.seg_cum[b.group_bounds])))
    lo_g, hi_g = b.group_range(g)
    mine = idx[cls == g]
    first = int((mine < lo_g + (hi_g - lo_g) // 2).sum())
    p = ((hi_g - lo_g) // 2) / (hi_g - lo_g)
    z2 = (first - len(mine) * p) ** 2 / (len(mine) * p * (1 - p))
    assert z2 < 23.93, z2


def test_segment_table_is_plain_data():
    t = SegmentTable([10, 40], [3, 2], [1, -1], [0, 1], [0, 1, 2], [0, 1])
    assert t.seg_cum.tolist() == [0, 3, 5] and t.total == 5 and t.n_seg == 2 and t.n_group == 2
    src, lab, rec = t.lookup([0, 2, 3, 4])
    assert src.tolist() == [10, 12, 40, 41] and lab.tolist() == [1, 1, -1, -1] and rec.tolist() == [0, 0, 1, 1]
