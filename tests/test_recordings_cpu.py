"""CPU: eegldm.recordings without a device.  The EDF / EDF+ / profusion readers against files written by tests/recordings_reference.py, the
stage mapping and the sleep span, the resampling ratio and the filter design (tap counts, symmetry, DC gain, pass- and stop-band bounds on a
2^20-point transform), the float64 reference of the resampler against an independent restatement and against sines it must keep or remove,
every Python refusal of the device calls, and the header's two prototypes."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import recordings_reference as R
from eegldm import recordings as rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (100, 125, 128, 200, 250, 256, 500, 512)
N_TAPS = (75, 367, 2347, 147, 367, 4695, 367, 9387)


# ---------------------------------------------------------------------------------------------------- EDF
def _mixed_edf(path, announce=None, n_rec=7, **kw):
    r = np.random.default_rng(3)
    a = r.integers(-2048, 2048, n_rec * 125).astype(np.int16)
    b = r.integers(-32768, 32768, n_rec * 125).astype(np.int16)
    c = r.integers(-100, 100, n_rec).astype(np.int16)
    sigs = [R.eeg_signal("EEG Fpz-Cz", a, 125), R.eeg_signal("EEG Pz-Oz", b, 125, pmin=-3.2768, pmax=3.2767, dmin=-32768, dmax=32767, dim="mV"),
            R.eeg_signal("Event marker", c, 1, pmin=-5, pmax=5, dmin=-100, dmax=100, dim="V")]
    R.write_edf(path, sigs, record_duration="1", announce=announce, **kw)
    return a, b, c


def test_edf_round_trip(tmp_path):
    p = str(tmp_path / "a.edf")
    a, b, c = _mixed_edf(p)
    out = rec.read_edf(p)
    assert list(out["signals"]) == ["EEG Fpz-Cz", "EEG Pz-Oz", "Event marker"]
    h = out["header"]
    assert h["n_records"] == 7 and h["n_signals"] == 3 and h["startdate"] == "01.01.89" and h["starttime"] == "22.00.00"
    for name, data, rate in (("EEG Fpz-Cz", a, Fraction(125)), ("EEG Pz-Oz", b, Fraction(125)), ("Event marker", c, Fraction(1))):
        s = out["signals"][name]
        assert s["data"].dtype == np.int16 and np.array_equal(s["data"], data)
        assert isinstance(s["sfreq"], Fraction) and s["sfreq"] == rate
    s = out["signals"]["EEG Fpz-Cz"]
    assert s["gain"] == 400.0 / 4095 and s["offset"] == -200.0 + 2048 * (400.0 / 4095) and s["dimension"] == "uV"
    s = out["signals"]["EEG Pz-Oz"]
    assert s["gain"] == (3.2767 + 3.2768) / 65535 and s["offset"] == -3.2768 + 32768 * s["gain"] and s["dimension"] == "mV"
    only = rec.read_edf(p, channels=["EEG Pz-Oz"])
    assert list(only["signals"]) == ["EEG Pz-Oz"] and np.array_equal(only["signals"]["EEG Pz-Oz"]["data"], b)


def test_edf_long_records_and_fractional_duration(tmp_path):
    r = np.random.default_rng(4)
    d = r.integers(-2048, 2048, 3 * 3000).astype(np.int16)
    p = R.write_edf(str(tmp_path / "b.edf"), [R.eeg_signal("EEG", d, 3000)], record_duration="30")
    s = rec.read_edf(p)["signals"]["EEG"]
    assert s["sfreq"] == Fraction(100) and np.array_equal(s["data"], d)
    e = r.integers(-5, 5, 4 * 64).astype(np.int16)
    p = R.write_edf(str(tmp_path / "c.edf"), [R.eeg_signal("EEG", e, 64)], record_duration="0.25")
    assert rec.read_edf(p)["signals"]["EEG"]["sfreq"] == Fraction(256)
    p = R.write_edf(str(tmp_path / "d.edf"), [R.eeg_signal("EEG", e, 64)], record_duration="0.3")
    assert rec.read_edf(p)["signals"]["EEG"]["sfreq"] == Fraction(640, 3)


def test_edf_unknown_record_count(tmp_path):
    p = str(tmp_path / "a.edf")
    a, _, _ = _mixed_edf(p, announce=-1)
    out = rec.read_edf(p)
    assert out["header"]["n_records"] == 7 and np.array_equal(out["signals"]["EEG Fpz-Cz"]["data"], a)


def test_edf_refusals(tmp_path):
    p = str(tmp_path / "a.edf")
    _mixed_edf(p)
    with pytest.raises(ValueError, match=r"no channel \['EEG C3'\]; the file has \['EEG Fpz-Cz', 'EEG Pz-Oz', 'Event marker'\]"):
        rec.read_edf(p, channels=["EEG C3"])
    q = str(tmp_path / "d.edf")
    _mixed_edf(q, reserved="EDF+D")
    with pytest.raises(ValueError, match=r"EDF\+D \(discontinuous recording\) is not supported"):
        rec.read_edf(q)
    _mixed_edf(q, reserved="EDF+C")
    assert rec.read_edf(q)["header"]["reserved"] == "EDF+C"
    raw = open(p, "rb").read()
    t = str(tmp_path / "t.edf")
    open(t, "wb").write(raw[:-10])
    with pytest.raises(ValueError, match="truncated: 7 records of 502 bytes announced"):
        rec.read_edf(t)
    open(t, "wb").write(raw[:100])
    with pytest.raises(ValueError, match="truncated: 100 bytes"):
        rec.read_edf(t)
    _mixed_edf(t, announce=-1)
    unknown = open(t, "rb").read()
    open(t, "wb").write(unknown[:-10])
    with pytest.raises(ValueError, match="no whole number of 502-byte records"):
        rec.read_edf(t)
    z = R.write_edf(str(tmp_path / "z.edf"), [R.eeg_signal("EEG", np.zeros(10, np.int16), 10, dmin=5, dmax=5)])
    with pytest.raises(ValueError, match="digital_max == digital_min == 5"):
        rec.read_edf(z)


# ---------------------------------------------------------------------------------------------------- stages
ANNOTS = [(0, 90, "Sleep stage W"), (90, 30, "Sleep stage 1"), (120, 60, "Sleep stage 2"), (180, 30, "Sleep stage 3"), (210, 30, "Sleep stage 4"),
          (240, 30, "Sleep stage R"), (270, 30, "Movement time"), (300, 30, "Sleep stage ?"), (330, 30, "Sleep stage 2")]


def test_annotations_round_trip_and_mapping(tmp_path):
    p = R.write_edf_annotations(str(tmp_path / "h.edf"), ANNOTS + [(45.5, None, "Lights off")])
    got = rec.read_edf_annotations(p)
    assert [(a, t) for a, _, t in got if t != "Lights off"] == [(float(a), t) for a, _, t in ANNOTS]
    assert [d for _, d, t in got if t != "Lights off"] == [float(d) for _, d, _ in ANNOTS]
    assert (45.5, 0.0, "Lights off") in got
    st = rec.stages_from_annotations(got, 14)
    assert st.dtype == np.int32 and st.tolist() == [0, 0, 0, 1, 2, 2, 3, 3, 4, -1, -1, 2, -1, -1]
    assert rec.stages_from_annotations(got, 5).tolist() == [0, 0, 0, 1, 2]
    with pytest.raises(ValueError, match="starts at 100 s, no multiple of the 30-s epoch"):
        rec.stages_from_annotations([(100, 30, "Sleep stage 2")], 10)
    assert rec.stages_from_annotations([(90, 70, "Sleep stage 2"), (180, 20, "Sleep stage R")], 8).tolist() == [-1, -1, -1, 2, 2, -1, -1, -1]      # ragged durations: whole epochs only
    with pytest.raises(ValueError, match="no 'EDF Annotations' signal"):
        rec.read_edf_annotations(R.write_edf(str(tmp_path / "n.edf"), [R.eeg_signal("EEG", np.zeros(10, np.int16), 10)]))


def test_profusion(tmp_path):
    p = R.write_profusion(str(tmp_path / "s-profusion.xml"), [0, 1, 2, 3, 4, 5, 6, 9, 0])
    codes = rec.read_profusion_stages(p)
    assert codes.tolist() == [0, 1, 2, 3, 4, 5, 6, 9, 0]
    st = rec.stages_from_profusion(codes)
    assert st.dtype == np.int32 and st.tolist() == [0, 1, 2, 3, 3, 4, -1, -1, 0]
    open(p, "w").write("<CMPStudyConfig><EpochLength>30</EpochLength></CMPStudyConfig>")
    with pytest.raises(ValueError, match="no SleepStages element"):
        rec.read_profusion_stages(p)


def test_sleep_span():
    s = np.zeros(300, np.int32)
    s[100:200] = 2
    assert rec.sleep_span(s) == (40, 260)
    assert rec.sleep_span(s, wake_mins=10) == (80, 220)
    s[:] = 0; s[5] = 1; s[290] = 4; s[295] = -1
    assert rec.sleep_span(s) == (0, 300)                       # both clamps
    assert rec.sleep_span(s, wake_mins=1) == (3, 293)
    with pytest.raises(ValueError, match="no epoch is scored as sleep"):
        rec.sleep_span(np.array([0, 0, -1, 0]))


# ---------------------------------------------------------------------------------------------------- design
@pytest.mark.parametrize("rates, ud", [((125, 100), (4, 5)), ((128, 100), (25, 32)), ((256, 100), (25, 64)), ((512, 100), (25, 128)),
                                       ((200, 100), (1, 2)), ((100, 100), (1, 1))])
def test_resample_ratio(rates, ud):
    assert rec.resample_ratio(*rates) == ud
    assert rec.resample_ratio(Fraction(rates[0]), float(rates[1])) == ud


@pytest.mark.parametrize("fin, n_taps", list(zip(RATES, N_TAPS)))
def test_design(fin, n_taps):
    u, d, t = rec.lowpass_resample_design(fin, 100)
    assert (u, d) == rec.resample_ratio(fin, 100) and t.dtype == np.float64 and t.size == n_taps
    assert np.array_equal(t, t[::-1]) or np.abs(t - t[::-1]).max() <= 1e-17
    assert abs(t.sum() - u) <= 1e-12 * u
    f, H = R.response(t, fin * u)
    H = H / u
    width = 4.5
    print(f"{fin} Hz: passband {np.abs(H[f <= 18.0] - 1).max():.2e}, stopband {H[f >= 18.0 + width].max():.2e}")
    assert np.abs(H[f <= 18.0] - 1).max() <= R.PASS_TOL
    assert H[f >= 18.0 + width].max() <= R.STOP_TOL
    if fin == 100:
        assert u == d == 1                                       # a plain 75-tap low-pass


def test_design_equals_firwin():
    signal = pytest.importorskip("scipy.signal")
    for fin in RATES:
        u, d, t = rec.lowpass_resample_design(fin, 100)
        ref = signal.firwin(t.size, 20.25, window="hamming", fs=float(fin * u))
        assert np.abs(t / u - ref).max() <= 1e-15


def test_design_refusals():
    with pytest.raises(ValueError, match="needs 32341 taps"):
        rec.lowpass_resample_design(44100, 100)
    with pytest.raises(ValueError, match="h_freq = 50 Hz is not below the Nyquist rates"):
        rec.lowpass_resample_design(125, 100, h_freq=50)
    with pytest.raises(ValueError, match="U = 100"):
        rec.lowpass_resample_design(101, 100)


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("U, D, M, L", [(1, 1, 75, 38), (4, 5, 367, 93), (4, 5, 367, 1000), (25, 32, 2347, 500), (3, 2, 31, 50), (64, 1, 33, 20),
                                         (1, 5, 11, 103), (1, 1, 1, 10)])
def test_reference_equals_its_restatement(U, D, M, L):
    r = np.random.default_rng(L)
    x = r.standard_normal((2, L)).astype(np.float32)
    h = r.standard_normal(M).astype(np.float32)
    for edge in (0, 1):
        if edge and -(-((M - 1) // 2) // U) > L - 1:
            continue
        a, b = R.resample64(x, h, U, D, edge), R.resample64_stuffed(x, h, U, D, edge)
        assert a.shape == (2, R.out_len(L, U, D)) and np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    d = r.integers(-2048, 2048, (2, L)).astype(np.int16)
    gn, of = np.array([0.1, 0.3], np.float32), np.array([1.0, -2.0], np.float32)
    a = R.resample64(d, h, U, D, 0, gn, of)
    b = R.resample64((d * gn.astype(np.float64)[:, None] + of.astype(np.float64)[:, None]), h, U, D, 0)
    assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max() + 1e-9           # b rounds the staged values to fp32 first
    E = R.resample_error_bound(x, h, U, D, 0)
    assert E.shape == a.shape and (E > 0).all()


def test_reference_support_mask():
    m = R.resample_support_mask(50, 11, 1, 1, 20, 0)
    assert np.nonzero(m)[0].tolist() == list(range(15, 26))
    m = R.resample_support_mask(50, 11, 1, 1, 2, 1)
    assert np.nonzero(m)[0].tolist() == list(range(0, 8))
    m = R.resample_support_mask(40, 9, 2, 1, 10, 0)               # c = 4: outputs 2 j + [-4, 4] of sample j, on the phases that hold a tap
    assert np.nonzero(m)[0].tolist() == list(range(16, 25))


@pytest.mark.parametrize("fin", RATES)
def test_reference_keeps_10_hz_and_removes_40_hz(fin):
    u, d, t = rec.lowpass_resample_design(fin, 100)
    n = np.arange(20 * fin)
    keep = slice(200, 1800)
    tt = np.arange(2000) / 100.0
    y = R.resample64(np.sin(2 * np.pi * 10.0 * n / fin).astype(np.float32)[None], t, u, d, 1)[0]
    assert y.size == 2000
    err = np.abs(y[keep] - np.sin(2 * np.pi * 10.0 * tt[keep])).max()
    z = R.resample64(np.sin(2 * np.pi * 40.0 * n / fin).astype(np.float32)[None], t, u, d, 1)[0]
    print(f"{fin} Hz: 10 Hz error {err:.2e}, 40 Hz residue {np.abs(z[keep]).max():.2e}")
    assert np.abs(z[keep]).max() <= R.STOP_TOL
    assert err <= R.PASS_TOL


# ---------------------------------------------------------------------------------------------------- refusals without a device
def test_python_refusals_without_a_device():
    x = np.zeros((2, 100), np.float32)
    t = np.ones(5) / 5
    bad = [(dict(taps=np.ones(4)), "odd number of taps"), (dict(taps=np.ones(0)), "odd number of taps"), (dict(taps=np.ones(16385)), "odd number of taps"),
           (dict(taps=[1.0, np.inf, 1.0]), "non-finite taps"), (dict(U=0), "U must be an integer in 1..64"), (dict(U=65), "U must be"),
           (dict(U=1.5), "U must be"), (dict(D=0), "D must be an integer in 1..4096"), (dict(D=4097), "D must be"), (dict(edge="wrap"), "edge must be one of"),
           (dict(gain=1.0, offset=0.0), "gain / offset belong to int16 rows"), (dict(x=np.zeros((2, 0), np.float32)), "rows of 1..2\\^30 samples"),
           (dict(x=np.zeros((2, 3, 4), np.float32)), "rows \\(B, L\\) expected"), (dict(x=np.zeros((2, 10), np.int32)), "floating point or int16"),
           (dict(x=np.zeros((2, 10), np.int16)), "int16 rows need gain and offset"), (dict(x=np.zeros((2, 10), np.int16), gain=[1.0, 2.0, 3.0], offset=0.0), "one value per row"),
           (dict(x=np.zeros((2, 10), np.int16), gain=np.nan, offset=0.0), "non-finite"),
           (dict(x=np.zeros((2, 3), np.float32), taps=np.ones(9), U=1), "reflect needs ceil")]
    for kw, msg in bad:
        a = dict(x=x, taps=t, U=4, D=5, edge="reflect")
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            rec.resample_fir(**a)
    for kw, msg in [(dict(epoch_len=0), "epoch_len must be"), (dict(epoch_len=12289), "epoch_len must be"), (dict(epoch_len=2.5), "epoch_len must be"),
                    (dict(x=np.zeros((2, 10), np.int16)), "floating point"), (dict(x=np.zeros((2, 3, 4), np.float32)), "rows")]:
        a = dict(x=x, epoch_len=10)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            rec.epoch_stats(**a)


def test_prepare_recording_refusals_without_a_device(tmp_path):
    r = np.random.default_rng(0)
    psg = R.write_edf(str(tmp_path / "SC4001E0-PSG.edf"), [R.eeg_signal("EEG Fpz-Cz", r.integers(-99, 99, 10 * 125).astype(np.int16), 125)])
    hyp = R.write_edf_annotations(str(tmp_path / "SC4001EC-Hypnogram.edf"), ANNOTS, starttime="23.00.00")
    with pytest.raises(ValueError, match="not the same recording"):
        rec.prepare_recording(psg, hyp, ["EEG Fpz-Cz"])
    with pytest.raises(ValueError, match="units must be"):
        rec.prepare_recording(psg, hyp, ["EEG Fpz-Cz"], units="mV")
    with pytest.raises(ValueError, match="no channel"):
        rec.prepare_recording(psg, hyp, ["EEG Cz"])


def test_entry_helpers():
    from eegldm.entry import prepare_recordings as P
    assert P.subject_night("SC4012E0-PSG") == ("01", "2") and P.subject_night("shhs1-200077") == ("200077", "1") and P.subject_night("night7") == ("", "")
    assert rec.channel_file_name("EEG Fpz-Cz") == "Fpz-Cz" and rec.channel_file_name("EEG(sec)") == "EEG_sec_"
    rows = [{"subject": f"{s:02d}", "recording": f"SC4{s:02d}{n}E0-PSG", "night": str(n)} for s in range(10) for n in (1, 2)]
    parts = P.split_subjects(rows, [0.6, 0.2, 0.2], seed=1)
    sets = [{r["subject"] for r in parts[k]} for k in ("train", "valid", "test")]
    assert [len(s) for s in sets] == [6, 2, 2] and not (sets[0] & sets[1]) and not (sets[0] & sets[2]) and not (sets[1] & sets[2])
    assert sum(len(parts[k]) for k in parts) == 20
    assert parts == P.split_subjects(rows, [0.6, 0.2, 0.2], seed=1)


def test_header_declares_the_two_exports():
    src = open(os.path.join(ROOT, "include", "eegldm.h")).read()
    assert re.search(r"int eegldm_resample_fir\(eegldm_ctx\*, const void\* x, long ldx, int xtype /\* 0 fp32, 1 int16 \*/, const float\* gain, "
                     r"const float\* offset,\s+const float\* taps, int M, int U, int D, float\* y, long ldy, long B, long L, int edge", src)
    assert re.search(r"int eegldm_epoch_stats\(eegldm_ctx\*, const float\* x, long ldx, long B, long L, int E, float\* out\);", src)
    from eegldm._lib import SIGNATURES, lib
    for name, n in (("eegldm_resample_fir", 15), ("eegldm_epoch_stats", 7)):
        assert len(SIGNATURES[name]) == n and hasattr(lib, name)
