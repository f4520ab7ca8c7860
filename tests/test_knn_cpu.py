"""CPU: everything of the nearest-neighbour metrics that needs no device -- the refusals, the lag / crop arithmetic, the quantile and flag
logic, the precision / recall / coverage composition, the lag merge and the ctypes table."""
import numpy as np
import pytest
import torch

import knn_reference as R


def test_refusals_come_before_the_device():
    from eegldm import metrics as M
    q, x = torch.zeros(4, 8), torch.zeros(6, 8)
    for k in (0, 33, -1, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            M.NearestNeighbours(q, k)
        with pytest.raises(ValueError, match="k must be"):
            M.knn(q, x, k)
        with pytest.raises(ValueError, match="k must be"):
            M.precision_recall_coverage(x, x, k=k)
    with pytest.raises(ValueError, match="feature dimensions differ"):
        M.knn(q, torch.zeros(6, 7), 1)
    with pytest.raises(ValueError, match="feature dimensions differ"):
        M.precision_recall_coverage(x, torch.zeros(6, 7), k=3)
    with pytest.raises(ValueError, match="empty queries"):
        M.NearestNeighbours(torch.zeros(0, 8), 1)
    with pytest.raises(ValueError, match="empty queries"):
        M.knn(torch.zeros(0, 8), x, 1)
    for bad in (torch.zeros(8), torch.zeros(2, 3, 8)):
        with pytest.raises(ValueError, match="2-D"):
            M.NearestNeighbours(bad, 1)
        with pytest.raises(ValueError, match="2-D"):
            M.knn(q, bad, 1)
        with pytest.raises(ValueError, match="2-D"):
            M.kth_radius(bad)
    with pytest.raises(ValueError, match="exclude_self"):
        M.knn(q, x, 1, exclude_self=True)
    with pytest.raises(ValueError, match="metric"):
        M.NearestNeighbours(q, 1, metric="cosine")
    with pytest.raises(ValueError, match="more than 3 rows"):
        M.kth_radius(torch.zeros(3, 8), k=3)
    w = torch.zeros(5, 100)
    with pytest.raises(ValueError, match="leaves no samples"):
        M.memorisation_audit(w, [w], w, lags=(-50, 0, 50))
    with pytest.raises(ValueError, match="empty queries"):
        M.memorisation_audit(torch.zeros(0, 100), [w], w)
    with pytest.raises(ValueError, match="feature dimensions differ"):
        M.memorisation_audit(w, [w], torch.zeros(5, 90))
    with pytest.raises(ValueError, match="windows"):
        M.memorisation_audit(torch.zeros(5, 2, 100), [w], w)
    with pytest.raises(ValueError, match="space"):
        M.memorisation_audit(w, [w], w, space="latent")
    with pytest.raises(ValueError, match="usleep"):
        M.memorisation_audit(w, [w], w, space="features")
    with pytest.raises(ValueError, match="k must be"):
        M.memorisation_audit(w, [w], w, k=40)


def test_lag_crops():
    from eegldm.metrics import lag_crops
    assert lag_crops(3000, (0,)) == (0, (0, 3000), {0: (0, 3000)})
    g, corpus, q = lag_crops(3000, (-5, 0, 5))
    assert g == 5 and corpus == (5, 2995) and q == {-5: (0, 2990), 0: (5, 2995), 5: (10, 3000)}
    assert all(hi - lo == corpus[1] - corpus[0] and lo >= 0 and hi <= 3000 for lo, hi in q.values())
    # a window that is a training window moved 5 samples early matches at lag -5, sample for sample
    train = np.arange(3000.0)
    early = np.concatenate([train[5:], np.zeros(5)])
    assert np.array_equal(early[q[-5][0]:q[-5][1]], train[corpus[0]:corpus[1]])
    late = np.concatenate([np.zeros(5), train[:-5]])
    assert np.array_equal(late[q[5][0]:q[5][1]], train[corpus[0]:corpus[1]])
    assert lag_crops(11, (5,)) == (5, (5, 6), {5: (10, 11)})
    for bad in ((6,), (-6, 0)):
        with pytest.raises(ValueError, match="leaves no samples"):
            lag_crops(12, bad)
    with pytest.raises(ValueError):
        lag_crops(12, ())


def test_quantile_and_flags():
    from eegldm.metrics import audit_summary
    hold = np.arange(1.0, 102.0)[:, None]                   # 1 .. 101: the q quantile is 1 + 100 q
    syn_d = np.array([[0.0], [1.99], [2.0], [50.0], [200.0]])
    syn_i = np.array([[7], [8], [9], [10], [11]])
    a = audit_summary(syn_d, syn_i, hold, quantile=0.01)
    assert a["threshold"] == pytest.approx(2.0) and a["flagged"] == [0, 1]              # strictly below the threshold
    assert a["holdout_quantiles"]["0.0"] == 1.0 and a["holdout_quantiles"]["0.5"] == 51.0 and a["holdout_quantiles"]["1.0"] == 101.0
    assert a["holdout_rank"] == [0.0, pytest.approx(1 / 101), pytest.approx(1 / 101), pytest.approx(49 / 101), 1.0]
    assert a["nearest_index"] == syn_i.tolist() and a["n_synthetic"] == 5 and a["n_holdout"] == 101
    assert audit_summary(syn_d, syn_i, hold, quantile=0.5)["flagged"] == [0, 1, 2, 3]
    assert audit_summary(syn_d, syn_i, hold, quantile=0.0)["flagged"] == [0]
    with pytest.raises(ValueError):
        audit_summary(syn_d, syn_i, hold, quantile=1.5)
    with pytest.raises(ValueError):
        audit_summary(syn_d, syn_i, np.zeros((0, 1)))


def test_precision_recall_coverage_composition():
    from eegldm.metrics import prc_from_tables
    out = prc_from_tables(fake_margin=[-1.0, 0.0, 0.5, 2.0], real_margin=[-0.1, 3.0, 4.0], real_nn_d2=[1.0, 2.0, 9.0], real_r2=[1.0, 1.5, 10.0])
    assert out == {"precision": 0.5, "recall": pytest.approx(1 / 3), "coverage": pytest.approx(2 / 3), "n_real": 3, "n_fake": 4}
    # the float64 reference composes the same tables
    rng = np.random.default_rng(0)
    real, fake = rng.standard_normal((40, 6)), rng.standard_normal((30, 6)) + 0.5
    want, m = R.prc64(real, fake, 3)
    r2 = R.kth_radius2_64(real, 3)
    got = prc_from_tables(m["precision"], m["recall"], R.sqdist64(real, fake).min(1), r2)
    assert all(got[n] == pytest.approx(want[n]) for n in want)
    with pytest.raises(ValueError):
        prc_from_tables([], [1.0], [1.0], [1.0])


def test_merge_over_lags():
    from eegldm.metrics import merge_lag_tables
    d = [np.array([[0.5, 0.9]], np.float32), np.array([[0.1, 0.5]], np.float32), np.array([[np.inf, np.inf]], np.float32)]
    i = [np.array([[4, 9]]), np.array([[9, 2]]), np.array([[-1, -1]])]
    md, mi = merge_lag_tables(d, i, 3)
    assert mi.tolist() == [[9, 2, 4]] and md.tolist() == [[np.float32(0.1), 0.5, 0.5]]       # index 9 keeps its smaller distance; ties by index
    md, mi = merge_lag_tables(d, i, 4)
    assert mi.tolist() == [[9, 2, 4, -1]] and np.isinf(md[0, 3])


def test_reference_bounds():
    assert R.c_of(1) == pytest.approx(3.0, rel=1e-6) and R.c_of(3000) == pytest.approx(3002 * (1 + 3002 * R.U), rel=1e-6)
    s, i = R.topk64(np.array([[3.0, 1.0, np.nan, 1.0]]), 3, index_base=10)
    assert s.tolist() == [[1.0, 1.0, 3.0]] and i.tolist() == [[11, 13, 10]]
    s, i = R.topk64(np.array([[3.0, 1.0], [0.0, 5.0]]), 2, self_base=0)
    assert i.tolist() == [[1, -1], [0, -1]] and np.isinf(s[:, 1]).all()


def test_ctypes_rows_exist():
    from eegldm._lib import SIGNATURES, lib
    for name, nargs in (("eegldm_knn_update", 14), ("eegldm_rows_sqnorm", 6), ("eegldm_rows_standardize", 7), ("eegldm_knn_rescore", 12)):
        assert len(SIGNATURES[name]) == nargs and hasattr(lib, name)
    assert lib.eegldm_knn_update(None, None, 0, None, 0, None, 0, 0, 0, 0, 0, 0, None, None) != 0        # argument check, no device
    assert b"null argument" in lib.eegldm_last_error()
