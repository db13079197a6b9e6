"""CPU: the numpy restatement of the pair-counting measures (tests/_pair_measures.py) against the goldens recorded from the
reference's own classes (tests/golden/gen_golden_pair.py), and of the ami / nmi average methods.  No GPU."""
import os

import numpy as np
import pytest

from tests import _pair_measures as PM

CASES = ["a", "b", "c", "d", "e"]

# Free-running departures from the reference: at these iterations the restatement's best candidates tie EXACTLY (equal Rand
# indices), and the reference's fp32 pair mean split the tie by one or two fp32 ulps (its recorded margin), so the first
# maximum differs.  Named here, checked to be such a tie below; every other free run equals the reference pick for pick.
RAND_FP32_NEAR_TIES = {"b": 37, "c": 19, "d": 22, "e": 27}


def _load(golden_dir, case, measure):
    return np.load(os.path.join(golden_dir, f"pair_{case}_{measure}.npz"))


def test_registry_names():
    from acav100m_amd.subset_selection.measures import get_measure
    from acav100m_amd.subset_selection.measures.pair import AdjustedRandScore, FowlkesMallowsScore, RandScore
    for names, cls in ((("fm", "efficient_fm"), FowlkesMallowsScore), (("rand", "efficient_rand"), RandScore),
                       (("arand", "efficient_arand", "ARAND"), AdjustedRandScore)):
        for n in names:
            assert get_measure(n) is cls


def test_unknown_average_method_is_an_error():
    from acav100m_amd.subset_selection.measures import get_measure
    a = np.zeros((4, 2), np.int64)
    for name in ("ami", "nmi"):
        with pytest.raises(ValueError, match="average_method"):
            get_measure(name)(a, average_method="geometric", ncentroids=2)
        get_measure(name)(a, average_method="MAX", ncentroids=2)  # case-insensitive, as the reference's .lower()


@pytest.mark.parametrize("measure", ["fm", "rand", "arand"])
@pytest.mark.parametrize("case", CASES)
def test_restatement_teacher_forced(golden_dir, case, measure):
    """replaying the reference's picks: S identical, every score vector within rtol 1e-5 of the reference's fp32 one
    (atol 1e-7 for ARI values near 0, where the reference's fp32 Nc - chance cancels), NaN in the same places"""
    g = _load(golden_dir, case, measure)
    r = PM.golden_pair_run(g, measure, forced=True)
    assert [int(g["start"])] + r["S"] == g["S"].tolist()
    L = len(r["scores"][0])
    for t, row in enumerate(r["scores"]):
        ref = g["scores"][t, :L - t].astype(np.float64)
        assert np.array_equal(np.isnan(row), np.isnan(ref)), f"iteration {t}: NaN positions differ"
        ok = ~np.isnan(ref)
        np.testing.assert_allclose(row[ok], ref[ok], rtol=1e-5, atol=1e-7, err_msg=f"iteration {t}")
    gain = g["GAIN"]
    assert np.array_equal(np.isnan(r["GAIN"]), np.isnan(gain))
    ok = ~np.isnan(gain)
    np.testing.assert_allclose(r["GAIN"][ok], gain[ok], rtol=1e-5, atol=1e-7)
    if measure == "arand":
        assert np.isnan(gain).any()  # every case reaches the degenerate (0/0) regime
    if measure != "arand":
        assert not np.isnan(r["GAIN"]).any()


@pytest.mark.parametrize("measure", ["fm", "rand", "arand"])
@pytest.mark.parametrize("case", CASES)
def test_restatement_free_running(golden_dir, case, measure):
    g = _load(golden_dir, case, measure)
    r = PM.golden_pair_run(g, measure, forced=False)
    ours, ref = r["S"], g["S"].tolist()[1:]
    first = next((t for t, (x, y) in enumerate(zip(ours, ref)) if x != y), None)
    expected = RAND_FP32_NEAR_TIES.get(case) if measure == "rand" else None
    assert first == expected, f"free run departs from the reference at iteration {first} (expected {expected})"
    if first is None:
        assert len(ours) == len(ref)
        return
    # a genuine fp32 near-tie: the reference's best and second-best were 1-2 fp32 ulps apart, and the two candidates
    # tie exactly in the canonical form
    t = first
    assert 0 < g["margin"][t] <= 2.0 ** -22
    f = PM.golden_pair_run(g, measure, forced=True)
    row = f["scores"][t]
    assert row[int(g["idx"][t])] == row[f["argmax"][t]]


def test_residue_regime_is_exercised(golden_dir):
    """case a (C = 40, one pair, start clip 5): the first FM gain is 1/C, a ratio of residues only (TP = eps,
    FP = FN = (C - 1) eps); from the third pick on, every candidate in a fresh row and column scores exactly 1.0 (integer TP,
    residue-only FP / FN) and the residue rule decides which candidates tie there"""
    g = _load(golden_dir, "a", "fm")
    assert int(g["start"]) == 5 and int(g["C"]) == 40
    assert g["GAIN"][0] == np.float32(1 / 40) and np.all(g["GAIN"][1:10] == 1.0)
    r = PM.golden_pair_run(g, "fm", forced=True)
    assert r["GAIN"][0] == 1 / 40
    top = r["scores"][2] == 1.0
    assert 100 < top.sum() < len(top)
    assert np.array_equal(top, g["scores"][2, :len(top)] == 1.0)


def test_pair_stats_identity_and_sklearn():
    """TP + FP + FN + TN = n (n - 1) / 2 exactly, and the counts are sklearn's pair_confusion_matrix / 2"""
    from sklearn.metrics.cluster import pair_confusion_matrix
    rs = np.random.RandomState(3)
    a = rs.randint(0, 7, size=(90, 3))
    pairs = [(0, 1), (0, 2), (1, 2)]
    m = PM.PairGreedy(a, pairs, 7)
    m.add_samples(range(60))
    st = m.pair_stats()
    assert np.array_equal(st["TP"] + st["FP"] + st["FN"] + st["TN"], np.full(3, 60 * 59 // 2))
    for p, (d0, d1) in enumerate(pairs):
        pcm = pair_confusion_matrix(a[:60, d0], a[:60, d1]) // 2
        assert [[st["TN"][p], st["FP"][p]], [st["FN"][p], st["TP"][p]]] == pcm.tolist()


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("method", ["max", "min", "arithmetic"])
@pytest.mark.parametrize("measure", ["ami", "nmi"])
def test_average_method_goldens(golden_dir, measure, method, case):
    """subset_selection's EfficientAMI / EfficientNMI with average_method max / min (and the default): the float64
    restatement over integer counts is within 1e-5 of the reference's fp32 scores on every iteration"""
    g = np.load(os.path.join(golden_dir, f"mi_avg_{measure}_{method}_{case}.npz"))
    rows = PM.golden_avg_run(g, measure, method)
    for t, row in enumerate(rows):
        np.testing.assert_allclose(row, g["scores"][t, :len(row)], rtol=1e-5, atol=1e-7, err_msg=f"iteration {t}")
