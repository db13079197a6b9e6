"""CPU: the float64 restatement of the exact silhouette (tests/_silhouette_np.py) on hand-computable cases and against
sklearn.metrics.silhouette_samples / silhouette_score(sample_size=, random_state=) on the seeded inputs of the GPU tests; the pure
numpy half of acav100m_amd.clustering.silhouette (sample_indices, summarise).

Both sides of the sklearn comparison are references.  sklearn takes its distances in the expanded form (euclidean_distances), the
restatement in the difference form; their disagreement was measured (sklearn 1.7.2, float64 copies of the fp32 rows) and 16 x that
is asserted:

    case               max |s - sklearn|   |mean s - silhouette_score(all rows)|   |sampled mean - silhouette_score(sample)|
    absent_values      4.44e-16            0                                       0
    block_ends         7.22e-16            0                                       0
    duplicates         5e-16               1.67e-16                                5.55e-17
    tails_65x87_k33    4.44e-16            5.55e-17                                5.55e-17
    tails_65x88_k33    5e-16               1.11e-16                                5.55e-17
    two_599_1          1.5e-15             1.11e-16                                0 (one label in the sample: both refuse)
    wide_1024          1.39e-15            7.22e-16                                6.66e-16
    wide_2304          1.05e-15            5.55e-17                                1.67e-16
"""
import numpy as np
import pytest

from tests import _silhouette_np as R

MEASURED = {"samples": 1.5e-15, "score": 7.22e-16, "sampled": 6.66e-16}  # the largest of each column
SAMPLE, SEED = 48, 11


def test_two_clusters_on_a_line():
    x = np.array([[0.0], [1.0], [10.0], [12.0]], np.float32)
    ref = R.Reference(x, [0, 0, 1, 1], 2)
    assert np.array_equal(ref.A, [1.0, 1.0, 2.0, 2.0])
    assert np.array_equal(ref.B, [11.0, 10.0, 9.5, 11.5])
    assert np.allclose(ref.s, [10 / 11, 9 / 10, 7.5 / 9.5, 9.5 / 11.5], rtol=1e-15, atol=0)
    assert (ref.tA < 1e-12).all() and (ref.tB < 1e-12).all() and (ref.ts < 1e-12).all()


def test_a_singleton_cluster_scores_zero():
    x = np.array([[0.0], [1.0], [5.0]], np.float32)
    ref = R.Reference(x, [0, 0, 1], 2)
    assert ref.s[2] == 0.0 and ref.A[2] == 0.0 and ref.B[2] == 4.5 and ref.ts[2] == 0.0
    assert np.array_equal(ref.A[:2], [1.0, 1.0]) and np.array_equal(ref.B[:2], [5.0, 4.0])


def test_an_empty_label_value_is_skipped():
    x = np.array([[0.0], [1.0], [10.0], [12.0]], np.float32)
    a, b = R.Reference(x, [0, 0, 3, 3], 5), R.Reference(x, [0, 0, 1, 1], 2)
    assert np.array_equal(a.A, b.A) and np.array_equal(a.B, b.B) and np.array_equal(a.s, b.s)


def test_one_non_empty_cluster_is_undefined():
    from acav100m_amd.clustering import silhouette as S
    x = np.array([[0.0], [1.0], [3.0]], np.float32)
    ref = R.Reference(x, [2, 2, 2], 4)
    assert np.isinf(ref.B).all() and np.array_equal(ref.A, [2.0, 1.5, 2.5])
    rep = S.summarise(ref.A, ref.B, ref.s, [2, 2, 2], 4)
    assert np.isnan(rep["silhouette_sampled"]) and "fewer than two" in rep["silhouette_undefined"] and rep["silhouette_sample"] == 3
    rep = S.summarise(np.zeros(3), np.ones(3), np.zeros(3), [0, 1, 3], 4)
    assert np.isnan(rep["silhouette_sampled"]) and "one row" in rep["silhouette_undefined"]


def test_duplicate_rows():
    x = np.array([[1.0, 2.0], [1.0, 2.0], [4.0, 6.0], [1.0, 2.0]], np.float32)
    ref = R.Reference(x, [0, 0, 1, 1], 2)
    assert np.array_equal(ref.A, [0.0, 0.0, 5.0, 5.0]) and np.array_equal(ref.B, [2.5, 2.5, 5.0, 0.0])
    assert np.array_equal(ref.s, [1.0, 1.0, 0.0, -1.0])
    assert (ref.tA[:2] > 0).all()  # a duplicate comes out within sqrt(Delta) of 0, not at 0
    both = R.Reference(np.ones((4, 3), np.float32), [0, 0, 1, 1], 2)
    assert np.array_equal(both.s, np.zeros(4))  # A = B = 0


def _sklearn_deviation(name, x, lab, k):
    metrics = pytest.importorskip("sklearn.metrics")
    from acav100m_amd.clustering import silhouette as S
    ref = R.Reference(x, lab, k)
    x64 = x.astype(np.float64)
    ds = np.abs(ref.s - metrics.silhouette_samples(x64, lab)).max()
    dm = abs(ref.s.mean() - metrics.silhouette_score(x64, lab))
    idx = S.sample_indices(len(x), SAMPLE, SEED)
    sub = R.Reference(x[idx], lab[idx], k)
    if S.undefined_reason(lab[idx], k) is not None:  # sklearn refuses such a sample, summarise names the reason
        with pytest.raises(ValueError):
            metrics.silhouette_score(x64, lab, sample_size=SAMPLE, random_state=SEED)
        assert np.isnan(S.summarise(sub.A, sub.B, sub.s, lab[idx], k)["silhouette_sampled"])
        dsub = 0.0
    else:
        dsub = abs(S.summarise(sub.A, sub.B, sub.s, lab[idx], k)["silhouette_sampled"]
                   - metrics.silhouette_score(x64, lab, sample_size=SAMPLE, random_state=SEED))
    print("    {:<18} {:<19.3g} {:<39.3g} {:.3g}".format(name, ds, dm, dsub))
    return ds, dm, dsub


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_restatement_against_sklearn(name):
    x, lab, k = R.cases()[name]
    ds, dm, dsub = _sklearn_deviation(name, x, lab, k)
    assert ds <= 16 * MEASURED["samples"]
    assert dm <= 16 * MEASURED["score"]
    assert dsub <= 16 * MEASURED["sampled"]  # (this also pins sample_indices to sklearn's draw)


def test_sample_indices_are_sklearns_draw():
    from acav100m_amd.clustering import silhouette as S
    idx = S.sample_indices(1000, 64, 5)
    assert np.array_equal(idx, np.sort(np.random.RandomState(5).permutation(1000)[:64]))
    assert idx.dtype.kind == "i" and (np.diff(idx) > 0).all()
    assert np.array_equal(S.sample_indices(10, 64, 5), np.arange(10))  # M >= N: every row
    assert np.array_equal(S.sample_indices(10, 10, 0), np.arange(10))


def test_summarise_on_hand_values():
    from acav100m_amd.clustering import silhouette as S
    s = np.array([0.5, -0.25, 0.75, 0.0, -1.0])
    lab = [0, 0, 2, 2, 3]
    rep = S.summarise(np.zeros(5), np.ones(5), s, lab, 5)
    assert rep["silhouette_sampled"] == 0.0 and rep["silhouette_sample"] == 5 and rep["silhouette_negative_share"] == 0.4
    by = rep["silhouette_by_cluster"]
    assert by[0] == 0.125 and by[2] == 0.375 and by[3] == -1.0 and np.isnan(by[1]) and np.isnan(by[4]) and len(by) == 5
    assert "silhouette_undefined" not in rep
    assert sorted(rep) == ["silhouette_by_cluster", "silhouette_negative_share", "silhouette_sample", "silhouette_sampled"]
