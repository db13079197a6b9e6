"""CPU: the float64 restatement of clustering.whiten (tests/_whiten_np.py) against scipy, and the host-side merge of
per-segment moments (whiten.ColumnMoments.merge) against the direct float64 std."""
import numpy as np
import pytest

from tests import _whiten_np as R

SHAPES = [(1, 5), (2, 3), (257, 88), (5000, 352), (70001, 64)]


@pytest.mark.parametrize("n,d", SHAPES, ids=["{}x{}".format(*s) for s in SHAPES])
def test_restatement_is_scipy_whiten_in_float64(n, d):
    """<= 3 ulp: the std's rounding to fp32 (2^-24), the fp32 division (2^-24) and the rounding of scipy's float64 result to
    fp32 (2^-24), against an ulp of at least 2^-24 relative"""
    vq = pytest.importorskip("scipy.cluster.vq")
    import warnings
    x = R.recipe(n, d, seed=n + d)
    got, std, nz = R.whiten(x)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scipy warns about the zero-variance columns it leaves alone
        want = vq.whiten(x.astype(np.float64)).astype(np.float32)
    assert got.dtype == np.float32 and nz >= 1 and std[0] == 1.0
    worst = int(R.ulp_diff(got, want).max())
    print("max ulp", worst)
    assert worst <= 3


def _segmentations(n, rs, count):
    yield [0, n]
    yield [0, 0, n, n]
    for _ in range(count):
        k = int(rs.randint(1, 9))
        cuts = np.sort(rs.randint(0, n + 1, k)).tolist()
        if rs.rand() < 0.5 and n > 1:
            cuts.append(cuts[-1] + 1 if cuts[-1] < n else cuts[-1])  # a one-row segment
            cuts.sort()
        yield [0] + cuts + [n]


@pytest.mark.parametrize("n,d", [(1, 5), (2, 3), (257, 88), (5000, 352), (70001, 16)], ids=lambda v: str(v))
def test_merge_of_ragged_segments_is_the_direct_std(n, d):
    """segments (empty and one-row ones among them) -> tile/Chan moments -> ColumnMoments.merge in order == the float64 std of all
    rows, to 0 ulp in fp32"""
    from acav100m_amd.clustering.whiten import ColumnMoments
    x = R.recipe(n, d, seed=3 * n + d)
    want, want_zero = R.std_of(x)
    rs = np.random.RandomState(n)
    for prefix in _segmentations(n, rs, 20 if n < 10000 else 4):
        cm = ColumnMoments(d)
        for a, b in zip(prefix[:-1], prefix[1:]):
            cm.add_segment(*R.segment_moments(x[a:b]))
        assert cm.n == n
        assert int(R.ulp_diff(cm.std(), want).max()) == 0, prefix
        assert cm.zero_columns == want_zero


def test_merge_is_pure_and_keeps_an_empty_side():
    from acav100m_amd.clustering.whiten import ColumnMoments
    a = (3, np.array([1.0, 2.0]), np.array([0.5, 0.0]))
    e = (0, np.zeros(2), np.zeros(2))
    for got in (ColumnMoments.merge(a, e), ColumnMoments.merge(e, a)):
        assert got[0] == 3 and np.array_equal(got[1], a[1]) and np.array_equal(got[2], a[2])
    b = (1, np.array([5.0, 2.0]), np.zeros(2))
    n, mean, m2 = ColumnMoments.merge(a, b)
    assert n == 4 and np.array_equal(mean, [2.0, 2.0]) and np.array_equal(m2, [0.5 + 16 * 0.75, 0.0])
    assert np.array_equal(a[1], [1.0, 2.0]) and np.array_equal(a[2], [0.5, 0.0])  # the inputs are left alone


def test_constant_column_has_std_exactly_zero():
    """0.1f is no dyadic fraction: a mean taken as sum x (1 / n) would leave rounding noise to divide by"""
    from acav100m_amd.clustering.whiten import ColumnMoments
    x = np.full((1000, 1), np.float32(0.1))
    cm = ColumnMoments(1)
    for a, b in ((0, 333), (333, 334), (334, 1000)):
        seg = R.segment_moments(x[a:b])
        assert seg[2][0] == 0.0
        cm.add_segment(*seg)
    assert cm.n == 1000 and cm.M2[0] == 0.0 and cm.zero_columns == 1
    assert cm.std().tolist() == [1.0]
