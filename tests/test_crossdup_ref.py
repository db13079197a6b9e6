"""CPU: the numpy restatement of acav_rows_crossdup (tests/_crossdup_np.py) against the three-line brute force on tiny inputs:
random rows, ties between two equal held-out rows, zero rows on either side, a label without a held-out row, and no blocking
== blocking with every label 0."""
import numpy as np
import pytest

from tests import _crossdup_np as R


def _agree(x, y, lx, ly):
    best, partner, _second = R.nearest_in(x, y, lx, ly)
    b, p = R.brute_force(x, y, lx, ly)
    assert np.array_equal(partner, p)
    assert np.array_equal(np.isneginf(best), p < 0)
    has = p >= 0
    assert np.abs(best[has] - b[has]).max() <= 4 * R.bound(x.shape[1])  # a BLAS product against a python dot
    return best, partner


@pytest.mark.parametrize("n,m,d,k", [(40, 17, 5, 3), (25, 30, 1, 2), (60, 9, 33, 4)])
def test_restatement_equals_brute_force(n, m, d, k):
    rs = np.random.RandomState(n + m + d)
    x, y = rs.randn(n, d).astype(np.float32), rs.randn(m, d).astype(np.float32)
    _agree(x, y, rs.randint(0, k, n), rs.randint(0, k, m))


def test_ties_zero_rows_and_a_label_without_held_out_rows():
    rs = np.random.RandomState(4)
    x, y = rs.randn(12, 6).astype(np.float32), rs.randn(10, 6).astype(np.float32)
    lx = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 0])
    ly = np.array([0, 0, 0, 0, 1, 1, 1, 3, 3, 3])  # label 2 has no held-out row
    y[3] = y[1]          # two equal held-out rows of label 0 ...
    x[0] = y[3]          # ... and a pool copy of them: the lower one, 1, is its partner
    x[2] = y[1]          # two pool rows copying one held-out row
    x[1] = 0.0           # a zero pool row
    y[5] = 0.0           # a zero held-out row of label 1 ...
    x[4] = 0.0           # ... and a zero pool row of label 1
    y[7:] = 0.0          # every held-out row of label 3 is zero
    best, partner = _agree(x, y, lx, ly)
    assert partner[0] == 1 and partner[2] == 1 and abs(best[0] - 1) <= R.bound(6) and best[0] == best[2]
    assert partner[1] == -1 and partner[4] == -1
    assert (partner[6:9] == -1).all() and (partner[9:11] == -1).all()
    assert not np.isin(partner, [5, 7, 8, 9]).any()
    assert set(partner[[3, 5]]) <= {4, 6}
    second = R.nearest_in(x, y, lx, ly)[2]
    assert second[0] < 1 - 1e-3  # the partner's copy is no rival


def test_unblocked_is_blocked_with_every_label_zero():
    rs = np.random.RandomState(8)
    x, y = rs.randn(30, 7).astype(np.float32), rs.randn(11, 7).astype(np.float32)
    y[4] = 0.0
    a = R.nearest_in(x, y)
    b = R.nearest_in(x, y, np.zeros(30, np.int64), np.zeros(11, np.int64))
    for u, w in zip(a, b):
        assert np.array_equal(u, w)
    assert np.array_equal(a[1], R.brute_force(x, y, np.zeros(30), np.zeros(11))[1]) and not (a[1] == 4).any()
