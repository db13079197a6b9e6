"""CPU: the numpy restatement of batch (Lloyd) k-means (tests/_lloyd_np.py) against what it restates -- the float64 per-cluster
mean, scipy's vq + mean -- and its fixed-point scale and empty-cluster rule at their edges.  No device, and no code of the
package: the loop's labels come from the CPU oracle."""
import numpy as np
import pytest

from tests import _lloyd_np as L


def _mixture(seed, n, d, k, scale=1.0):
    rs = np.random.RandomState(seed)
    cen = rs.randn(k, d).astype(np.float32) * 3
    return ((cen[rs.randint(0, k, n)] + rs.randn(n, d)) * scale).astype(np.float32)


def _ulp32(v):
    """the spacing of fp32 at |v| (float64 array)"""
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _check_update(x, labels, k):
    n = len(x)
    absmax = float(np.abs(x).max())
    s = L.shift_of(absmax, n)
    centers, sizes, splits = L.update(x, labels, k, s)
    assert splits == 0 and np.array_equal(sizes, np.bincount(labels, minlength=k))
    mean = np.stack([x[labels == c].astype(np.float64).mean(0) for c in range(k)])
    # the fixed-point rounding: every q is off by at most 1/2 in units of 2^-s, so is their mean; the int64 -> float64 conversion
    # of a sum and the two float64 operations after it add three roundings of 2^-53 relative, the float64 mean it is compared with
    # (numpy's pairwise sum of at most 3 000 terms, one division) fewer than thirteen more
    fixed = 0.5 * 2.0 ** -s + 16 * 2.0 ** -53 * np.abs(mean)
    assert 0.5 * 2.0 ** -s <= absmax * 2.0 ** -40, (s, n)  # what the scale promises for N <= 2^21 rows
    err = np.abs(centers.astype(np.float64) - mean)
    bound = 0.5 * _ulp32(np.abs(mean) + fixed) + fixed  # (the ulp of the binade the unrounded centre can lie in)
    print("worst error / bound", float((err / bound).max()), "s", s)
    assert (err <= bound).all()
    return centers, mean


@pytest.mark.parametrize("scale", [1.0, 1e-20, 1e20])
def test_update_is_the_float64_mean(scale):
    x = _mixture(0, 3000, 24, 7, scale)
    labels = np.random.RandomState(1).randint(0, 7, len(x))
    _check_update(x, labels, 7)


def test_update_against_scipy_vq():
    vq = pytest.importorskip("scipy.cluster.vq")
    x = _mixture(2, 2000, 16, 5)
    book = x[:5].astype(np.float64)
    labels, _ = vq.vq(x.astype(np.float64), book)
    assert len(np.unique(labels)) == 5
    _check_update(x, labels.astype(np.int64), 5)


@pytest.mark.parametrize("n", [2, 3, 2 ** 27])
@pytest.mark.parametrize("absmax", [1e-30, 1.0, 0.5, np.nextafter(np.float32(1), np.float32(0)), 1e30, np.finfo(np.float32).max])
def test_scale_never_overflows(n, absmax):
    absmax = float(np.float32(absmax))
    s = L.shift_of(absmax, n)
    q = int(L.quantise(np.array([absmax], np.float32), s)[0])  # the largest term there can be
    assert q * n < 2 ** 62 + n  # |x 2^s| < 2^62 / n before rounding: n terms stay below 2^62 (+ n halves of rounding)
    assert q * n < 2 ** 63 - 1 and -q * n > -2 ** 63
    assert q * 2 * n >= 2 ** 59  # and no bit more head-room than a factor 8: the scale is not wasted
    assert -1000 <= s <= 1000


def test_scale_formula():
    assert L.shift_of(1.0, 2) == 62 - 1 - 1       # frexp(1.0) = (0.5, 1)
    assert L.shift_of(0.75, 1024) == 62 - 10 - 0
    assert L.shift_of(0.75, 1025) == 62 - 11 - 0
    assert L.shift_of(3.0, 1) == 62 - 1 - 2       # max(N, 2)


def test_quantise_rounds_half_to_even():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.25, 0.75], np.float32)
    assert L.quantise(x, 0).tolist() == [0, 2, 2, 0, -2, 0, 1]
    assert L.quantise(x, 1).tolist() == [1, 3, 5, -1, -3, 0, 2]


def test_two_empty_clusters_and_a_tie():
    d = 5
    centers = np.arange(6 * d, dtype=np.float32).reshape(6, d) + 1
    counts = np.array([7, 0, 9, 0, 9, 2], np.int64)
    c0 = centers.copy()
    assert L.split_empty(centers, counts) == 2
    up, down = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    even = np.arange(d) % 2 == 0
    # empty 1: the largest is 9, clusters 2 and 4 tie -> 2.  It keeps 5, cluster 1 gets 4.
    want1 = np.where(even, c0[2] * up, c0[2] * down)
    two = np.where(even, c0[2] * down, c0[2] * up)
    # empty 3: the largest is now cluster 4 (9).  It keeps 5, cluster 3 gets 4.
    want3 = np.where(even, c0[4] * up, c0[4] * down)
    four = np.where(even, c0[4] * down, c0[4] * up)
    assert counts.tolist() == [7, 4, 5, 4, 5, 2]
    for got, want in ((centers[1], want1), (centers[2], two), (centers[3], want3), (centers[4], four), (centers[0], c0[0]), (centers[5], c0[5])):
        assert got.dtype == np.float32 and got.tobytes() == want.astype(np.float32).tobytes()


def test_a_cluster_split_twice():
    centers = np.array([[1.0, 2.0], [0, 0], [0, 0], [5.0, 6.0]], np.float32)
    counts = np.array([100, 0, 0, 3], np.int64)
    assert L.split_empty(centers, counts) == 2
    assert counts.tolist() == [25, 50, 25, 3]  # 100 -> 50 + 50; then the tie 0 / 1 goes to 0: 50 -> 25 + 25
    up, down = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    assert centers[1].tobytes() == (np.array([1.0, 2.0], np.float32) * np.array([up, down])).astype(np.float32).tobytes()
    assert centers[2].tobytes() == (np.array([1.0, 2.0], np.float32) * np.array([down, up]) * np.array([up, down])).astype(np.float32).tobytes()


def test_loop_inertia_falls():
    x = _mixture(3, 640, 8, 4)
    steps = L.loop(x, x[:4], 12)
    inertia = [float(((x.astype(np.float64) - st["centers"][st["labels"]].astype(np.float64)) ** 2).sum()) for st in steps]
    print(inertia, [st["changed"] for st in steps])
    assert steps[0]["changed"] == len(x)
    assert steps[-1]["changed"] == 0 or len(steps) == 12
    # the mean minimises a cluster's inertia and the nearest centre a row's.  What may rise: a row's label is the argmin of
    # fp32 distances, each within (d + 2) 2^-23 (|x|^2 + |c|^2) of the exact one, so a row may sit at a centre that much farther
    # than its nearest (twice: both distances are rounded); the fp32 rounding of a centre moves a cluster's inertia in second order
    d = x.shape[1]
    big = float((x.astype(np.float64) ** 2).sum(1).max() + max((st["centers"].astype(np.float64) ** 2).sum(1).max() for st in steps))
    allow = len(x) * 2 * (d + 2) * 2.0 ** -23 * big
    for a, b in zip(inertia, inertia[1:]):
        assert b <= a + allow
