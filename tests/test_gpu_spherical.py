"""GPU: spherical Lloyd k-means (clustering.lloyd.fit(..., normalize=True, spherical=True)) against the numpy restatement
(tests/_rownorm_np.py: spherical_loop), centres and labels bit for bit -- the plain loop, an iteration that splits an empty
cluster, an iteration whose cluster mean is the zero vector, the unit length of every centre, and normalize without spherical."""
import numpy as np
import pytest

from tests import _lloyd_np as L
from tests import _rownorm_np as R

pytestmark = pytest.mark.gpu

ITERS = 5


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _mixture(n, d, k, seed):
    rs = np.random.RandomState(seed)
    cen = rs.standard_normal((k, d))
    x = cen[rs.randint(0, k, n)] + 0.4 * rs.standard_normal((n, d))
    return (x * np.exp(rs.uniform(np.log(1e-2), np.log(1e2), (n, 1)))).astype(np.float32)  # row norms over four decades


def _picks(n, k, seed):
    """the rows fit() starts from: the first draw of the seeded generator"""
    import acav100m_amd
    from acav100m_amd.rng import default_generator
    acav100m_amd.manual_seed(seed)
    return default_generator.randperm(n)[:k]


def _fit(x, k, seed, **kw):
    """-> (the fitted KMeans, labels, report, the K initial rows' indices)"""
    import acav100m_amd
    from acav100m_amd.clustering import lloyd
    perm = _picks(len(x), k, seed)
    acav100m_amd.manual_seed(seed)
    km, labels, report = lloyd.fit(x, k, ITERS, **kw)
    return km, labels.cpu().numpy(), report, perm


def _check(km, labels, report, steps):
    assert len(report) == len(steps)
    for (changed, splits), st in zip(report, steps):
        assert (changed, splits) == (st["changed"], st["splits"])
    last = steps[-1]
    centers = km.centers.numpy()
    assert centers.tobytes() == last["centers"].tobytes()
    assert np.array_equal(km.counts.numpy(), last["sizes"].astype(np.float32))
    assert np.array_equal(labels, last["labels"])
    n2 = (centers.astype(np.float64) ** 2).sum(1)
    assert (np.abs(n2 - 1.0) <= 6e-7).all(), float(np.abs(n2 - 1).max())
    dt = km.get_attrs()
    assert dt["algorithm"] == "lloyd" and dt["spherical"] is True


@pytest.mark.parametrize("n,d,k", [(2000, 24, 7), (4099, 130, 33)])
def test_fit_is_the_restatement(torch, n, d, k):
    x = _mixture(n, d, k, seed=n)
    before = x.copy()
    km, labels, report, perm = _fit(x, k, 3, normalize=True, spherical=True)
    assert x.tobytes() == before.tobytes()
    y, zero = R.normalize(x)
    assert zero == 0
    steps = R.spherical_loop(y, y[perm], ITERS)
    print("changed:", [st["changed"] for st in steps], "splits:", [st["splits"] for st in steps])
    _check(km, labels, report, steps)
    # the same through a cuda tensor, which must stay what it is too
    t = torch.from_numpy(x).cuda()
    km2, labels2, _report, _ = _fit(t, k, 3, spherical=True)  # spherical implies normalize
    assert t.cpu().numpy().tobytes() == before.tobytes()
    assert km2.centers.numpy().tobytes() == km.centers.numpy().tobytes() and np.array_equal(labels2, labels)


def test_duplicated_initial_rows_take_the_split_path(torch):
    n, d, k, seed = 1500, 40, 6, 5
    x = _mixture(n, d, k, seed=77)
    perm = _picks(n, k, seed)
    x[perm[3]] = x[perm[1]]  # two equal initial centres: the later one gets no row (first-index argmin)
    x[perm[4]] = 4.0 * x[perm[1]]  # ... and neither does one that only differs in magnitude (a power of two: the same unit row)
    km, labels, report, perm2 = _fit(x, k, seed, normalize=True, spherical=True)
    assert np.array_equal(perm, perm2)
    y, _ = R.normalize(x)
    steps = R.spherical_loop(y, y[perm], ITERS)
    print("changed:", [st["changed"] for st in steps], "splits:", [st["splits"] for st in steps])
    assert steps[0]["splits"] >= 1
    _check(km, labels, report, steps)


def test_a_zero_mean_cluster_takes_the_empty_rule(torch):
    """rows u and -u that land in one cluster: its integer sums cancel exactly, the fp32 mean is the zero vector, the kernel counts
    the centre as a zero row, and the iteration takes the host path with that cluster emptied.  (x and -x share a nearest centre
    only on an exact tie between all centres, so the labels of this iteration are set by hand: one iteration through
    lloyd.accumulate and lloyd.finish_iteration, the two calls fit() makes.)"""
    from acav100m_amd.clustering import KMeans, lloyd
    n, d, k = 600, 19, 5
    y, _ = R.normalize(_mixture(n, d, k, seed=78))
    labels = np.random.RandomState(1).randint(0, k, n)
    labels[labels == 2] = 3
    y[40:60] = -y[20:40]
    labels[20:60] = 2  # cluster 2: twenty rows and their negatives, nothing else
    labels[labels == 4] = 0  # cluster 4: empty
    s = L.shift_of(np.abs(y).max(), n)
    want_c, want_n, want_splits = R.spherical_update(y, labels, k, s)
    assert want_splits == 2 and (want_n > 0).all()
    km = KMeans(None, d, k).to_lloyd(y[:k], spherical=True).to("cuda:0")
    t = torch.from_numpy(y).cuda()
    sums = torch.zeros((k, d), dtype=torch.int64, device="cuda")
    counts = torch.zeros(k, dtype=torch.int64, device="cuda")
    lloyd.accumulate(t, torch.from_numpy(labels).cuda(), s, sums, counts)
    assert int(counts[2]) == 40 and not bool(sums[2].any())
    splits = lloyd.finish_iteration(km, sums, counts, s, spherical=True)
    assert splits == want_splits
    assert km.centers.numpy().tobytes() == want_c.tobytes()
    assert np.array_equal(km.counts.numpy(), want_n.astype(np.float32)) and km.count == n
    n2 = (km.centers.numpy().astype(np.float64) ** 2).sum(1)
    assert (np.abs(n2 - 1.0) <= 6e-7).all()
    # only the cancelling cluster, no empty one: the device path meets the zero row and hands over to the host path
    lab2 = labels.copy()
    lab2[0] = 4
    want_c, want_n, want_splits = R.spherical_update(y, lab2, k, s)
    assert want_splits == 1
    sums.zero_(), counts.zero_()
    lloyd.accumulate(t, torch.from_numpy(lab2).cuda(), s, sums, counts)
    assert lloyd.finish_iteration(km, sums, counts, s, spherical=True) == 1
    assert km.centers.numpy().tobytes() == want_c.tobytes() and np.array_equal(km.counts.numpy(), want_n.astype(np.float32))
    # the same tables without the switch: plain means, the zero vector among them, no split
    assert lloyd.finish_iteration(km, sums, counts, s) == 0
    assert not km.centers.numpy()[2].any()


def test_normalize_without_spherical_is_plain_fit_on_normalised_rows(torch):
    import acav100m_amd
    from acav100m_amd.clustering import lloyd
    n, d, k = 2000, 24, 7
    x = _mixture(n, d, k, seed=79)
    km, labels, report, perm = _fit(x, k, 4, normalize=True)
    y, _ = R.normalize(x)
    acav100m_amd.manual_seed(4)
    km2, labels2, report2 = lloyd.fit(y, k, ITERS)
    assert km.centers.numpy().tobytes() == km2.centers.numpy().tobytes()
    assert np.array_equal(labels, labels2.cpu().numpy()) and list(report) == list(report2)
    assert "spherical" not in km.get_attrs() and km.get_attrs()["algorithm"] == "lloyd"
    steps = L.loop(y, y[perm], ITERS)
    assert km.centers.numpy().tobytes() == steps[-1]["centers"].tobytes()
    n2 = (km.centers.numpy().astype(np.float64) ** 2).sum(1)
    assert (n2 < 1.0).all()  # means of unit rows lie inside the ball
