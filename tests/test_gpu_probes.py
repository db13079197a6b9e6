"""GPU: acav_kmeans_probes (KMeans.probe_centers) against the float64 restatement of tests/_probedup_np.py: the lists identical,
the distances within the bound the header states -- after the restatement alone has shown every rank decided (the gap between
consecutive ranked distances exceeds four times their two bounds summed, no row left out).  Shapes past one row tile, one pass
of 64 centres, one 32-column stage, a d that is no multiple of 4, and more tiles than workgroups; the bytes of
KMeans.quality(rows=True); exact ties; k below m; labels that are not the nearest centre; the purity the header promises (the
rows in pieces, device and unaligned input, a second call: the same bytes); the refusals."""
import numpy as np
import pytest

from tests import _probedup_np as R

pytestmark = pytest.mark.gpu

SHAPES = [(600, 24, 7, 3), (2000, 70, 12, 4), (300, 3, 5, 2), (40000, 8, 133, 4)]  # (n, d, K, m)
_cache = {}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _state(centres):
    from acav100m_amd.clustering import KMeans
    return KMeans(None, centres.shape[1], centres.shape[0]).to_lloyd(centres).to("cuda:0")


def _case(n, d, K):
    """(rows, centres, a Lloyd state with them, calc_best's labels) -- built once and shared, never changed"""
    if (n, d, K) not in _cache:
        rs = np.random.RandomState(n + d + K)
        x = rs.randn(n, d).astype(np.float32)
        centres = (x[rs.choice(n, K, replace=False)] + 0.25 * rs.randn(K, d)).astype(np.float32)
        km = _state(centres)
        labels, _ = km.calc_best(x, need_mean=False)
        _cache[(n, d, K)] = (x, centres, km, np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels, np.int64))
    return _cache[(n, d, K)]


def _compare(x, centres, labels, m, got, what):
    """got = (probes, dist) of the kernel against the restatement; no row is left out"""
    probes, dist, gap, room = R.probe_centers(x, centres, labels, m)
    slack = (gap / np.maximum(room, np.finfo(float).tiny)).min() if gap.size else np.inf
    print("{}: n {} d {} K {} m {}: smallest gap / bounds summed {:.3g}".format(what, len(x), x.shape[1], len(centres), m, slack))
    assert (gap > 4 * room).all(), "the restatement does not decide every rank"
    assert got[0].dtype == np.int64 and got[0].shape == probes.shape and np.array_equal(got[0], probes)
    fin = np.isfinite(dist)
    assert np.array_equal(np.isposinf(got[1]), ~fin) and not np.isnan(got[1]).any()
    B = R.dist_bound(x, centres)
    allowed = np.take_along_axis(B, np.maximum(probes, 0), 1)
    err = np.abs(got[1][fin] - dist[fin]) / allowed[fin]
    print("{}: largest |dist - restatement| / bound {:.3g}".format(what, err.max()))
    assert (err <= 1.0).all()
    return probes, dist


@pytest.mark.parametrize("n,d,K,m", SHAPES, ids=["n{}-d{}-K{}-m{}".format(*s) for s in SHAPES])
def test_lists_and_distances_match_the_restatement(torch_gpu, n, d, K, m):
    x, centres, km, labels = _case(n, d, K)
    got = km.probe_centers(x, m, labels, dists=True)
    _compare(x, centres, labels, m, got, "host input")
    assert np.array_equal(km.probe_centers(x, m), got[0])  # labels=None: calc_best's
    # dist[:, 0] and dist[:, 1] are quality's a2 and b2, bit for bit
    _stats, rows = km.quality(x, labels, rows=True)
    assert got[1][:, 0].tobytes() == rows[:, 0].tobytes() and got[1][:, 1].tobytes() == rows[:, 1].tobytes()
    # a list is a prefix of a longer one
    longer = km.probe_centers(x, min(16, m + 3), labels, dists=True)
    assert longer[0][:, :m].tobytes() == got[0].tobytes() and longer[1][:, :m].tobytes() == got[1].tobytes()


def test_sixteen_probes_past_one_pass_of_centres(torch_gpu):
    x, centres, km, labels = _case(40000, 8, 133)
    got = km.probe_centers(x[:3000], 16, labels[:3000], dists=True)
    _compare(x[:3000], centres, labels[:3000], 16, got, "m = 16")
    with pytest.raises(ValueError, match="m=17"):
        km.probe_centers(x[:10], 17)


def test_labels_that_are_not_the_nearest_centre(torch_gpu):
    n, d, K, m = 600, 24, 7, 3
    x, centres, km, labels = _case(n, d, K)
    moved = labels.copy()
    moved[::3] = (moved[::3] + 2) % K
    got = km.probe_centers(x, m, moved, dists=True)
    probes, _dist = _compare(x, centres, moved, m, got, "moved labels")
    assert (got[0][:, 0] == moved).all() and (got[0][::3, 1] == labels[::3]).all()  # slot 0 the label, then the nearest centre
    assert not (got[0][:, 1:] == moved[:, None]).any()                                # the rest skip the label
    _stats, rows = km.quality(x, moved, rows=True)
    assert got[1][:, :2].tobytes() == rows.tobytes() and (rows[::3, 1] < rows[::3, 0]).all()


def test_equal_centres_tie_exactly_and_the_lower_index_comes_first(torch_gpu):
    n, d, K, m = 600, 24, 7, 4
    x, centres, _km, _labels = _case(n, d, K)
    centres = centres.copy()
    centres[5] = centres[2]  # two bitwise-equal centres
    km = _state(centres)
    labels = np.full(n, 0, np.int64)
    got = km.probe_centers(x, m, labels, dists=True)
    _compare(x, centres, labels, m, got, "equal centres")
    at = [np.flatnonzero(row == 2) for row in got[0]]
    hit = [i for i, a in enumerate(at) if len(a) and a[0] + 1 < m]
    assert len(hit) >= 50  # the rows that list centre 2 before their last slot
    for i in hit:
        p = at[i][0]
        assert got[0][i, p + 1] == 5 and got[1][i, p] == got[1][i, p + 1]


def test_fewer_centres_than_probes(torch_gpu):
    rs = np.random.RandomState(2)
    x = rs.randn(200, 5).astype(np.float32)
    two = _state(x[:2] + np.float32(0.5))
    labels = np.asarray(two.calc_best(x, need_mean=False)[0])
    got = two.probe_centers(x, 3, labels, dists=True)
    _compare(x, x[:2] + np.float32(0.5), labels, 3, got, "K = 2")
    assert (got[0][:, 1] == 1 - labels).all() and (got[0][:, 2] == -1).all() and np.isposinf(got[1][:, 2]).all()
    one = _state(x[:1].copy())
    got = one.probe_centers(x, 2, dists=True)
    assert (got[0] == [0, -1]).all() and np.isposinf(got[1][:, 1]).all()
    assert got[1][:, 0].tobytes() == one.quality(x, np.zeros(200, np.int64), rows=True)[1][:, 0].tobytes()
    assert got[1][0, 0] == 0.0  # the row that is the centre


def test_purity_pieces_device_unaligned_and_a_second_call(torch_gpu):
    torch = torch_gpu
    n, d, K, m = 2000, 70, 12, 4
    x, _centres, km, labels = _case(n, d, K)
    want = km.probe_centers(x, m, labels, dists=True)
    same = lambda got: got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()  # noqa: E731
    assert same(km.probe_centers(x, m, labels, dists=True))
    cuts = [0, 333, 1430, n]  # three pieces of unequal length, none a multiple of 64
    pieces = [km.probe_centers(x[a:b], m, labels[a:b], dists=True) for a, b in zip(cuts[:-1], cuts[1:])]
    assert same((np.concatenate([p[0] for p in pieces]), np.concatenate([p[1] for p in pieces])))
    xd = torch.from_numpy(x).cuda()
    assert same(km.probe_centers(xd, m, torch.from_numpy(labels).cuda(), dists=True))
    buf = torch.empty(xd.numel() + 1, dtype=torch.float32, device="cuda")
    off = buf[1:].view(n, d)
    off.copy_(xd)
    assert off.data_ptr() % 16 == 4 and same(km.probe_centers(off, m, labels, dists=True))


def test_refusals_leave_the_outputs_untouched(torch_gpu):
    from acav100m_amd import _lib
    from acav100m_amd.clustering import KMeans
    lib = _lib.load_library()
    x, _centres, km, labels = _case(600, 24, 7)
    probes, dist = np.full((600, 3), -9, np.int64), np.full((600, 3), 7.5)
    call = lambda h, lab, m, n=600, xp=x, pp=probes: lib.acav_kmeans_probes(  # noqa: E731
        h, _lib.ptr(xp), n, _lib.ptr(lab), m, _lib.ptr(pp), _lib.ptr(dist))
    h = km._require_handle()
    bad = labels.copy()
    bad[[3, 599]] = [7, -1]
    assert call(h, bad, 3) == -1 and "2 of 600 labels" in lib.acav_last_error().decode()
    for kw in (dict(m=0), dict(m=17), dict(m=3, n=-1), dict(m=3, xp=None), dict(m=3, pp=None), dict(m=3, lab=None)):
        assert call(h, kw.pop('lab', labels), **kw) == -1, kw
    assert call(None, labels, 3) == -1
    warm = KMeans(None, 24, 7).to("cuda:0")  # count = 0: the warm-up
    assert call(warm._require_handle(), labels, 3) != 0 and "warm-up" in lib.acav_last_error().decode()
    with pytest.raises(_lib.AcavError, match="warm-up"):
        warm.probe_centers(x, 3, labels)
    with pytest.raises(ValueError):
        km.probe_centers(x, True)
    with pytest.raises(ValueError):
        km.probe_centers(x[:, :5], 3)
    assert (probes == -9).all() and (dist == 7.5).all()
    assert call(h, labels, 3) == 0 and (probes[:, 0] == labels).all() and not (dist == 7.5).any()
    assert call(h, labels, 3, n=0) == 0
