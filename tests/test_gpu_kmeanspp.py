"""GPU: acav_kmeanspp_weights and acav_kmeanspp_seed against the numpy restatement (tests/_kmeanspp_np.py), bit for bit -- the
weights are float64 sums in one stated order, everything after them is integer -- and lloyd.fit(init='kmeans++')."""
import numpy as np
import pytest

from tests import _kmeanspp_np as P
from tests.test_kmeanspp_ref import blobs

pytestmark = pytest.mark.gpu

B = P.BLOCK
DS = [1, 3, 63, 64, 65, 100, 257, 2304]
MS = [1, B - 1, B, B + 1, 2 * B + 1]
TS = [1, 2, 8, 16]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _rows(seed, m, d, scale=1.0):
    rs = np.random.RandomState(seed)
    return (rs.randn(m, d) * np.exp(rs.uniform(-2, 2, d)) * scale).astype(np.float32)


def _grid(d):
    """every m with one T each; over the eight d every (m, T) pair is met"""
    di = DS.index(d)
    return [(m, TS[(mi + di) % len(TS)]) for mi, m in enumerate(MS)]


def _cands(rs, m, T):
    c = rs.randint(0, m, T)
    c[0], c[-1] = m - 1, 0  # the last row and (T > 1) the first one are candidates; repeats are allowed
    return c.astype(np.int64)


@pytest.mark.parametrize("d", DS)
def test_weights_are_the_restatements(torch, d):
    from acav100m_amd.clustering import kmeanspp
    rs = np.random.RandomState(d)
    for m, T in _grid(d):
        x = _rows(m + d, m, d)
        t = P.shift_of(np.abs(x).max(), m, d)
        assert kmeanspp.weight_shift(np.abs(x).max(), m, d) == t
        cand = _cands(rs, m, T)
        want = P.weights(x, cand, t)
        got = kmeanspp.weights(x, cand, t)  # host rows
        assert got.dtype == np.int64 and got.shape == (T, m)
        assert np.array_equal(got, want), (m, T, "host")
        assert np.array_equal(kmeanspp.weights(torch.from_numpy(x).cuda(), cand, t), want), (m, T, "device")
        assert all(got[q, cand[q]] == 0 for q in range(T))


@pytest.mark.parametrize("d", [3, 65, 100])
def test_weights_of_rows_that_start_off_16_bytes(torch, d):
    from acav100m_amd.clustering import kmeanspp
    m = B + 2
    x = _rows(7 * d, m, d)
    t = P.shift_of(np.abs(x).max(), m, d)
    cand = np.array([0, m - 2, 5], np.int64)
    want = P.weights(x[1:], cand, t)
    xt = torch.from_numpy(x).cuda()
    assert xt[1:].data_ptr() % 16 != 0 or d % 4 == 0
    assert np.array_equal(kmeanspp.weights(xt[1:], cand, t), want)
    assert np.array_equal(kmeanspp.weights(x[1:], cand, t), want)


def test_weights_with_more_candidate_columns_than_lds_holds(torch):
    from acav100m_amd.clustering import kmeanspp
    m, d, T = 300, 4096, 16  # 16 x 4096 floats = 256 KB: four sweeps of four trials
    x = _rows(1, m, d)
    t = P.shift_of(np.abs(x).max(), m, d)
    cand = _cands(np.random.RandomState(2), m, T)
    assert np.array_equal(kmeanspp.weights(torch.from_numpy(x).cuda(), cand, t), P.weights(x, cand, t))


@pytest.mark.parametrize("scale", [1e-20, 1e20])
def test_weights_at_the_extremes_of_the_scale(torch, scale):
    from acav100m_amd.clustering import kmeanspp
    m, d = B + 1, 100
    x = _rows(3, m, d, scale)
    t = kmeanspp.weight_shift(np.abs(x).max(), m, d)
    assert t == P.shift_of(np.abs(x).max(), m, d) and (t > 100 if scale < 1 else t < -60)
    cand = np.array([m - 1, 17], np.int64)
    got = kmeanspp.weights(torch.from_numpy(x).cuda(), cand, t)
    assert np.array_equal(got, P.weights(x, cand, t))
    assert 2 ** 30 < int(got.max()) and int(got.sum(axis=1).max()) < 2 ** 62  # the weights are neither flushed nor overflowing


def _u(seed, k, T):
    return np.random.RandomState(seed).random_sample(1 + (k - 1) * T)


@pytest.mark.parametrize("d", DS)
def test_seeds_are_the_restatements(torch, d):
    from acav100m_amd.clustering import kmeanspp
    for m, T in _grid(d):
        k = min(m, 4 if d < 1000 else 2)  # (the restatement's cost is k T sweeps in numpy)
        x = _rows(m * 3 + d, m, d)
        u = _u(m + d, k, T)
        want = P.seed(x, k, T, u)
        got = kmeanspp.seed(torch.from_numpy(x).cuda(), k, T, u=u)
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (m, T)
        if d in (3, 2304):
            host = kmeanspp.seed(x, k, T, u=u)  # host rows
            assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1]), (m, T, "host")


def test_seeds_with_more_candidate_columns_than_lds_holds(torch):
    from acav100m_amd.clustering import kmeanspp
    m, d, T, k = 300, 4096, 16, 3
    x = _rows(4, m, d)
    u = _u(5, k, T)
    got, want = kmeanspp.seed(torch.from_numpy(x).cuda(), k, T, u=u), P.seed(x, k, T, u)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_seeds_do_not_depend_on_the_stream_or_the_side_of_the_rows(torch):
    from acav100m_amd.clustering import kmeanspp
    m, d, k, T = 2 * B + 77, 88, 9, 3
    x = _rows(8, m, d)
    u = _u(9, k, T)
    xt = torch.from_numpy(x).cuda()
    one = kmeanspp.seed(xt, k, T, u=u)
    stream = torch.cuda.Stream()
    two = kmeanspp.seed(xt, k, T, u=u, stream=stream.cuda_stream)
    host = kmeanspp.seed(x, k, T, u=u)
    off = kmeanspp.seed(torch.from_numpy(np.concatenate([x[:1], x])).cuda()[1:], k, T, u=u)
    want = P.seed(x, k, T, u)
    for got in (one, two, host, off):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the generator's uniforms: two draws per value, and the same seeds as the explicit array
    from acav100m_amd.rng import Generator
    g, h = Generator(5), Generator(5)
    uu = kmeanspp.uniforms(h, 1 + (k - 1) * T)
    drawn = kmeanspp.seed(xt, k, T, generator=g)
    assert g.u32() == h.u32()
    again = kmeanspp.seed(xt, k, T, u=uu)
    assert np.array_equal(drawn[0], again[0]) and np.array_equal(drawn[1], again[1])


def test_edge_uniforms_pick_the_first_and_the_last_row_of_weight(torch):
    from acav100m_amd.clustering import kmeanspp
    m, d = B + 5, 20
    x = _rows(12, m, d)
    x[1] = x[0]          # a duplicate of the first pick: weight 0, skipped
    x[m - 2] = x[m - 1]
    xt = torch.from_numpy(x).cuda()
    for T in (1, 2):
        rows, pot = kmeanspp.seed(xt, 4, T, u=np.zeros(1 + 3 * T))
        assert rows.tolist() == [0, 2, 3, 4]
        want = P.seed(x, 4, T, np.zeros(1 + 3 * T))
        assert np.array_equal(rows, want[0]) and np.array_equal(pot, want[1])
        last = np.full(1 + 3 * T, 1 - 2.0 ** -53)
        rows, pot = kmeanspp.seed(xt, 4, T, u=last)
        assert rows.tolist() == [m - 1, m - 3, m - 4, m - 5]
        want = P.seed(x, 4, T, last)
        assert np.array_equal(rows, want[0]) and np.array_equal(pot, want[1])


def test_every_row_is_chosen_once_when_k_is_m(torch):
    from acav100m_amd.clustering import kmeanspp
    m, d = 70, 6
    x = _rows(13, m, d)
    u = _u(14, m, 2)
    rows, pot = kmeanspp.seed(torch.from_numpy(x).cuda(), m, 2, u=u)
    assert sorted(rows.tolist()) == list(range(m)) and pot[-1] == 0 and (np.diff(pot) < 0).all()
    want = P.seed(x, m, 2, u)
    assert np.array_equal(rows, want[0]) and np.array_equal(pot, want[1])


def test_duplicates_are_never_picked_twice_and_one_centre_too_many_is_a_value_error(torch):
    from acav100m_amd.clustering import kmeanspp
    base = _rows(15, 9, 33)
    x = base[np.random.RandomState(16).randint(0, 9, B + 40)]
    x[:9] = base  # every distinct row is there
    xt = torch.from_numpy(x).cuda()
    u = _u(17, 9, 3)
    rows, pot = kmeanspp.seed(xt, 9, 3, u=u)
    assert len({x[r].tobytes() for r in rows}) == 9 and pot[-1] == 0
    want = P.seed(x, 9, 3, u)
    assert np.array_equal(rows, want[0]) and np.array_equal(pot, want[1])
    with pytest.raises(ValueError, match="only 9 distinct rows"):
        kmeanspp.seed(xt, 10, 3, u=_u(18, 10, 3))
    with pytest.raises(ValueError, match="only 9 distinct rows"):
        kmeanspp.seed(xt, 12, 1, u=_u(18, 12, 1))
    again = kmeanspp.seed(xt, 9, 3, u=u)  # the refusal leaves the library working
    assert np.array_equal(again[0], rows) and np.array_equal(again[1], pot)


def test_two_trials_on_the_same_row_tie_to_the_lower_one(torch):
    from acav100m_amd.clustering import kmeanspp
    m, d, k, T = 500, 10, 5, 3
    x = _rows(19, m, d)
    u = _u(20, k, T)
    u[1:] = np.repeat(u[1::T], T)  # the T trials of a pick share their uniform: the same row, the same potential
    rows, pot = kmeanspp.seed(torch.from_numpy(x).cuda(), k, T, u=u)
    single = kmeanspp.seed(torch.from_numpy(x).cuda(), k, 1, u=u[[0] + list(range(1, len(u), T))])
    assert np.array_equal(rows, single[0]) and np.array_equal(pot, single[1])
    want = P.seed(x, k, T, u)
    assert np.array_equal(rows, want[0]) and np.array_equal(pot, want[1])


def test_bad_arguments_are_value_errors(torch):
    from acav100m_amd.clustering import kmeanspp
    x = _rows(21, 50, 8)
    with pytest.raises(ValueError):
        kmeanspp.seed(x, 51, 1, u=np.zeros(51))
    with pytest.raises(ValueError):
        kmeanspp.seed(x, 3, 1, u=np.zeros(4))      # a u of the wrong length
    with pytest.raises(ValueError):
        kmeanspp.seed(x, 3, 1, u=np.array([0.5, 1.0, 0.5]))  # outside [0, 1)
    with pytest.raises(ValueError):
        kmeanspp.weights(x, [50], 3)
    with pytest.raises(ValueError):
        kmeanspp.weights(x, [0], 1001)
    with pytest.raises(ValueError):
        kmeanspp.weights(x, list(range(17)), 3)


@pytest.mark.parametrize("trials", [1, 'auto'])
def test_fit_finds_the_blobs_from_kmeanspp_seeds(torch, trials):
    from acav100m_amd.clustering import lloyd
    from acav100m_amd.rng import Generator
    x, ids = blobs()
    km, labels, report = lloyd.fit(x, 16, 10, generator=Generator(3), init='kmeans++', trials=trials)
    labels = labels.cpu().numpy()
    pairs = {(int(a), int(b)) for a, b in zip(ids, labels)}
    assert len(pairs) == 16 and len({a for a, _ in pairs}) == 16 and len({b for _, b in pairs}) == 16
    assert all(splits == 0 for _changed, splits in report) and report[-1][0] == 0 and len(report) == 2
    assert report.potential.shape == (16,) and (np.diff(report.potential) < 0).all()
    # the sample: all rows (1024 < 256 k), in ascending order; the seeds are the restatement's from the generator's uniforms
    g = Generator(3)
    rows = np.sort(g.randperm(1024))
    T = P.trials_for(16, trials)
    want = P.seed(x[rows], 16, T, P.uniforms(g.u32, 1 + 15 * T))
    assert np.array_equal(report.potential, want[1])
    assert len({int(i) for i in ids[rows[want[0]]]}) == 16


def test_fit_with_random_init_draws_what_it_drew(torch):
    from acav100m_amd.clustering import lloyd
    from acav100m_amd.rng import Generator
    x, _ids = blobs()
    g, h = Generator(4), Generator(4)
    km, _labels, report = lloyd.fit(x, 16, 2, generator=g)
    perm = h.randperm(1024)[:16]
    h.rand(16, 32)  # the KMeans object's own initial draw, as before
    a, b = g.get_state(), h.get_state()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert report.potential is None and isinstance(report, list)
    g2 = Generator(4)
    km2, _l2, report2 = lloyd.fit(x, 16, 2, generator=g2, init='random', trials=7, sample=100)  # the other keys are not looked at
    assert km2.centers.numpy().tobytes() == km.centers.numpy().tobytes() and list(report2) == list(report)
    assert np.array_equal(g2.get_state()[0], a[0])
    # the first iteration started from the rows of the permutation
    from tests import _lloyd_np as L
    want = L.loop(x, x[perm], 2)
    assert want[-1]["centers"].tobytes() == km.centers.numpy().tobytes()
