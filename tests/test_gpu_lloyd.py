"""GPU: acav_rows_absmax, acav_lloyd_accumulate and the Lloyd loop against the numpy restatement (tests/_lloyd_np.py), bit for
bit: the tables are integer sums, the centres one float64 expression of them, the labels the assign sweep's."""
import numpy as np
import pytest

from tests import _lloyd_np as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _rows(seed, n, d):
    rs = np.random.RandomState(seed)
    return (rs.randn(n, d) * np.exp(rs.uniform(-3, 3, d))).astype(np.float32)


@pytest.mark.parametrize("n,d", [(1000, 88), (4099, 130), (3, 2304)])
def test_absmax_is_numpys(torch, n, d):
    from acav100m_amd.clustering import rows_absmax
    x = _rows(n, n, d)
    want = float(np.abs(x).max())
    assert rows_absmax(x) == want  # host rows
    xt = torch.from_numpy(x).cuda()
    assert rows_absmax(xt) == want
    assert rows_absmax(xt[1:]) == float(np.abs(x[1:]).max())  # rows that start off 16 bytes when d % 4 != 0
    # the largest value in the last element (a tail), negative
    x[-1, -1] = -3e30
    assert rows_absmax(torch.from_numpy(x).cuda()) == float(np.float32(3e30))
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[n // 2, d // 3] = bad
        with pytest.raises(ValueError, match="not finite"):
            rows_absmax(torch.from_numpy(y).cuda())


def _labels(case, n, k, seed):
    rs = np.random.RandomState(seed)
    if case == "skewed":  # one cluster with 2 500 rows, one empty
        lab = rs.randint(0, k, n)
        lab[(lab == 1) | (lab == 2)] = 0
        lab[rs.permutation(n)[:2500]] = 1
        return lab.astype(np.int64)
    if case == "singles":  # two thirds of the clusters hold one row each, scattered over the rows
        lab = rs.randint(2 * k // 3, k, n)
        lab[rs.permutation(n)[:2 * k // 3]] = np.arange(2 * k // 3)
        return lab.astype(np.int64)
    return rs.randint(0, k, n).astype(np.int64)


CASES = [("skewed", 3000, 88, 5), ("singles", 4099, 1408, 300), ("even", 700, 64, 1024)]


@pytest.fixture(scope="module")
def accumulated(torch):
    """per case: rows, labels, s and the restatement's tables -- computed once"""
    out = {}
    for case, n, d, k in CASES:
        x = _rows(n + d, n, d)
        lab = _labels(case, n, k, n)
        s = L.shift_of(np.abs(x).max(), n)
        out[n] = (x, lab, k, s) + L.sums_counts(x, lab, k, s)
    return out


@pytest.mark.parametrize("n", [c[1] for c in CASES])
def test_accumulate_is_the_restatement(torch, accumulated, n):
    from acav100m_amd.clustering import accumulate
    x, lab, k, s, sums, counts = accumulated[n]
    d = x.shape[1]
    if n == 3000:
        assert (counts == 2500).any() and (counts == 0).any()
    if n == 4099:
        assert (counts == 1).sum() == 200 and d > 64 * 16  # one-row lists, more strips than one round of a workgroup's waves
    if n == 700:
        assert k > n
    xt, lt = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()

    def run(pieces, on_dev=True, host_rows=False):
        if on_dev:
            S, Cn = torch.zeros((k, d), dtype=torch.int64, device="cuda"), torch.zeros(k, dtype=torch.int64, device="cuda")
        else:
            S, Cn = np.zeros((k, d), np.int64), np.zeros(k, np.int64)
        for a, b in zip(pieces[:-1], pieces[1:]):
            accumulate(x[a:b] if host_rows else xt[a:b], lab[a:b] if host_rows else lt[a:b], s, S, Cn)
        return (S.cpu().numpy(), Cn.cpu().numpy()) if on_dev else (S, Cn)

    one = run([0, n])
    assert one[0].dtype == np.int64 and np.array_equal(one[0], sums) and np.array_equal(one[1], counts)
    three = run([0, 1, n // 3 + 7, n])  # three calls of uneven size into the same tables
    assert np.array_equal(three[0], sums) and np.array_equal(three[1], counts)
    again = run([0, n])  # a second run: the same bits
    assert again[0].tobytes() == one[0].tobytes() and again[1].tobytes() == one[1].tobytes()
    host = run([0, n // 2, n], on_dev=False, host_rows=True)  # host rows, labels and tables
    assert np.array_equal(host[0], sums) and np.array_equal(host[1], counts)


def test_accumulate_adds_to_what_is_there_and_refuses_bad_labels(torch, accumulated):
    from acav100m_amd.clustering import accumulate
    x, lab, k, s, sums, counts = accumulated[3000]
    d = x.shape[1]
    S = torch.full((k, d), -5, dtype=torch.int64, device="cuda")
    Cn = torch.full((k,), 11, dtype=torch.int64, device="cuda")
    accumulate(torch.from_numpy(x).cuda(), lab, s, S, Cn)
    assert np.array_equal(S.cpu().numpy(), sums - 5) and np.array_equal(Cn.cpu().numpy(), counts + 11)
    for bad in (-1, k, 2 ** 40):
        wrong = lab.copy()
        wrong[1234] = bad
        before = S.clone()
        with pytest.raises(ValueError, match="label"):
            accumulate(torch.from_numpy(x).cuda(), wrong, s, S, Cn)
        assert torch.equal(S, before)  # nothing was added


def test_accumulate_at_the_extremes_of_the_scale(torch):
    """values next to the largest magnitude, at both ends of fp32's range: no sum overflows, every bit is the restatement's"""
    from acav100m_amd.clustering import accumulate, fixed_point_shift, rows_absmax
    for scale in (1e-30, 1e30):
        x = np.full((1500, 70), scale, np.float32)  # every |x| is (next to) absmax, one cluster takes nearly all of them
        x[:, 1::2] *= -1
        x[::2, ::3] *= np.float32(0.999)
        lab = np.zeros(1500, np.int64)
        lab[:3] = 1
        s = fixed_point_shift(rows_absmax(x), 1500)
        assert s == L.shift_of(np.abs(x).max(), 1500)
        S, Cn = np.zeros((2, 70), np.int64), np.zeros(2, np.int64)
        accumulate(x, lab, s, S, Cn)
        want = L.sums_counts(x, lab, 2, s)
        assert np.array_equal(S, want[0]) and np.array_equal(Cn, want[1])
        assert np.abs(S).min(1).max() > 2 ** 59 and (S[:, 1::2] < 0).all()  # the sums really use the 64 bits, in both signs


def _g1(seed=0, n=2048, d=64, k=16):
    rs = np.random.RandomState(seed)
    cen = rs.randn(k, d).astype(np.float32)
    return (cen[rs.randint(0, k, n)] + 0.5 * rs.randn(n, d)).astype(np.float32)


def _run_loop(torch, x, centers0, iters):
    """the package's loop from given initial centres -> per iteration (labels, centers, sizes, splits, changed), and the KMeans"""
    from acav100m_amd.clustering import KMeans, fixed_point_shift, rows_absmax
    from acav100m_amd.clustering.lloyd import finish_iteration
    k, d = centers0.shape
    xt = torch.from_numpy(x).cuda()
    km = KMeans(None, d, k).to_lloyd(centers0).to("cuda:0")
    s = fixed_point_shift(rows_absmax(xt), len(x))
    out, prev = [], None
    for _t in range(iters):
        labels, sums, counts = km.lloyd_update(xt, s)
        labels = labels.cpu().numpy()
        changed = len(x) if prev is None else int((labels != prev).sum())
        splits = finish_iteration(km, sums, counts, s)
        out.append(dict(labels=labels, centers=km.centers.numpy().copy(), sizes=km.counts.numpy().astype(np.int64), splits=splits,
                        changed=changed, count=km.count))
        prev = labels
        if changed == 0:
            break
    return out, km, xt


def _same(got, want, n):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["labels"], w["labels"]), t
        assert g["centers"].tobytes() == w["centers"].tobytes(), t
        assert np.array_equal(g["sizes"], w["sizes"]) and g["splits"] == w["splits"] and g["changed"] == w["changed"], t
        assert g["count"] == n * (t + 1)


def test_loop_is_the_restatement(torch):
    import acav100m_amd
    x = _g1()
    acav100m_amd.manual_seed(11)
    from acav100m_amd.rng import default_generator
    perm = default_generator.randperm(len(x))[:16]
    assert len(set(perm.tolist())) == 16
    want = L.loop(x, x[perm], 8)
    got, km, xt = _run_loop(torch, x, x[perm], 8)
    _same(got, want, len(x))
    changed = [g["changed"] for g in got]
    print("changed labels per iteration:", changed)
    assert changed[0] == len(x) and (changed[-1] == 0 or all(b <= a for a, b in zip(changed, changed[1:])))
    assert all(g["splits"] == 0 for g in got)
    stats = km.quality(xt)
    assert int(stats[:, 4].sum()) == 0  # displaced: every row sits at its nearest centre
    assert km.algorithm == "lloyd" and km.initial_rounds == 0 and tuple(km.reinit) == (.7, 1.0)
    # fit(): the same run from the seeded generator
    from acav100m_amd.clustering import fit
    acav100m_amd.manual_seed(11)
    km2, labels2, report = fit(xt, 16, 8)
    assert km2.centers.numpy().tobytes() == got[-1]["centers"].tobytes() and np.array_equal(labels2.cpu().numpy(), got[-1]["labels"])
    assert [r[0] for r in report] == changed


def test_a_start_that_forces_empty_clusters(torch):
    x = _g1(seed=3)
    c0 = x[np.random.RandomState(4).permutation(len(x))[:16]].copy()
    c0[[2, 5, 9, 15]] = np.float32(1e4)  # four copies far from every row: they win no row
    want = L.loop(x, c0, 4)
    assert want[0]["splits"] == 4
    got, _km, _xt = _run_loop(torch, x, c0, 4)
    _same(got, want, len(x))
    print("splits per iteration:", [g["splits"] for g in got])
