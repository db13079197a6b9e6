"""GPU: acav_rows_neardup (clustering/dedup.py: nearest_earlier) against the float64 restatement of tests/_neardup_np.py: best
within the bound the header derives, partner identical -- after the restatement alone has shown that every row's partner is
decided (the gap to the runner-up exceeds four times the bound; bitwise copies of the partner excepted, they tie exactly and the
lowest position wins).  Shapes past one tile, one column block, one stage of d and both tile heights; host, device and
unaligned input; the same bytes from a second call and from one cluster passed alone; the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import _neardup_np as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _rows(seed, n, d, k, copies=0, interleaved=False):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, d).astype(np.float32)
    lab = (np.arange(n) % k if interleaved else rs.randint(0, k, n)).astype(np.int64)
    for _ in range(copies):  # a later row becomes a bitwise copy of an earlier one, in its cluster
        s, t = np.sort(rs.choice(n, 2, replace=False))
        x[t], lab[t] = x[s], lab[s]
    return x, lab


def _compare(x, lab, k, got, what):
    """got = (best, partner) of the kernel against the restatement; no row is left out"""
    d = x.shape[1]
    best, partner, second = R.nearest_earlier(x, lab, k)
    b = R.bound(d)
    has = partner >= 0
    gap = (best[has] - second[has]).min() if has.any() else np.inf
    print("{}: n {} d {} k {}: {} rows with a partner, smallest gap to the runner-up {:.3g}, bound {:.3g}".format(
        what, len(lab), d, k, int(has.sum()), gap, b))
    assert gap > 4 * b, "the restatement does not decide every partner"
    err = np.abs(got[0][has] - best[has]).max() if has.any() else 0.0
    print("{}: largest |best - restatement| {:.3g}".format(what, err))
    assert np.array_equal(np.isneginf(got[0]), ~has) and not np.isnan(got[0]).any()
    assert err <= b
    assert np.array_equal(got[1], partner)
    return best, partner


SHAPES = [  # (n, d, k, interleaved labels, planted copies)
    (600, 24, 4, True, 12),    # the permutation is not the identity; 64-row tiles, three column blocks per cluster
    (2000, 70, 6, False, 20),  # d neither a multiple of 4 nor of 32: the guarded loads, a zero-filled tail in the third stage
    (300, 3, 2, False, 4),     # d below one MFMA step
    (40000, 8, 133, False, 50),  # 128-row tiles on 256 compute units, 313 workgroups, about five column blocks per cluster
]


@pytest.mark.parametrize("n,d,k,inter,copies", SHAPES, ids=["n{}-d{}-k{}".format(*s[:3]) for s in SHAPES])
def test_best_and_partner_match_the_restatement(torch_gpu, n, d, k, inter, copies):
    from acav100m_amd.clustering.dedup import nearest_earlier
    x, lab = _rows(n + d, n, d, k, copies, inter)
    got = nearest_earlier(x, lab, k)
    best, partner = _compare(x, lab, k, got, "host input")
    copies_found = int((np.abs(best - 1.0) <= R.bound(d)).sum())
    assert copies_found >= 1  # the planted copies come out within the bound of 1
    again = nearest_earlier(x, lab, k)  # the same call, the same bytes
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


def test_d_1_every_cosine_is_exactly_plus_or_minus_one(torch_gpu):
    """d = 1: cos = a b / sqrt(fl(a^2 b^2)) with a b and both squares exact, and sqrt(fl(t^2)) = |t| in IEEE arithmetic: every
    cosine is exactly +-1 in the kernel and in numpy alike, every row ties exactly, the lowest earlier row of its sign wins"""
    from acav100m_amd.clustering.dedup import nearest_earlier
    x, lab = _rows(5, 300, 1, 3)
    best, partner, _ = R.nearest_earlier(x, lab, 3)
    assert set(np.unique(best)) <= {-np.inf, -1.0, 1.0}
    got = nearest_earlier(x, lab, 3)
    assert np.array_equal(got[0], best) and np.array_equal(got[1], partner)


def test_small_clusters_ties_and_zero_rows(torch_gpu):
    from acav100m_amd.clustering.dedup import nearest_earlier
    n, d, k = 150, 12, 6
    x, _ = _rows(9, n, d, k)
    lab = np.full(n, 3, np.int64)  # labels 2 and 5 are empty
    lab[10] = 0                    # a cluster of one
    lab[[20, 90]] = 1              # a cluster of two
    lab[100:] = 4
    x[0] = 0.0                     # a zero row that is the first of its cluster
    x[[30, 31, 120]] = 0.0         # zero rows inside clusters
    x[40] = x[5]                   # two bitwise-equal earlier rows ...
    x[60] = x[5]                   # ... and a third: its partner is the lowest, 5
    x[130] = x[101]
    got = nearest_earlier(x, lab, k)
    _compare(x, lab, k, got, "small clusters")
    assert got[1][10] == -1 and got[1][20] == -1 and got[1][90] == 20
    assert got[1][40] == 5 and got[1][60] == 5 and got[1][130] == 101
    assert abs(got[0][60] - 1.0) <= R.bound(d) and got[0][40] == got[0][60]
    for z in (0, 30, 31, 120):
        assert got[1][z] == -1 and np.isneginf(got[0][z])
    assert not np.isin(got[1], [0, 30, 31, 120]).any()  # a zero row is never a partner
    assert got[1][1] == -1  # only the zero row 0 lies before row 1


def test_device_unaligned_and_torch_labels_give_the_same_bytes(torch_gpu):
    torch = torch_gpu
    from acav100m_amd.clustering.dedup import nearest_earlier
    for n, d, k in ((600, 24, 4), (700, 70, 5)):
        x, lab = _rows(3, n, d, k, copies=5)
        want = nearest_earlier(x, lab, k)
        xd = torch.from_numpy(x).cuda()
        on_dev = nearest_earlier(xd, torch.from_numpy(lab).cuda(), k)
        buf = torch.empty(n * d + 1, dtype=torch.float32, device="cuda")
        off = buf[1:].view(n, d)  # off 16-byte alignment by one float: the guarded loads
        off.copy_(xd)
        assert off.data_ptr() % 16 == 4
        shifted = nearest_earlier(off, lab, k)
        for got in (on_dev, shifted):
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_one_cluster_alone_gives_its_bytes_of_the_full_call(torch_gpu):
    from acav100m_amd.clustering.dedup import nearest_earlier
    n, d, k = 40000, 8, 133
    x, lab = _rows(n + d, n, d, k, 50)  # the large shape: 128-row tiles in the full call, 64-row tiles for a cluster alone
    full = nearest_earlier(x, lab, k)
    for c in (0, 77, 132):
        idx = np.flatnonzero(lab == c)
        alone = nearest_earlier(x[idx], np.zeros(len(idx), np.int64), 1)
        assert alone[0].tobytes() == full[0][idx].tobytes()
        mapped = np.where(alone[1] >= 0, idx[np.maximum(alone[1], 0)], -1)
        assert np.array_equal(mapped, full[1][idx])


def test_refusals_leave_the_outputs_untouched(torch_gpu):
    from acav100m_amd import _lib
    lib = _lib.load_library()
    x, lab = _rows(1, 200, 8, 3)
    best, partner = np.full(200, 7.5), np.full(200, -9, np.int64)

    def call(x, lab, n=200, d=8, k=3, xp=True, lp=True, bp=True, pp=True):
        return lib.acav_rows_neardup(0, _lib.ptr(x) if xp else None, n, d, _lib.ptr(lab) if lp else None, k,
                                     _lib.ptr(best) if bp else None, _lib.ptr(partner) if pp else None, None)

    bad_lab = lab.copy()
    bad_lab[[3, 150]] = [3, -1]
    assert call(x, bad_lab) == -1
    assert "2 of 200 labels" in lib.acav_last_error().decode()
    bad_x = x.copy()
    bad_x[7, 2], bad_x[9, 0], bad_x[199, 7] = np.nan, np.inf, -np.inf
    assert call(bad_x, lab) == -1
    assert "3 of the" in lib.acav_last_error().decode() and "not finite" in lib.acav_last_error().decode()
    for kw in (dict(n=0), dict(n=2 ** 31), dict(d=0), dict(d=16385), dict(k=0), dict(xp=False), dict(lp=False), dict(bp=False),
               dict(pp=False)):
        assert call(x, lab, **kw) == -1, kw
    assert (best == 7.5).all() and (partner == -9).all()
    with pytest.raises(ValueError, match="labels are outside"):
        from acav100m_amd.clustering.dedup import nearest_earlier
        nearest_earlier(x, bad_lab, 3)
    assert call(x, lab) == 0 and np.isneginf(best[0]) and partner[0] == -1
