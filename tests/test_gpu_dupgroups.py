"""GPU: acav_rows_neardup_pairs (clustering/dedup.py: pairs_earlier) against the float64 restatement of tests/_dupgroups_np.py:
offsets and pair_j identical, pair_cos within the bound the header derives, best and partner the bytes of nearest_earlier --
after the restatement alone has shown that no cosine of the input lies within four times the bound of the threshold.  Shapes
past one tile, one column block, one stage of d and both tile heights, a row with more than 128 pairs; the invariants that tie
the pairs to (best, partner); host, device and unaligned input; one cluster passed alone; a cap below the total; the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _dupgroups_np as G
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


@functools.lru_cache(maxsize=None)
def _case(n, d, k, inter, copies, t):
    """the rows of a shape and their restated pairs, computed once and shared (never written to)"""
    x, lab = _rows(n + d, n, d, k, copies, inter)
    ref = G.pairs(x, lab, t)
    for a in (x, lab) + ref[:3]:
        a.setflags(write=False)
    return x, lab, ref


def _invariants(got, t):
    best, partner, offsets, pair_j, pair_cos = got
    n = len(best)
    deg = np.diff(offsets)
    assert offsets[0] == 0 and (deg >= 0).all() and offsets[n] == len(pair_j) == len(pair_cos)
    assert np.array_equal(deg > 0, best >= t)
    rows = np.flatnonzero(deg > 0)
    if len(rows):
        top = np.maximum.reduceat(pair_cos, offsets[rows])
        assert top.tobytes() == best[rows].tobytes()  # bit for bit: the same chain
        later = np.repeat(np.arange(n), deg)
        first = np.full(n, -1, np.int64)
        hit = np.flatnonzero(pair_cos == best[later])[::-1]
        first[later[hit]] = pair_j[hit]  # reversed: the first pair that attains the maximum stays
        assert np.array_equal(first[rows], partner[rows])
        assert (pair_j < later).all() and (pair_cos >= t).all()
        assert all(np.all(np.diff(pair_j[offsets[i]:offsets[i + 1]]) > 0) for i in rows[:200])  # ascending input position


def _compare(x, lab, k, t, ref, got, what):
    """got = pairs_earlier's five arrays against the restatement; no row is left out"""
    from acav100m_amd.clustering.dedup import nearest_earlier
    d = x.shape[1]
    offsets, pair_j, pair_cos, margin = ref
    b = R.bound(d)
    print("{}: n {} d {} k {} t {}: {} pairs, largest degree {}, nearest cosine to the threshold {:.3g}, bound {:.3g}".format(
        what, len(lab), d, k, t, offsets[-1], np.diff(offsets).max(), margin, b))
    assert margin > 4 * b, "the restatement does not decide every pair"
    assert np.array_equal(got[2], offsets) and np.array_equal(got[3], pair_j)
    err = np.abs(got[4] - pair_cos).max() if len(pair_cos) else 0.0
    print("{}: largest |pair_cos - restatement| {:.3g}".format(what, err))
    assert err <= b
    plain = nearest_earlier(x, lab, k)
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
    _invariants(got, t)


SHAPES = [  # (n, d, k, interleaved labels, planted copies, threshold) -> pairs, largest degree
    ((600, 24, 4, True, 12, 0.5), (241, 4)),       # the permutation is not the identity; 64-row tiles
    ((2000, 70, 6, False, 20, 0.3), (1847, 7)),    # the guarded loads, a zero-filled tail in d
    ((300, 3, 2, False, 4, 0.5), (5618, 46)),      # d below one MFMA step, many pairs per row
    ((600, 3, 1, False, 0, 0.02), (None, None)),   # a row with more than 128 pairs: they span at least three column blocks
    ((40000, 8, 133, False, 50, 0.9), (2893, 3)),  # 128-row tiles on 256 compute units, 313 workgroups
    ((40000, 8, 133, False, 50, 0.995), (50, 1)),  # the planted copies alone: most tiles hold no pair
]


@pytest.mark.parametrize("shape,want", SHAPES, ids=["n{}-d{}-k{}-t{}".format(s[0], s[1], s[2], s[5]) for s, _ in SHAPES])  # = IDS
def test_pairs_match_the_restatement(torch_gpu, shape, want):
    from acav100m_amd.clustering.dedup import pairs_earlier
    n, d, k, _inter, _copies, t = shape
    x, lab, ref = _case(*shape)
    deg = np.diff(ref[0])
    if want[0] is None:
        assert deg.max() > 128  # on the restatement
    else:
        assert (int(ref[0][-1]), int(deg.max())) == want
    got = pairs_earlier(x, lab, t, k)
    _compare(x, lab, k, t, ref, got, "host input")
    again = pairs_earlier(x, lab, t, k)  # the same call, the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_the_groups_of_the_first_shape(torch_gpu):
    from acav100m_amd.clustering.dedup import choose_kept, components, pairs_earlier
    shape = SHAPES[0][0]
    x, lab, _ref = _case(*shape)
    best, _partner, offsets, pair_j, _cos = pairs_earlier(x, lab, shape[5], shape[2])
    root = components(len(lab), offsets, pair_j)
    size = np.bincount(root, minlength=len(lab))
    kept = choose_kept(root, 'first')
    assert (int((size >= 2).sum()), int(size.max()), int((~kept & ~(best >= shape[5])).sum())) == (97, 19, 41)
    assert np.array_equal(root, G.components(len(lab), offsets, pair_j))


def test_the_emit_sweep_launches_the_tiles_that_hold_a_pair(torch_gpu):
    """40 000 rows at t = 0.995: the pairs are the 50 planted copies, 46 of the 313 tiles hold a later copy, and the plan entry
    -- the function the entry point launches from -- names exactly those"""
    from acav100m_amd import _lib
    lib = _lib.load_library()
    shape = SHAPES[5][0]
    n, d, k = shape[:3]
    _x, lab, ref = _case(*shape)
    cus = torch_gpu.cuda.get_device_properties(0).multi_processor_count
    hist = np.bincount(lab, minlength=k).astype(np.int64)
    plain = (C.c_int64 * 6)()
    assert lib.acav_rows_neardup_plan(_lib.ptr(hist), k, d, cus, plain, None, 0) == 0
    H, count_tiles = plain[0], plain[1]
    perm = np.argsort(lab, kind='stable')
    flags = np.zeros(count_tiles, np.uint8)
    flags[np.flatnonzero(np.diff(ref[0])[perm] > 0) // H] = 1
    out = (C.c_int64 * 7)()
    tiles = np.full((count_tiles, 4), -7, np.int64)
    assert lib.acav_rows_neardup_pairs_plan(_lib.ptr(hist), k, d, cus, _lib.ptr(flags), out, _lib.ptr(tiles), count_tiles) == 0
    assert (out[0], out[1], out[2]) == (plain[0], plain[1], plain[2]) and out[3] == int(flags.sum())
    assert sorted(tiles[:out[3], 0].tolist()) == (np.flatnonzero(flags) * H).tolist() and (tiles[out[3]:] == -7).all()
    assert out[4] == tiles[:out[3], 3].sum() < out[2]
    key = [(-b, q) for q, _r, _c, b in tiles[:out[3]].tolist()]
    assert key == sorted(key)  # the longest first
    assert H == (128 if 313 >= cus else 64)  # the plan's rule: ceil(40000 / 128) = 313 tiles of 128 rows once they fill the device
    if H == 128:  # the figures of the shape (the MI355X has 256 compute units)
        assert (count_tiles, out[3]) == (313, 46)


def test_d_1_at_threshold_1_the_pairs_are_the_earlier_rows_of_the_same_sign(torch_gpu):
    """d = 1: every cosine is exactly +-1 in the kernel and in numpy alike (tests/test_gpu_neardup.py states why), so the pairs
    at t = 1.0 are compared exactly, without a margin: all earlier rows of the cluster with the row's sign"""
    from acav100m_amd.clustering.dedup import pairs_earlier
    x, lab = _rows(5, 300, 1, 3)
    offsets, pair_j, pair_cos, _margin = G.pairs(x, lab, 1.0)
    assert set(np.unique(pair_cos)) == {1.0}
    sign = np.sign(x[:, 0])
    want = [[j for j in range(i) if lab[j] == lab[i] and sign[j] == sign[i]] for i in range(300)]
    assert [list(pair_j[offsets[i]:offsets[i + 1]]) for i in range(300)] == want
    got = pairs_earlier(x, lab, 1.0, 3)
    assert np.array_equal(got[2], offsets) and np.array_equal(got[3], pair_j) and np.array_equal(got[4], pair_cos)
    _invariants(got, 1.0)


def test_small_clusters_copies_and_zero_rows(torch_gpu):
    from acav100m_amd.clustering.dedup import components, pairs_earlier
    n, d, k, t = 150, 12, 6, 0.7
    x, _ = _rows(9, n, d, k)
    lab = np.full(n, 3, np.int64)  # labels 2 and 5 are empty
    lab[10] = 0                    # a cluster of one
    lab[[20, 90]] = 1              # a cluster of two ...
    x[90] = x[20]                  # ... that is a pair
    lab[100:] = 4
    x[0] = 0.0                     # a zero row that is the first of its cluster
    x[[30, 31, 120]] = 0.0         # zero rows inside clusters
    x[40] = x[5]                   # three bitwise-equal rows: a triangle
    x[60] = x[5]
    x[130] = x[101]
    ref = G.pairs(x, lab, t)
    got = pairs_earlier(x, lab, t, k)
    _compare(x, lab, k, t, ref, got, "small clusters")
    offsets, pair_j = got[2], got[3]
    row = lambda i: pair_j[offsets[i]:offsets[i + 1]].tolist()  # noqa: E731
    assert row(90) == [20] and row(40) == [5] and row(60) == [5, 40] and row(130) == [101] and row(10) == [] and row(20) == []
    for z in (0, 30, 31, 120):  # a zero row has no pairs and is in none
        assert row(z) == []
    assert not np.isin(pair_j, [0, 30, 31, 120]).any()
    root = components(n, offsets, pair_j)
    assert root[[5, 40, 60]].tolist() == [5, 5, 5] and root[90] == 20 and root[130] == 101 and root[0] == 0


@functools.lru_cache(maxsize=None)
def _full(shape):
    """pairs_earlier of a shape's host rows, once (never written to)"""
    from acav100m_amd.clustering.dedup import pairs_earlier
    x, lab, _ref = _case(*shape)
    got = pairs_earlier(x, lab, shape[5], shape[2])
    for a in got:
        a.setflags(write=False)
    return got


IDS = ["n{}-d{}-k{}-t{}".format(s[0], s[1], s[2], s[5]) for s, _ in SHAPES]


@pytest.mark.parametrize("shape", [s for s, _ in SHAPES], ids=IDS)
def test_device_unaligned_and_torch_labels_give_the_same_bytes(torch_gpu, shape):
    """on every shape; the 40 000-row shapes off alignment are the 128-row tiles with guarded loads"""
    torch = torch_gpu
    from acav100m_amd.clustering.dedup import pairs_earlier
    n, d, k, t = shape[0], shape[1], shape[2], shape[5]
    x, lab, _ref = _case(*shape)
    want = _full(shape)
    xd = torch.from_numpy(x.copy()).cuda()  # the shared arrays are read-only: torch wants writable memory
    on_dev = pairs_earlier(xd, torch.from_numpy(lab.copy()).cuda(), t, k)
    buf = torch.empty(n * d + 1, dtype=torch.float32, device="cuda")
    off = buf[1:].view(n, d)  # off 16-byte alignment by one float: the guarded loads
    off.copy_(xd)
    assert off.data_ptr() % 16 == 4
    shifted = pairs_earlier(off, lab, t, k)
    for got in (on_dev, shifted):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


def test_device_outputs_receive_the_same_bytes(torch_gpu):
    torch = torch_gpu
    from acav100m_amd import _lib
    from acav100m_amd.clustering.dedup import pairs_earlier
    lib = _lib.load_library()
    shape = SHAPES[0][0]
    n, d, k, t = shape[0], shape[1], shape[2], shape[5]
    x, lab, _ref = _case(*shape)
    want = pairs_earlier(x, lab, t, k)
    total = int(want[2][n])
    dev = [torch.full((n,), 7.5, dtype=torch.float64, device="cuda"), torch.full((n,), -9, dtype=torch.int64, device="cuda"),
           torch.full((n + 1,), -9, dtype=torch.int64, device="cuda"), torch.full((total + 3,), -9, dtype=torch.int64, device="cuda"),
           torch.full((total + 3,), 7.5, dtype=torch.float64, device="cuda")]
    torch.cuda.synchronize()
    assert lib.acav_rows_neardup_pairs(0, _lib.ptr(x), n, d, _lib.ptr(lab), k, t, _lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]),
                                       total + 3, _lib.ptr(dev[3]), _lib.ptr(dev[4]), None) == 0
    got = [a.cpu().numpy() for a in dev]
    assert all(a[:len(b)].tobytes() == b.tobytes() for a, b in zip(got, want))
    assert (got[3][total:] == -9).all() and (got[4][total:] == 7.5).all()  # nothing beyond offsets[n]


@pytest.mark.parametrize("shape", [s for s, _ in SHAPES], ids=IDS)
def test_one_cluster_alone_gives_its_pairs_of_the_full_call(torch_gpu, shape):
    """on every shape: the first and the last cluster and the one with the most pairs (at 40 000 rows: 128-row tiles in the full
    call, 64-row tiles for a cluster alone)"""
    from acav100m_amd.clustering.dedup import pairs_earlier
    k, t = shape[2], shape[5]
    x, lab, _ref = _case(*shape)
    full = _full(shape)
    deg = np.diff(full[2])
    most = int(np.bincount(lab, weights=deg, minlength=k).argmax())
    assert deg[lab == most].sum() > 0
    for c in sorted({0, most, k - 1}):
        idx = np.flatnonzero(lab == c)
        alone = pairs_earlier(x[idx], np.zeros(len(idx), np.int64), t, 1)
        assert np.array_equal(np.diff(alone[2]), deg[idx])
        at = np.concatenate([np.arange(full[2][i], full[2][i + 1]) for i in idx])
        assert np.array_equal(idx[alone[3]], full[3][at]) and alone[4].tobytes() == full[4][at].tobytes()
        assert alone[0].tobytes() == full[0][idx].tobytes()
        assert np.array_equal(np.where(alone[1] >= 0, idx[np.maximum(alone[1], 0)], -1), full[1][idx])


def test_duplicate_groups_of_a_kmeans_state(torch_gpu):
    """KMeans.duplicate_groups: the labels are calc_best's (labels=None), the groups components' of pairs_earlier on them, keep=
    'central' chooses by quality(rows=True)'s a2"""
    from acav100m_amd.clustering import KMeans
    from acav100m_amd.clustering.dedup import choose_kept, components, pairs_earlier
    shape = SHAPES[0][0]
    n, d, k, t = shape[0], shape[1], shape[2], shape[5]
    x, _lab, _ref = _case(*shape)
    centres = np.random.RandomState(4).randn(k, d).astype(np.float32)
    km = KMeans(None, d, k).to_lloyd(centres).to("cuda:0")
    labels, _ = km.calc_best(x, need_mean=False)
    labels = labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)
    _best, _partner, offsets, pair_j, _cos = pairs_earlier(x, labels, t, k)
    want = components(n, offsets, pair_j)
    assert (np.bincount(want, minlength=n) >= 2).sum() > 10  # there are groups to choose in
    root, kept = km.duplicate_groups(x, t)
    assert np.array_equal(root, want) and np.array_equal(kept, want == np.arange(n))
    a2 = km.quality(x, labels, rows=True)[1][:, 0]
    root_c, kept_c = km.duplicate_groups(x, t, labels=labels, keep='central')
    assert np.array_equal(root_c, want) and np.array_equal(kept_c, choose_kept(want, 'central', a2))
    assert not np.array_equal(kept_c, kept)  # in some group the central row is not the first
    assert np.array_equal(kept_c, G.choose_kept(want, 'central', a2))
    with pytest.raises(ValueError, match="keep"):
        km.duplicate_groups(x, t, keep='last')


def test_a_cap_below_the_total_fills_the_offsets_and_leaves_the_pairs_alone(torch_gpu, monkeypatch):
    from acav100m_amd import _lib
    from acav100m_amd.clustering import dedup
    lib = _lib.load_library()
    shape = SHAPES[2][0]
    n, d, k, t = shape[0], shape[1], shape[2], shape[5]
    x, lab, ref = _case(*shape)
    total = int(ref[0][-1])
    best, partner, offsets = np.full(n, 7.5), np.full(n, -9, np.int64), np.full(n + 1, -9, np.int64)
    pair_j, pair_cos = np.full(total, -9, np.int64), np.full(total, 7.5)

    def call(cap, pj=pair_j, pc=pair_cos):
        return lib.acav_rows_neardup_pairs(0, _lib.ptr(x), n, d, _lib.ptr(lab), k, t, _lib.ptr(best), _lib.ptr(partner), _lib.ptr(offsets),
                                           cap, _lib.ptr(pj), _lib.ptr(pc), None)

    assert call(total - 1) == 0
    assert np.array_equal(offsets, ref[0]) and (pair_j == -9).all() and (pair_cos == 7.5).all() and best[1] != 7.5
    offsets[:] = -9
    assert call(0, None, None) == 0 and np.array_equal(offsets, ref[0])  # the pure count call
    assert call(total, pair_j, None) == 0 and np.array_equal(pair_j, ref[1]) and (pair_cos == 7.5).all()  # pair_cos not wanted
    assert call(total) == 0 and np.abs(pair_cos - ref[2]).max() <= R.bound(d)
    # pairs_earlier: a first call with too little room, then one with the exact size
    monkeypatch.setattr(dedup, "FIRST_CAP", 16)
    got = dedup.pairs_earlier(x, lab, t, k)
    assert np.array_equal(got[2], ref[0]) and np.array_equal(got[3], pair_j) and got[4].tobytes() == pair_cos.tobytes()
    assert dedup.pairs_earlier(x, lab, t, k, max_pairs=total)[3].tobytes() == pair_j.tobytes()
    per = np.bincount(lab, weights=np.diff(ref[0]), minlength=k).astype(np.int64)
    with pytest.raises(ValueError, match="{} pairs .* more than max_pairs = {}; the clusters with the most: .*{}: {}.*raise the "
                                         "threshold".format(total, total - 1, int(per.argmax()), int(per.max()))):
        dedup.pairs_earlier(x, lab, t, k, max_pairs=total - 1)


def test_refusals_leave_the_outputs_untouched(torch_gpu):
    from acav100m_amd import _lib
    lib = _lib.load_library()
    x, lab = _rows(1, 200, 8, 3)
    best, partner, offsets = np.full(200, 7.5), np.full(200, -9, np.int64), np.full(201, -9, np.int64)
    pair_j, pair_cos = np.full(4000, -9, np.int64), np.full(4000, 7.5)

    def call(x, lab, n=200, d=8, k=3, t=0.5, cap=4000, xp=True, lp=True, bp=True, pp=True, op=True, jp=True):
        return lib.acav_rows_neardup_pairs(0, _lib.ptr(x) if xp else None, n, d, _lib.ptr(lab) if lp else None, k, t,
                                           _lib.ptr(best) if bp else None, _lib.ptr(partner) if pp else None,
                                           _lib.ptr(offsets) if op else None, cap, _lib.ptr(pair_j) if jp else None, _lib.ptr(pair_cos), None)

    bad_lab = lab.copy()
    bad_lab[[3, 150]] = [3, -1]
    assert call(x, bad_lab) == -1
    assert "2 of 200 labels" in lib.acav_last_error().decode()
    bad_x = x.copy()
    bad_x[7, 2], bad_x[9, 0], bad_x[199, 7] = np.nan, np.inf, -np.inf
    assert call(bad_x, lab) == -1
    assert "3 of the" in lib.acav_last_error().decode() and "not finite" in lib.acav_last_error().decode()
    for kw in (dict(n=0), dict(n=2 ** 31), dict(d=0), dict(d=16385), dict(k=0), dict(xp=False), dict(lp=False), dict(bp=False),
               dict(pp=False), dict(op=False), dict(t=0.0), dict(t=-0.5), dict(t=1.0000001), dict(t=float("nan")), dict(cap=-1),
               dict(jp=False), dict(jp=False, cap=1)):
        assert call(x, lab, **kw) == -1, kw
    assert (best == 7.5).all() and (partner == -9).all() and (offsets == -9).all() and (pair_j == -9).all() and (pair_cos == 7.5).all()
    with pytest.raises(ValueError, match="threshold"):
        from acav100m_amd.clustering.dedup import pairs_earlier
        pairs_earlier(x, lab, 1.5, 3)
    assert call(x, lab) == 0 and np.isneginf(best[0]) and partner[0] == -1 and offsets[0] == 0 and offsets[200] >= 0
