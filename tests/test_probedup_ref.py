"""CPU: the device-free side of the multi-probe dedup -- the numpy restatements of tests/_probedup_np.py against the brute force
over all pairs and, at m = 1, against the restatements of acav_rows_neardup and acav_rows_crossdup; the report keys of
summarise / summarise_against; dedup.check_options for dedup.probes; acav_rows_probedup_plan against the restatement of the rule
the header states, and the triangle: in the in-set use m probes walk at most m times acav_rows_neardup_plan's blocks plus two
edge blocks per tile."""
import ctypes as C

import numpy as np
import pytest

from tests import _crossdup_np as RC
from tests import _neardup_np as RN
from tests import _probedup_np as R

PLAN_LEN = 6


def _data(n, my, d, k, m, seed, inset=False):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, d).astype(np.float32)
    y = x if inset else rs.randn(my, d).astype(np.float32)
    centres = (x[rs.choice(n, k, replace=False)] + 0.25 * rs.randn(k, d)).astype(np.float32)
    lx = R.distances(x, centres).argmin(1)
    ly = lx if inset else R.distances(y, centres).argmin(1)
    probes = R.probe_centers(x, centres, lx, m)[0]
    return x, y, centres, lx, ly, probes


@pytest.mark.parametrize("n,d,k,m", [(150, 6, 7, 3), (200, 3, 5, 5), (60, 9, 2, 3), (40, 4, 1, 2)])
def test_the_probes_restatement_equals_the_brute_force(n, d, k, m):
    x, _y, centres, lx, _ly, _ = _data(n, n, d, k, m, seed=n, inset=True)
    lx = lx.copy()
    lx[::7] = (lx[::7] + 1) % k  # labels that are not the nearest centre: slot 0 is the label, the rest skip it
    probes, dist, gap, _room = R.probe_centers(x, centres, lx, m)
    want = R.brute_force_probes(x, centres, lx, m)
    assert np.array_equal(probes, want[0]) and np.array_equal(dist, want[1])
    assert (probes[:, 0] == lx).all() and (probes[:, min(m, k):] == -1).all() and np.isinf(dist[:, min(m, k):]).all()
    assert (np.diff(dist[:, 1:], axis=1) >= 0).all() and gap.shape == (n, m - 1) and (gap >= 0).all()


@pytest.mark.parametrize("inset", [True, False], ids=["in-set", "against"])
def test_the_pair_restatement_equals_the_brute_force(inset):
    n, my, d, k, m = 160, 90, 5, 6, 3
    x, y, _c, _lx, ly, probes = _data(n, my, d, k, m, seed=3, inset=inset)
    x = x.copy()
    y = x if inset else y.copy()
    probes = probes.copy()
    x[11] = 0.0                     # a zero query (and, in-set, a zero candidate)
    y[40] = y[7]                    # bitwise copies among the candidates: the lower position is named
    probes[5, 1] = -1               # a -1 slot
    probes[6, 2] = probes[6, 0]     # a repeated label counts once
    before = np.arange(n) if inset else None
    best, partner, second, each = R.nearest(x, y, probes, ly, before)
    want = R.brute_force(x, y, probes, ly, before)
    assert np.array_equal(partner, want[1])
    has = partner >= 0
    assert np.array_equal(np.isneginf(best), ~has) and np.abs(best[has] - want[0][has]).max() <= R.bound(d)
    fin = np.isfinite(want[2])
    assert np.array_equal(np.isfinite(each), fin) and np.abs(each[fin] - want[2][fin]).max() <= R.bound(d)
    assert np.array_equal(best, each.max(1)) and (second <= best).all()
    assert partner[11] == -1 and np.isneginf(each[5, 1]) and np.isneginf(each[6, 2]) and has.sum() > n // 2


def test_with_one_probe_it_is_the_neardup_and_the_crossdup_restatement():
    n, my, d, k = 300, 120, 7, 5
    x, y, _c, lx, ly, _ = _data(n, my, d, k, 1, seed=9)
    def same(a, b):
        """partner identical; best and the runner-up of the rows that have one within the bound (the two restatements take
        the norms from different BLAS calls)"""
        has = b[1] >= 0
        return (np.array_equal(a[1], b[1]) and has.sum() > n // 2 and np.array_equal(np.isneginf(a[0]), ~has)
                and np.allclose(a[0][has], b[0][has], rtol=0, atol=R.bound(d))
                and np.allclose(a[2][has], b[2][has], rtol=0, atol=R.bound(d)))

    assert same(R.nearest(x, x, lx[:, None], lx, np.arange(n)), RN.nearest_earlier(x, lx, k))
    assert same(R.nearest(x, y, lx[:, None], ly), RC.nearest_in(x, y, lx, ly))


def test_the_report_keys_of_a_multi_probe_run():
    from acav100m_amd.clustering.dedup import probe_pairs, summarise, summarise_against
    n, my, d, k, m, thr = 400, 150, 4, 6, 4, 0.9
    x, y, _c, lx, ly, probes = _data(n, my, d, k, m, seed=5)
    best, partner, _s, each = R.nearest(x, x, probes, lx, np.arange(n))
    one = R.nearest(x, x, probes[:, :1], lx, np.arange(n))
    base = summarise(one[0], one[1], lx, k, thr)
    assert summarise(one[0], one[1], lx, k, thr, probes=probes[:, :1], best_each=one[3]) == base  # probes = 1: today's keys
    got = summarise(best, partner, lx, k, thr, probes=probes, best_each=each)
    assert set(got) == set(base) | {'probes', 'pairs', 'flagged_by_probes'} and got['probes'] == m
    curve = got['flagged_by_probes']
    assert len(curve) == m and curve[0] == base['flagged'] and curve == sorted(curve) and curve[-1] == got['flagged'] > curve[0]
    by_hand = sum(int((lx[:i] == c).sum()) for i in range(n) for c in probes[i])
    assert got['pairs'] == by_hand == probe_pairs(probes, lx, np.arange(n))
    # against a held-out set
    hist_y = np.bincount(ly, minlength=k)
    best, partner, _s, each = R.nearest(x, y, probes, ly)
    one = R.nearest(x, y, probes[:, :1], ly)
    base = summarise_against(one[0], one[1], lx, hist_y, k, thr, my)
    assert summarise_against(one[0], one[1], lx, hist_y, k, thr, my, probes_x=probes[:, :1], best_each=one[3]) == base
    got = summarise_against(best, partner, lx, hist_y, k, thr, my, probes_x=probes, best_each=each)
    assert set(got) == set(base) | {'probes', 'flagged_by_probes'} and got['probes'] == m
    curve = got['flagged_by_probes']
    assert curve[0] == base['flagged'] and curve == sorted(curve) and curve[-1] == got['flagged']
    assert got['pairs'] == int(hist_y[probes].sum()) > base['pairs']
    # a -1 slot and a repeated label count no pair
    odd = probes.copy()
    odd[0, 1], odd[1, 2] = -1, odd[1, 0]
    assert probe_pairs(odd, ly) == int(hist_y[probes].sum()) - int(hist_y[probes[0, 1]]) - int(hist_y[probes[1, 2]])
    with pytest.raises(ValueError):
        summarise(best, partner, lx, k, thr, probes=probes)
    with pytest.raises(ValueError):
        summarise_against(best, partner, None, None, 1, thr, my, probes_x=probes, best_each=each)


def test_check_options_refuses_bad_probes_before_anything_is_read():
    from acav100m_amd.clustering.dedup import check_options, check_probes
    ok = {'threshold': 0.95, 'out_path': 'dups.csv'}
    against = dict(ok, against_path='held/shard-{000000..000001}.pkl', against_meta_path='held/videos')
    assert check_probes(ok) == 1 and check_probes(dict(ok, probes=1)) == 1 and check_probes(dict(ok, probes=16), k=16) == 16
    assert check_options(dict(ok, probes=3)) == (0.95, None, 'dups.csv', None)  # the old answer: the key is only checked
    assert check_options(dict(ok, probes=3), k=3) == (0.95, None, 'dups.csv', None)
    assert check_probes(dict(against, blocking='cluster', probes=2), k=4) == 2
    for bad, k, match in ((dict(ok, probes=0), None, "dedup.probes"), (dict(ok, probes=17), None, "dedup.probes"),
                          (dict(ok, probes=True), None, "dedup.probes"), (dict(ok, probes=2.0), None, "dedup.probes"),
                          (dict(ok, probes='2'), None, "dedup.probes"), (dict(ok, probes=5), 4, "exceeds the K=4"),
                          (dict(against, probes=2), None, "blocking=none"),
                          (dict(against, blocking='none', probes=2), None, "blocking=none")):
        with pytest.raises(ValueError, match=match):
            check_options(bad, k=k)
        with pytest.raises(ValueError, match=match):
            check_probes(bad, k)
    assert check_options(dict(against, probes=1)) == (0.95, None, 'dups.csv', None)  # one probe is today's run, blocked or not


def test_parse_cli_reads_the_key_as_an_integer():
    from acav100m_amd.config import CLUSTERING_DEFAULTS, merge, parse_cli
    _command, kwargs = parse_cli(['dedup', '--feature_path=f', '--clustering.cached_epoch=3', '--dedup.threshold=0.99',
                                  '--dedup.out_path=dups.csv', '--dedup.probes=3'])
    assert merge(CLUSTERING_DEFAULTS, kwargs).get('dedup') == {'threshold': 0.99, 'out_path': 'dups.csv', 'probes': 3}


# ------------------------------------------------------------------ acav_rows_probedup_plan
@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _plan(lib, probes, labels_y, before, k, d=8, cus=256):
    pr, ly = np.ascontiguousarray(probes, np.int64), np.ascontiguousarray(labels_y, np.int64)
    bf = None if before is None else np.ascontiguousarray(before, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = (ptr(pr), pr.shape[0], pr.shape[1], ptr(ly), len(ly), ptr(bf), k, d, cus)
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    assert lib.acav_rows_probedup_plan(*args, out, None, 0) == 0, lib.acav_last_error()
    tiles = np.full((out[1], 4), -7, np.int64)
    again = (C.c_int64 * PLAN_LEN)()
    assert lib.acav_rows_probedup_plan(*args, again, ptr(tiles), len(tiles)) == 0
    assert tuple(again) == tuple(out)
    return tuple(out), tiles.tolist()


def _neardup_blocks(lib, labels, k, cus):
    hist = np.bincount(labels, minlength=k).astype(np.int64)
    out = (C.c_int64 * PLAN_LEN)()
    assert lib.acav_rows_neardup_plan(hist.ctypes.data_as(C.c_void_p), k, 8, cus, out, None, 0) == 0
    return out[0], out[2]


def _ring(labels, k, m):
    """row i probes its own cluster and the m - 1 next ones: every cluster is probed by as many rows of each of m clusters"""
    return (labels[:, None] + np.arange(m)[None, :]) % k


CASES = {
    # the labels interleaved (i mod k), equal clusters: every probed cluster is as large as the own one
    "interleaved": lambda rs: (np.arange(3000) % 6, 6, 3),
    # one cluster holds half the rows, the others share the rest
    "skewed": lambda rs: (np.where(rs.rand(2500) < 0.5, 0, rs.randint(1, 9, 2500)), 9, 4),
    "two-clusters": lambda rs: (rs.randint(0, 2, 700), 2, 2),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("cus", [4, 256], ids=["H128", "H64"])
def test_plan_against_the_restated_rule_in_set_and_against(lib, case, cus):
    labels, k, m = CASES[case](np.random.RandomState(1))
    labels = labels.astype(np.int64)
    n = len(labels)
    probes = _ring(labels, k, m)
    for before, ly in ((np.arange(n), labels), (None, labels[:n // 3]), (np.random.RandomState(2).randint(-5, n + 5, n), labels)):
        out, tiles = _plan(lib, probes, ly, before, k, cus=cus)
        want, want_tiles = R.plan(probes, ly, before, cus)
        assert out[:3] == want and out[3] == out[1] and tiles == want_tiles
        E, my = n * m, len(ly)
        assert out[0] == (128 if cus == 4 else 64) and out[4] == 8 * out[0] * 65
        assert out[5] == 4 * (3 * E + my + n * m) + 8 * (E + my) + 16 * out[1] + 16 * (E + n) + 8 * n * m


def test_plan_with_missing_slots_repeated_labels_and_clusters_without_rows(lib):
    rs = np.random.RandomState(4)
    n, k, m = 900, 7, 4
    lx = rs.randint(0, 5, n).astype(np.int64)     # the clusters 5 and 6 hold no row of y ...
    probes = _ring(lx, k, m)                       # ... and are probed all the same
    probes[rs.rand(n) < 0.2, 3] = -1               # lists with -1
    rep = rs.rand(n) < 0.2
    probes[rep, 2] = probes[rep, 0]                # and with a repeated label
    probes[5] = -1                                 # a row without any probe
    out, tiles = _plan(lib, probes, lx, np.arange(n), k, cus=256)
    want, want_tiles = R.plan(probes, lx, np.arange(n), 256)
    assert out[:3] == want and tiles == want_tiles
    assert any(t[3] == 0 for t in tiles)           # the entries of the empty clusters walk nothing
    counted = R._counted(probes)
    assert sum(t[1] for t in tiles) == int(counted.sum()) < n * m


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("cus", [4, 256], ids=["H128", "H64"])
def test_the_triangle_m_probes_walk_at_most_m_times_the_blocks_plus_two_per_tile(lib, case, cus):
    """In-set, with the ring lists (every cluster is probed by as many rows of each of m clusters, in input order: the probing
    rows of a cluster are as many as m times its own).  A tile of H entries of cluster c ends at an entry whose row has at
    most ceil(e / m) + (a cluster's lead over its ring neighbours) rows of c before it, e its rank among c's entries, so the m
    tiles that cover what ONE neardup tile covers walk its prefix each: m times the blocks, plus the block a prefix ends in
    and the one it starts in (shared with the previous run) per tile.  The lead is the further edge term: it is 0 for
    interleaved labels; for random labels the counts below show whether it is needed."""
    labels, k, m = CASES[case](np.random.RandomState(1))
    labels = labels.astype(np.int64)
    n = len(labels)
    H, base = _neardup_blocks(lib, labels, k, cus)
    out, _tiles = _plan(lib, _ring(labels, k, m), labels, np.arange(n), k, cus=cus)
    assert out[0] == H
    print("{}: neardup {} blocks; {} probes {} blocks in {} tiles".format(case, base, m, out[2], out[1]))
    assert out[2] <= m * base + 2 * out[1]
    one, _ = _plan(lib, labels[:, None], labels, np.arange(n), k, cus=cus)
    assert one[2] <= base + 2 * one[1] and one[1] == -(-n // H)


def test_plan_refusals(lib):
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    pr = np.array([[0, 1], [1, 0], [2, -1]], np.int64)
    ly, bf = np.array([0, 1, 2, 2], np.int64), np.arange(3, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tiles = np.zeros((1, 4), np.int64)
    good = [p(pr), 3, 2, p(ly), 4, p(bf), 3, 8, 256, out, None, 0]
    for at, value in ((0, None), (3, None), (9, None), (1, 0), (1, 2 ** 31), (2, 0), (2, 17), (4, 0), (4, 2 ** 31), (6, 0),
                      (6, 2), (7, 0), (7, 16385), (8, 0)):   # k = 2: the probe 2 and the label 2 are outside
        args = list(good)
        args[at] = value
        assert lib.acav_rows_probedup_plan(*args) == -1, (at, value)
    bad = pr.copy()
    bad[1, 1] = -2
    assert lib.acav_rows_probedup_plan(*([p(bad)] + good[1:])) == -1 and b"probes" in lib.acav_last_error()
    bad = ly.copy()
    bad[0] = 3
    assert lib.acav_rows_probedup_plan(*(good[:3] + [p(bad)] + good[4:])) == -1 and b"labels of y" in lib.acav_last_error()
    big = np.zeros((200, 1), np.int64)
    assert lib.acav_rows_probedup_plan(p(big), 200, 1, p(ly), 4, None, 3, 8, 1, out, p(tiles), 1) == -1  # two tiles, room for one
    assert tuple(out) == (-7,) * PLAN_LEN and not tiles.any()
    assert lib.acav_rows_probedup_plan(*good) == 0 and out[1] == 1
