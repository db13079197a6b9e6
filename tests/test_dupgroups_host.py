"""CPU: the device-free side of the duplicate groups -- acav_pairs_components against the plain union-find of
tests/_dupgroups_np.py (random graphs, one row, no pairs, a star, a long path in the order that makes the deepest tree), its
refusals with root untouched, acav_rows_neardup_pairs_plan on hand-computed histograms, and check_groups, choose_kept,
summarise_groups and the two csv writers of clustering/dedup.py on synthetic arrays; `--exclude_path` reads the new csv."""
import csv
import ctypes as C

import numpy as np
import pytest

from tests import _dupgroups_np as G

PLAN_LEN = 7


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _csr(n, edges):
    """offsets, pair_j of undirected edges: each at its later row, ascending earlier row"""
    rows = [[] for _ in range(n)]
    for a, b in edges:
        rows[max(a, b)].append(min(a, b))
    rows = [sorted(set(r)) for r in rows]
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return offsets, np.array([j for r in rows for j in r], np.int64)


def _components(lib, n, offsets, pair_j, root=None):
    root = np.full(n, -5, np.int64) if root is None else root
    rc = lib.acav_pairs_components(n, offsets.ctypes.data_as(C.c_void_p), pair_j.ctypes.data_as(C.c_void_p) if pair_j is not None else None,
                                   root.ctypes.data_as(C.c_void_p))
    return rc, root


@pytest.mark.parametrize("seed,n,m", [(0, 50, 20), (1, 400, 150), (2, 400, 1200), (3, 3000, 2500)])
def test_components_of_random_graphs(lib, seed, n, m):
    rs = np.random.RandomState(seed)
    edges = [tuple(e) for e in rs.randint(0, n, (m, 2)) if e[0] != e[1]]
    offsets, pair_j = _csr(n, edges)
    rc, root = _components(lib, n, offsets, pair_j)
    assert rc == 0 and np.array_equal(root, G.components(n, offsets, pair_j))
    assert (root <= np.arange(n)).all() and np.array_equal(root[root], root)  # the lowest position, itself a root
    from acav100m_amd.clustering.dedup import components
    assert np.array_equal(components(n, offsets, pair_j), root)


def test_components_one_row_no_pairs_and_a_star(lib):
    rc, root = _components(lib, 1, np.zeros(2, np.int64), None)
    assert rc == 0 and root.tolist() == [0]
    rc, root = _components(lib, 7, np.zeros(8, np.int64), None)
    assert rc == 0 and root.tolist() == list(range(7))
    offsets, pair_j = _csr(9, [(5, j) for j in (0, 2, 3, 8)] + [(6, 7)])  # centre 5; 1 and 4 alone
    rc, root = _components(lib, 9, offsets, pair_j)
    assert rc == 0 and root.tolist() == [0, 1, 0, 0, 4, 0, 6, 6, 0]


def test_a_long_path_in_the_worst_order_does_not_touch_the_stack(lib):
    """the path L_m - H_0 - L_{m-1} - H_1 - ... - L_0 with L_k = k and H_k = m + 1 + k: row H_k joins the component found so far,
    whose root is L_{m-k}, to the new lower row L_{m-k-1}, so the roots chain L_m -> L_{m-1} -> ... -> L_0 -- a tree 50 000
    deep, no find on the way compresses it; a recursive find would need that many frames"""
    m = 50000
    n = 2 * m + 1
    offsets = np.zeros(n + 1, np.int64)
    offsets[m + 2:] = 2 * np.arange(1, m + 1)
    k = np.arange(m)
    pair_j = np.stack([m - k - 1, m - k], 1).reshape(-1).astype(np.int64)
    rc, root = _components(lib, n, offsets, pair_j)
    assert rc == 0 and not root.any()  # one component, its lowest row 0 (the plain restatement would walk the chain per find)


def test_components_refusals_leave_root_untouched(lib):
    offsets, pair_j = _csr(6, [(1, 0), (4, 2), (5, 4)])
    for off, pj, n in ((np.array([1, 1, 2, 2, 2, 3, 4], np.int64), pair_j, 6),      # does not start at 0
                       (np.array([0, 1, 1, 0, 1, 2, 3], np.int64), pair_j, 6),      # decreases
                       (offsets, np.array([0, 2, 6], np.int64), 6),                 # a partner outside [0, n)
                       (offsets, np.array([0, -1, 4], np.int64), 6),
                       (offsets, None, 6),                                          # pairs and no pair_j
                       (offsets, pair_j, 0)):
        rc, root = _components(lib, n, off, pj, np.full(6, -5, np.int64))
        assert rc == -1 and (root == -5).all(), (off, pj, n)
    root = np.full(6, -5, np.int64)
    assert lib.acav_pairs_components(6, None, pair_j.ctypes.data_as(C.c_void_p), root.ctypes.data_as(C.c_void_p)) == -1
    assert lib.acav_pairs_components(6, offsets.ctypes.data_as(C.c_void_p), pair_j.ctypes.data_as(C.c_void_p), None) == -1
    assert (root == -5).all()
    assert _components(lib, 6, offsets, np.array([0, 2, 6], np.int64))[0] == -1
    assert "outside [0, 6)" in lib.acav_last_error().decode()


def _pairs_plan(lib, hist, flags, d=8, cus=256):
    h, f = np.asarray(hist, np.int64), np.asarray(flags, np.uint8)
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    assert lib.acav_rows_neardup_pairs_plan(h.ctypes.data_as(C.c_void_p), len(h), d, cus, f.ctypes.data_as(C.c_void_p), out, None, 0) == 0
    tiles = np.full((max(out[3], 1), 4), -7, np.int64)
    again = (C.c_int64 * PLAN_LEN)()
    assert lib.acav_rows_neardup_pairs_plan(h.ctypes.data_as(C.c_void_p), len(h), d, cus, f.ctypes.data_as(C.c_void_p), again,
                                            tiles.ctypes.data_as(C.c_void_p), out[3]) == 0
    assert tuple(again) == tuple(out)
    return tuple(out), tiles[:out[3]]


def test_pairs_plan_on_hand_computed_histograms(lib):
    # 200 rows in runs of 100, 30, 70 (starts 0, 100, 130), 64-row tiles: tile 0 = blocks 0; tile 1 (first row 64, run 0) = 0 ... 1;
    # tile 2 (first row 128, run 1: block 1) = 1 ... 2; tile 3 (first row 192, run 2: block 2, last row 199) = 2 ... 3.  The count
    # sweep walks 7 blocks in the order 64, 128, 192, 0; flagged tiles 0 and 2: the emit sweep launches 128, then 0: 3 blocks
    hist = [100, 30, 70]
    out, tiles = _pairs_plan(lib, hist, [1, 0, 1, 0])
    scratch = 32 * 200 + 16 * 4 + 4 * 200 + 8 * 201 + 16 * 2
    assert out == (64, 4, 7, 2, 3, 8 * 64 * 65, scratch)
    assert tiles.tolist() == [[128, 64, 1, 2], [0, 64, 0, 1]]
    out, tiles = _pairs_plan(lib, hist, [0, 0, 0, 0])
    assert out[:5] == (64, 4, 7, 0, 0) and len(tiles) == 0
    out, tiles = _pairs_plan(lib, hist, [9, 1, 1, 255])  # every tile: the count sweep's list
    assert out[:5] == (64, 4, 7, 4, 7) and tiles.tolist() == [[64, 64, 0, 2], [128, 64, 1, 2], [192, 8, 2, 2], [0, 64, 0, 1]]
    # one run of 300 rows on one compute unit: 128-row tiles walking 2, 4 and 5 blocks; the last two are flagged
    out, tiles = _pairs_plan(lib, [300], [0, 1, 1], cus=1)
    assert out[:6] == (128, 3, 11, 2, 9, 8 * 128 * 65) and tiles.tolist() == [[256, 44, 0, 5], [128, 128, 0, 4]]


def test_pairs_plan_refusals(lib):
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    h, f = np.array([100, 30, 70], np.int64), np.array([1, 1, 1, 0], np.uint8)
    hp, fp = h.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    tiles = np.zeros((2, 4), np.int64)
    for args in ((None, 3, 8, 256, fp, out, None, 0), (hp, 3, 8, 256, None, out, None, 0), (hp, 3, 8, 256, fp, None, None, 0),
                 (hp, 0, 8, 256, fp, out, None, 0), (hp, 3, 0, 256, fp, out, None, 0), (hp, 3, 16385, 256, fp, out, None, 0),
                 (hp, 3, 8, 0, fp, out, None, 0), (hp, 3, 8, 256, fp, out, tiles.ctypes.data_as(C.c_void_p), 2)):  # three flagged tiles
        assert lib.acav_rows_neardup_pairs_plan(*args) == -1, args
    bad = np.array([-1, 5, 5], np.int64)
    assert lib.acav_rows_neardup_pairs_plan(bad.ctypes.data_as(C.c_void_p), 3, 8, 256, fp, out, None, 0) == -1
    assert tuple(out) == (-7,) * PLAN_LEN and not tiles.any()


def test_check_groups():
    from acav100m_amd.clustering.dedup import MAX_PAIRS, check_groups, check_options
    assert check_groups({}) == (False, None, None, None) and check_groups(None) == (False, None, None, None)
    assert check_groups({'groups': False}) == (False, None, None, None)
    assert check_groups({'groups': True}) == (True, 'first', MAX_PAIRS, None) and MAX_PAIRS == 2 ** 27
    assert check_groups({'groups': True, 'keep': 'central', 'max_pairs': 1000, 'groups_path': 'g.csv'}) == (True, 'central', 1000, 'g.csv')
    for key, value in (('keep', 'first'), ('max_pairs', 10), ('groups_path', 'g.csv')):
        for base in ({}, {'groups': False}):
            with pytest.raises(ValueError, match="only valid with --dedup.groups=True"):
                check_groups(dict(base, **{key: value}))
    with pytest.raises(ValueError, match="bipartite"):
        check_groups({'groups': True, 'against_path': 'h.pkl', 'against_meta_path': 'm'})
    with pytest.raises(ValueError, match="follow-up"):
        check_groups({'groups': True, 'probes': 2})
    assert check_groups({'groups': True, 'probes': 1})[0]
    for bad in ({'groups': 'yes'}, {'groups': 1}, {'groups': True, 'keep': 'last'}, {'groups': True, 'max_pairs': 0},
                {'groups': True, 'max_pairs': 2.5}, {'groups': True, 'max_pairs': True}, {'groups': True, 'groups_path': ''}):
        with pytest.raises(ValueError):
            check_groups(bad)
    # check_options refuses them before any file is read
    ok = {'threshold': 0.95, 'out_path': 'dups.csv'}
    assert check_options(dict(ok, groups=True, keep='central')) == (0.95, None, 'dups.csv', None)
    with pytest.raises(ValueError, match="only valid with"):
        check_options(dict(ok, keep='central'))
    with pytest.raises(ValueError, match="follow-up"):
        check_options(dict(ok, groups=True, probes=3))
    with pytest.raises(ValueError, match="bipartite"):
        check_options(dict(ok, groups=True, against_path='h.pkl', against_meta_path='m'))


def test_choose_kept():
    from acav100m_amd.clustering.dedup import choose_kept
    root = np.array([0, 1, 0, 3, 1, 0, 6, 3], np.int64)  # groups {0, 2, 5}, {1, 4}, {3, 7}; 6 alone
    assert choose_kept(root, 'first').tolist() == [True, True, False, True, False, False, True, False]
    a2 = np.array([5.0, 2.0, 1.0, 4.0, 2.0, 1.0, 9.0, 3.5])  # ties in {0, 2, 5} (2 and 5) and in {1, 4}: the lower position
    assert choose_kept(root, 'central', a2).tolist() == [False, True, True, False, False, False, True, True]
    rs = np.random.RandomState(0)
    root = G.components(200, *_csr(200, [tuple(e) for e in rs.randint(0, 200, (90, 2)) if e[0] != e[1]]))
    a2 = rs.randint(0, 4, 200).astype(np.float64)
    for keep in ('first', 'central'):
        assert np.array_equal(choose_kept(root, keep, a2), G.choose_kept(root, keep, a2))
    for bad in (dict(keep='last'), dict(keep='central'), dict(keep='central', a2=np.zeros(3))):
        with pytest.raises(ValueError):
            choose_kept(root, **bad)


def _synthetic():
    """12 rows in clusters 0 and 1: groups {0, 3, 4, 9} and {2, 5} in cluster 0, {6, 7, 8} in cluster 1; 1, 10 and 11 alone"""
    lab = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 1], np.int64)
    edges = {(3, 0): 0.91, (4, 3): 0.95, (9, 4): 0.97, (9, 0): 0.93, (5, 2): 0.99, (7, 6): 0.92, (8, 6): 0.94}
    offsets, pair_j = _csr(12, list(edges))
    rows = np.repeat(np.arange(12), np.diff(offsets))
    pair_cos = np.array([edges[int(i), int(j)] for i, j in zip(rows, pair_j)])
    best, partner = np.full(12, -np.inf), np.full(12, -1, np.int64)
    best[[1, 2, 6, 10, 11]] = [0.1, 0.2, -np.inf, 0.3, 0.4]
    partner[[1, 2, 10, 11]] = [0, 1, 6, 10]
    for i in np.unique(rows):
        at = slice(offsets[i], offsets[i + 1])
        best[i], partner[i] = pair_cos[at].max(), pair_j[at][np.argmax(pair_cos[at])]
    return lab, offsets, pair_j, pair_cos, best, partner


def test_summarise_groups_and_pair_similarity():
    from acav100m_amd.clustering.dedup import choose_kept, components, pair_similarity, summarise, summarise_groups
    lab, offsets, pair_j, pair_cos, best, partner = _synthetic()
    root = components(12, offsets, pair_j)
    assert root.tolist() == [0, 1, 2, 0, 0, 2, 6, 6, 6, 0, 10, 11]
    sim = pair_similarity(12, offsets, pair_j, pair_cos)
    assert sim.tolist() == [0.93, -np.inf, 0.99, 0.95, 0.97, 0.99, 0.94, 0.92, 0.94, 0.97, -np.inf, -np.inf]
    kept = choose_kept(root, 'first')
    report = summarise_groups(best, partner, lab, 2, 0.9, offsets, root, kept)
    base = summarise(best, partner, lab, 2, 0.9)
    assert {key: report[key] for key in base} == base and list(report)[:len(base)] == list(base)
    assert list(report)[len(base):] == ['pairs', 'groups', 'removed', 'removed_beyond_nearest_rule', 'group_size_counts',
                                         'largest_groups', 'keep']
    assert (report['pairs'], report['groups'], report['removed'], report['removed_beyond_nearest_rule']) == (7, 3, 6, 0)
    assert dict(report['group_size_counts']) == {'2': 1, '3-4': 2} and list(report['group_size_counts']) == ['2', '3-4']
    assert [dict(g) for g in report['largest_groups']] == [dict(size=4, cluster=0, kept=0), dict(size=3, cluster=1, kept=6),
                                                           dict(size=2, cluster=0, kept=2)]
    assert report['keep'] == 'first' and report['flagged'] == 6
    # central: the roots 0 and 6 go, rows the nearest rule does not flag
    a2 = np.array([9.0, 1, 1, 2, 3, 1, 5, 4, 4, 2, 1, 1])
    central = choose_kept(root, 'central', a2)
    assert np.flatnonzero(~central).tolist() == [0, 4, 5, 6, 8, 9]
    report = summarise_groups(best, partner, lab, 2, 0.9, offsets, root, central, 'central')
    assert (report['removed'], report['removed_beyond_nearest_rule'], report['keep']) == (6, 2, 'central')
    assert [g['kept'] for g in report['largest_groups']] == [3, 7, 2]
    big = np.zeros(40, np.int64)  # one group of 33 and one of 5 ... 8: the bins in between are stated, at 0
    big[33:38], big[38:] = 33, [38, 39]
    counts = summarise_groups(np.full(40, -np.inf), np.full(40, -1), np.zeros(40, np.int64), 1, 0.9, np.zeros(41, np.int64), big,
                              choose_kept(big, 'first'))['group_size_counts']
    assert list(counts.items()) == [('2', 0), ('3-4', 0), ('5-8', 1), ('9-16', 0), ('17-32', 0), ('33-64', 1)]
    for bad_kept in (np.ones(12, bool), np.zeros(12, bool)):
        with pytest.raises(ValueError, match="kept"):
            summarise_groups(best, partner, lab, 2, 0.9, offsets, root, bad_kept)


def test_the_csv_writers_and_the_exclude_reader(tmp_path):
    from acav100m_amd.clustering.dedup import _write_groups_csv, _write_removed_csv, choose_kept, components, pair_similarity
    from acav100m_amd.subset_selection import exclude
    _lab, offsets, pair_j, pair_cos, _best, _partner = _synthetic()
    root = components(12, offsets, pair_j)
    names = (["s%d" % (i // 5) for i in range(12)], ["clip%02d.mp4" % i for i in range(12)])
    sim = pair_similarity(12, offsets, pair_j, pair_cos)
    a2 = np.array([9.0, 1, 1, 2, 3, 1, 5, 4, 4, 2, 1, 1])
    for keep, removed, kept_of in (('first', [3, 4, 5, 7, 8, 9], {0: 0, 2: 2, 6: 6}), ('central', [0, 4, 5, 6, 8, 9], {0: 3, 2: 2, 6: 7})):
        kept = choose_kept(root, keep, a2)
        out = _write_removed_csv(tmp_path / keep / "dups.csv", root, kept, sim, names)
        lines = list(csv.reader(open(out, newline='')))
        size = {0: 4, 2: 2, 6: 3}
        assert lines == [[names[0][i], names[1][i], names[0][kept_of[root[i]]], names[1][kept_of[root[i]]], repr(float(sim[i])),
                          str(size[root[i]])] for i in removed]
        assert exclude.read_exclude(out) == {(names[0][i], "clip%02d" % i) for i in removed}  # its first two columns
        groups = _write_groups_csv(tmp_path / keep / "groups.csv", root, kept, names)
        lines = list(csv.reader(open(groups, newline='')))
        members = [0, 3, 4, 9, 2, 5, 6, 7, 8]  # by group, then by row
        assert lines == [[str(root[i]), str(size[root[i]]), str(int(kept[i])), names[0][i], names[1][i]] for i in members]
        assert sum(int(ln[2]) for ln in lines) == 3
    _write_removed_csv(tmp_path / "first" / "dups.csv", np.arange(12), np.ones(12, bool), sim, names)  # overwritten, not appended to
    assert open(tmp_path / "first" / "dups.csv").read() == ""
