"""CPU: the numpy restatement of the duplicate groups (tests/_dupgroups_np.py) against an all-pairs brute force with a breadth-
first search; the a / b / c example of order dependence; the rows the nearest-earlier rule flags are among the removed ones;
the groups as sets of rows do not depend on the order of the rows; and the figures the GPU tests rely on."""
import numpy as np
import pytest

from tests import _dupgroups_np as G
from tests import _neardup_np as R


def _rows(seed, n, d, k, copies=0, interleaved=False):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, d).astype(np.float32)
    lab = (np.arange(n) % k if interleaved else rs.randint(0, k, n)).astype(np.int64)
    for _ in range(copies):  # a later row becomes a bitwise copy of an earlier one, in its cluster
        s, t = np.sort(rs.choice(n, 2, replace=False))
        x[t], lab[t] = x[s], lab[s]
    return x, lab


def _brute(x, labels, t):
    """every pair by the three-line definition, and the components by breadth-first search"""
    x64, n = np.asarray(x, np.float64), len(labels)
    cos = lambda i, j: (x64[i] @ x64[j]) / np.sqrt((x64[i] @ x64[i]) * (x64[j] @ x64[j]))  # noqa: E731
    earlier = [[j for j in range(i) if labels[j] == labels[i] and x64[i].any() and x64[j].any() and cos(i, j) >= t] for i in range(n)]
    adj = [set(e) for e in earlier]
    for i, e in enumerate(earlier):
        for j in e:
            adj[j].add(i)
    root = np.full(n, -1, np.int64)
    for s in range(n):
        if root[s] < 0:
            root[s], queue = s, [s]
            while queue:
                for v in adj[queue.pop()]:
                    if root[v] < 0:
                        root[v] = s
                        queue.append(v)
    return earlier, root


@pytest.mark.parametrize("n,d,k,t", [(60, 5, 3, 0.3), (80, 3, 2, 0.6), (40, 9, 1, 0.1)])
def test_the_restatement_against_brute_force_and_bfs(n, d, k, t):
    x, lab = _rows(n, n, d, k, copies=4)
    x[[7, 19]] = 0.0  # zero rows: no pairs, in none
    offsets, pair_j, pair_cos, margin = G.pairs(x, lab, t)
    assert margin > 4 * R.bound(d)
    earlier, root = _brute(x, lab, t)
    assert [list(pair_j[offsets[i]:offsets[i + 1]]) for i in range(n)] == earlier
    assert offsets[n] == len(pair_j) == len(pair_cos) > 0 and (pair_cos >= t).all()
    assert offsets[8] == offsets[7] and offsets[20] == offsets[19] and not np.isin(pair_j, [7, 19]).any()
    assert np.array_equal(G.components(n, offsets, pair_j), root)
    kept = G.choose_kept(root, 'first')
    assert np.array_equal(kept, root == np.arange(n))
    a2 = np.random.RandomState(1).rand(n)
    central = G.choose_kept(root, 'central', a2)
    for g in np.unique(root):
        members = np.flatnonzero(root == g)
        assert central[members].sum() == 1 and a2[members[central[members]][0]] == a2[members].min()


def _abc():
    deg = np.deg2rad([0.0, 50.0, 25.0])  # a, b, c: c lies between a and b
    return np.stack([np.cos(deg), np.sin(deg)], 1).astype(np.float32), np.cos(np.deg2rad(30.0))


def test_the_a_b_c_example_the_nearest_rule_depends_on_the_order_the_groups_do_not():
    x, t = _abc()
    lab = np.zeros(3, np.int64)
    for order, flagged_want in (([0, 1, 2], [False, False, True]), ([2, 0, 1], [False, True, True])):  # a b c; c a b
        best, _partner, _ = R.nearest_earlier(x[order], lab)
        assert list(best >= t) == flagged_want
        offsets, pair_j, _cos, margin = G.pairs(x[order], lab, t)
        assert margin > 1e-3 and offsets[3] == 2
        root = G.components(3, offsets, pair_j)
        assert list(root) == [0, 0, 0] and list(G.choose_kept(root, 'first')) == [True, False, False]


SHAPES = [  # (n, d, k, interleaved, copies, t) -> pairs, groups, largest group, removed, flagged by the nearest rule
    ((600, 24, 4, True, 12, 0.5), (241, 97, 19, 229, 188)),
    ((2000, 70, 6, False, 20, 0.3), (1847, 90, 271, 1600, 1072)),
]


@pytest.mark.parametrize("shape,want", SHAPES, ids=["n600", "n2000"])
def test_the_flagged_rows_are_removed_and_the_groups_ignore_the_row_order(shape, want):
    n, d, k, inter, copies, t = shape
    x, lab = _rows(n + d, n, d, k, copies, inter)
    offsets, pair_j, _cos, margin = G.pairs(x, lab, t)
    assert margin > 4 * R.bound(d)
    root = G.components(n, offsets, pair_j)
    kept = G.choose_kept(root, 'first')
    best, _partner, _ = R.nearest_earlier(x, lab, k)
    flagged = best >= t
    assert not (flagged & kept).any()  # flagged by the nearest rule: among the removed
    size = np.bincount(root, minlength=n)
    assert (int(offsets[n]), int((size >= 2).sum()), int(size.max()), int((~kept).sum()), int(flagged.sum())) == want
    order = np.random.RandomState(3).permutation(n)
    off_p, pj_p, _c, _m = G.pairs(x[order], lab[order], t)
    assert off_p[n] == offsets[n]  # the same graph
    sets_p = {frozenset(int(order[i]) for i in s) for s in G.groups_as_sets(G.components(n, off_p, pj_p))}
    assert sets_p == G.groups_as_sets(root)
    best_p, _pp, _ = R.nearest_earlier(x[order], lab[order], k)
    assert int((best_p >= t).sum()) <= want[3]  # the nearest rule never removes more than the groups do
