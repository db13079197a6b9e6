"""The numpy restatement of the duplicate groups (include/acav_hip.h: acav_rows_neardup_pairs, acav_pairs_components;
clustering/dedup.py: pairs_earlier, components, choose_kept).

Pairs: per cluster the cosines of tests/_neardup_np.py (strict lower triangle: the earlier rows of the cluster, zero rows out),
every entry >= t is a pair, listed at its later row in ascending earlier row -- the CSR layout of the entry point.  Groups: a
plain union-find over those pairs, the lowest row of a component its root."""
import numpy as np

from tests import _neardup_np as R


def pairs(x, labels, t):
    """(offsets int64 [n + 1], pair_j int64 [P], pair_cos float64 [P], margin): margin = the smallest |cos - t| over every
    cosine the definition compares (inf when there is none) -- what a test needs to show that every pair is decided"""
    x, labels = np.asarray(x, np.float32), np.asarray(labels, np.int64)
    n = len(labels)
    js, cs = [np.empty(0, np.int64)] * n, [np.empty(0)] * n
    margin = np.inf
    for c in np.unique(labels):
        idx = np.flatnonzero(labels == c)  # ascending input position
        cos = R.cluster_cosines(x[idx])
        live = np.isfinite(cos)
        if live.any():
            margin = min(margin, float(np.abs(cos[live] - t).min()))
        for r in np.flatnonzero((cos >= t).any(1)):
            hit = np.flatnonzero(cos[r] >= t)
            js[idx[r]], cs[idx[r]] = idx[hit], cos[r, hit]
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([len(j) for j in js])
    return offsets, np.concatenate(js) if n else np.empty(0, np.int64), np.concatenate(cs) if n else np.empty(0), margin


def components(n, offsets, pair_j):
    """root int64 [n]: the lowest row of every row's component"""
    up = list(range(n))

    def find(a):
        while up[a] != a:
            a = up[a]
        return a

    for i in range(n):
        for e in range(int(offsets[i]), int(offsets[i + 1])):
            a, b = find(i), find(int(pair_j[e]))
            if a != b:
                up[max(a, b)] = min(a, b)
        up[i] = find(i)  # a row's own path stays short
    return np.array([find(i) for i in range(n)], np.int64)


def choose_kept(root, keep, a2=None):
    """kept bool [n]: every row outside the groups and one row per group -- 'first': the root; 'central': the member with the
    smallest a2, the lower row on a tie"""
    root = np.asarray(root, np.int64)
    kept = np.zeros(len(root), bool)
    for g in np.unique(root):
        members = np.flatnonzero(root == g)  # ascending
        kept[g if keep == 'first' else members[np.argmin(np.asarray(a2, np.float64)[members])]] = True  # argmin: the first
    return kept


def groups_as_sets(root):
    """the groups of two rows or more as a set of frozensets of rows"""
    root = np.asarray(root, np.int64)
    return {frozenset(np.flatnonzero(root == g).tolist()) for g in np.unique(root) if (root == g).sum() >= 2}
