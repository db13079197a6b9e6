"""The numpy restatements of acav_kmeans_probes and acav_rows_probedup (include/acav_hip.h; KMeans.probe_centers and
clustering/dedup.py: nearest_earlier / nearest_in with probes), their error bounds, and the brute force over all pairs.

Probes: D = (||x||^2 + ||c||^2) - 2 x.c in float64, clamped at 0; slot 0 the label, then the other centres by ascending D, ties to
the lower index.  Pairs: per probed cluster the cosines of the rows that probe it against the rows of y it holds, cut at
before[i]; per row the best of every slot, then the best slot, the lowest position on ties."""
import numpy as np

from tests import _crossdup_np, _neardup_np

gamma = _neardup_np.gamma
bound = _neardup_np.bound  # |cos_computed - cos|: the rounding operations are acav_rows_neardup's


def dist_bound(x, centres):
    """[n, K]: |D_computed - D| <= 2 gamma_{d+2} (||x_i||^2 + ||c||^2), acav_kmeans_quality's bound for a2"""
    x64, c64 = np.asarray(x, np.float64), np.asarray(centres, np.float64)
    return 2.0 * gamma(x64.shape[1] + 2) * ((x64 * x64).sum(1)[:, None] + (c64 * c64).sum(1)[None, :])


def distances(x, centres):
    """float64 [n, K]; bitwise-equal centres get one column's values (a BLAS product may differ in the last bit between them,
    the kernel's chains do not)"""
    x64 = np.asarray(x, np.float64)
    cu, inv = np.unique(np.asarray(centres, np.float32), axis=0, return_inverse=True)
    c64 = cu.astype(np.float64)
    D = ((x64 * x64).sum(1)[:, None] + (c64 * c64).sum(1)[None, :]) - 2.0 * (x64 @ c64.T)
    return np.maximum(D, 0.0)[:, inv.reshape(-1)]


def probe_centers(x, centres, labels, m):
    """(probes int64 [n, m], dist float64 [n, m], gap float64 [n, m - 1], room float64 [n, m - 1]).  gap[:, r]: the distance
    between the other centres ranked r + 1 and r + 2 (the last one: between the last listed centre and the first one left out;
    +inf where there is no such centre, and between bitwise-equal centres, which tie exactly); room[:, r]: the two error bounds
    of that pair summed -- a rank is decided when gap > 4 room"""
    labels = np.asarray(labels, np.int64)
    n, K = len(labels), len(centres)
    D, B = distances(x, centres), dist_bound(x, centres)
    rows = np.arange(n)
    others = D.copy()
    others[rows, labels] = np.inf
    order = np.argsort(others, axis=1, kind='stable')  # ties: the lower index first
    probes, dist = np.full((n, m), -1, np.int64), np.full((n, m), np.inf)
    probes[:, 0], dist[:, 0] = labels, D[rows, labels]
    have = min(m - 1, K - 1)
    probes[:, 1:1 + have] = order[:, :have]
    dist[:, 1:1 + have] = np.take_along_axis(D, order[:, :have], 1)
    gap, room = np.full((n, max(m - 1, 0)), np.inf), np.zeros((n, max(m - 1, 0)))
    cu_inv = np.unique(np.asarray(centres, np.float32), axis=0, return_inverse=True)[1].reshape(-1)
    for r in range(min(m - 1, K - 2)):  # the ranks r + 1 and r + 2 among the K - 1 others
        a, b = order[:, r], order[:, r + 1]
        gap[:, r] = np.where(cu_inv[a] == cu_inv[b], np.inf, D[rows, b] - D[rows, a])
        room[:, r] = B[rows, a] + B[rows, b]
    return probes, dist, gap, room


def _counted(probes):
    """bool [n, m]: the slots that count -- not -1, not a label repeated in the row's list"""
    counts = probes >= 0
    for p in range(1, probes.shape[1]):
        counts[:, p] &= ~(probes[:, :p] == probes[:, p:p + 1]).any(1)
    return counts


def nearest(x, y, probes, labels_y, before=None):
    """(best float64 [n], partner int64 [n], second float64 [n], best_each float64 [n, m]); second = the largest cosine to a
    candidate of any probed cluster other than the partner and its bitwise copies among y (-inf when there is none)"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    probes, ly = np.asarray(probes, np.int64), np.asarray(labels_y, np.int64)
    n, m = probes.shape
    counts = _counted(probes)
    same = np.unique(y, axis=0, return_inverse=True)[1].reshape(-1)  # bitwise copies among y share a number
    cut = np.full(n, len(y), np.int64) if before is None else np.asarray(before, np.int64)
    each, arg = np.full((n, m), -np.inf), np.full((n, m), -1, np.int64)

    def block(c):
        """the rows that probe c with their slots, the rows of y it holds, and the cosines, -inf where cut"""
        ix, slot = np.nonzero((probes == c) & counts)
        iy = np.flatnonzero(ly == c)
        if not len(ix) or not len(iy):
            return None
        cos = _crossdup_np.label_cosines(x[ix], y[iy])
        cos[iy[None, :] >= cut[ix][:, None]] = -np.inf
        return ix, slot, iy, cos

    clusters = np.unique(probes[counts])
    for c in clusters:
        got = block(c)
        if got is None:
            continue
        ix, slot, iy, cos = got
        top = cos.argmax(1)
        copies = (same[iy][None, :] == same[iy[top]][:, None]) & np.isfinite(cos)  # they tie exactly: the lowest one is named
        low = copies.argmax(1)
        has = copies.any(1)
        each[ix[has], slot[has]] = cos[np.arange(len(ix)), low][has]
        arg[ix[has], slot[has]] = iy[low[has]]
    best, partner = np.full(n, -np.inf), np.full(n, -1, np.int64)
    has = np.flatnonzero((arg >= 0).any(1))
    top = each[has].argmax(1)
    named = arg[has, top]
    tied = (arg[has] >= 0) & (same[np.maximum(arg[has], 0)] == same[named][:, None])  # the partner's copies in other probed clusters
    best[has], partner[has] = each[has, top], np.where(tied, arg[has], len(y)).min(1)
    second = np.full(n, -np.inf)
    for c in clusters:
        got = block(c)
        if got is None:
            continue
        ix, _slot, iy, cos = got
        rival = np.where(same[iy][None, :] == same[np.maximum(partner[ix], 0)][:, None], -np.inf, cos)
        np.maximum.at(second, ix, rival.max(1))
    return best, partner, second, each


def brute_force_probes(x, centres, labels, m):
    """the definition row by row: (D, index) sorted"""
    D = distances(x, centres)
    probes, dist = np.full((len(labels), m), -1, np.int64), np.full((len(labels), m), np.inf)
    for i, lab in enumerate(labels):
        ranked = sorted((D[i, c], c) for c in range(len(centres)) if c != lab)[:m - 1]
        probes[i, :1 + len(ranked)] = [lab] + [c for _, c in ranked]
        dist[i, :1 + len(ranked)] = [D[i, lab]] + [v for v, _ in ranked]
    return probes, dist


def brute_force(x, y, probes, labels_y, before=None):
    """the statement of the header over all pairs, in float64: (best, partner, best_each)"""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, m = np.shape(probes)
    cos = lambda a, b: (a @ b) / np.sqrt((a @ a) * (b @ b))  # noqa: E731
    best, partner, each = np.full(n, -np.inf), np.full(n, -1, np.int64), np.full((n, m), -np.inf)
    for i in range(n):
        for p in range(m):
            c = probes[i][p]
            if c < 0 or c in list(probes[i][:p]) or not x64[i].any():
                continue
            E = [j for j in range(len(y64)) if labels_y[j] == c and y64[j].any() and (before is None or j < before[i])]
            if E:
                each[i, p] = max(cos(x64[i], y64[j]) for j in E)
        pairs = [(cos(x64[i], y64[j]), -j) for j in range(len(y64))
                 if labels_y[j] in [c for c in probes[i] if c >= 0] and y64[j].any() and x64[i].any()
                 and (before is None or j < before[i])]
        if pairs:
            best[i], partner[i] = max(pairs)[0], -max(pairs)[1]
    return best, partner, each


def plan(probes, labels_y, before, cus):
    """the rule acav_rows_probedup_plan states, restated: (H, tiles, blocks) and the tile list [(first entry, entries, first
    column block, blocks)] by descending blocks, ties by ascending first entry"""
    probes, ly = np.asarray(probes, np.int64), np.asarray(labels_y, np.int64)
    n, m = probes.shape
    counts = _counted(probes)
    ystart = {c: int((ly < c).sum()) for c in np.unique(probes[counts])}
    entries = sorted((int(probes[i, p]), i) for i in range(n) for p in range(m) if counts[i, p])  # by cluster, then by row
    ranges = []
    for c, i in entries:
        held = np.flatnonzero(ly == c)
        r = len(held) if before is None else int((held < before[i]).sum())
        ranges.append((ystart[c], ystart[c] + r))
    E = len(entries)
    H = 128 if -(-E // 128) >= cus else 64
    tiles = []
    for q0 in range(0, E, H):
        mine = ranges[q0:q0 + H]
        full = [(lo, hi) for lo, hi in mine if hi > lo]
        if full:
            first = full[0][0] // 64
            tiles.append((q0, len(mine), first, max(-(-hi // 64) for _, hi in full) - first))
        else:
            tiles.append((q0, len(mine), mine[0][0] // 64, 0))
    blocks = sum(t[3] for t in tiles)
    return (H, len(tiles), blocks), [list(t) for t in sorted(tiles, key=lambda t: (-t[3], t[0]))]
