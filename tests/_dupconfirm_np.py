"""The numpy restatement of the confirmation in a second view (include/acav_hip.h: acav_pairs_cosine; clustering/dedup.py:
pair_cosines, confirm_pairs, `dedup --dedup.confirm_view=`).

With view A = the view the pairs are found in at threshold t, view B = the confirming view and cosB the cosine of B's rows:
  P_i' = { j in P_i : cosB(i, j) >= t2 }
Roots, groups, kept and similarity are tests/_dupgroups_np.py's definitions over P' in place of P; similarity stays a cosine of
view A, the largest among a row's confirmed pairs."""
import numpy as np

from tests import _dupgroups_np as G


def pair_cos(x, i, j):
    """float64 [P]: the cosines of the listed pairs (i[e], j[e]) of x, -inf where either row is all zero"""
    x64 = np.asarray(x, np.float64)
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    dot = (x64[i] * x64[j]).sum(1)
    nrm = (x64 * x64).sum(1)
    with np.errstate(invalid='ignore', divide='ignore'):
        cos = dot / np.sqrt(nrm[i] * nrm[j])
    cos[(nrm[i] == 0) | (nrm[j] == 0)] = -np.inf
    return cos


def confirmed(xa, xb, labels, t, t2):
    """(offsets int64 [n + 1], pair_j int64 [P'], pair_cos float64 [P'] of view A, cos_b float64 [P] of ALL of A's pairs,
    margin, margin_b): _dupgroups_np.pairs on view A, then the filter cosB >= t2.  margin: pairs'; margin_b: the smallest
    |cosB - t2| over A's pairs (inf without any) -- what a test needs to show that every pair is decided in both views"""
    offsets, pair_j, cos_a, margin = G.pairs(xa, labels, t)
    n = len(offsets) - 1
    later = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    cos_b = pair_cos(xb, later, pair_j)
    live = np.isfinite(cos_b)
    margin_b = float(np.abs(cos_b[live] - t2).min()) if live.any() else np.inf
    keep = cos_b >= t2
    out = np.zeros(n + 1, np.int64)
    out[1:] = np.cumsum(np.bincount(later[keep], minlength=n))
    return out, pair_j[keep], cos_a[keep], cos_b, margin, margin_b
