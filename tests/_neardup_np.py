"""The numpy restatement of acav_rows_neardup (include/acav_hip.h, clustering/dedup.py) and its error bound.

Per cluster: G = X64 @ X64.T, cos = G / sqrt(outer(diag G, diag G)), for every row the maximum over the strict lower triangle
(the earlier rows of the cluster, in input order), the lowest argmax on ties; a zero row has no partner and is none."""
import numpy as np


def gamma(m):
    u = 2.0 ** -53
    return m * u / (1.0 - m * u)


def bound(d):
    """|cos_computed - cos| of the kernel: gamma_{d + 4 ceil(d / 64) + 30} (the derivation is in include/acav_hip.h)"""
    return gamma(d + 4 * ((d + 63) // 64) + 30)


def cluster_cosines(x):
    """float64 [m, m] cosines of the rows of one cluster, the upper triangle and the diagonal at -inf, and so are the columns of
    zero rows and the rows of zero rows"""
    x64 = np.asarray(x, np.float64)
    G = x64 @ x64.T
    nrm = np.diag(G).copy()
    with np.errstate(invalid='ignore', divide='ignore'):
        cos = G / np.sqrt(np.outer(nrm, nrm))
    m = len(nrm)
    dead = np.triu(np.ones((m, m), bool)) | (nrm == 0)[None, :] | (nrm == 0)[:, None]
    cos[dead] = -np.inf
    return cos


def nearest_earlier(x, labels, k=None):
    """(best float64 [n], partner int64 [n], second float64 [n]): second = the largest cosine to an earlier row of the cluster
    other than the partner and its bitwise copies (-inf when there is none) -- what the tests need to show that a partner is
    decided"""
    x, labels = np.asarray(x, np.float32), np.asarray(labels, np.int64)
    n = len(labels)
    best, partner, second = np.full(n, -np.inf), np.full(n, -1, np.int64), np.full(n, -np.inf)
    for c in np.unique(labels):
        idx = np.flatnonzero(labels == c)  # ascending input position
        cos = cluster_cosines(x[idx])
        arg = cos.argmax(1)  # numpy's argmax: the first, hence the lowest position
        # bitwise copies of that row tie exactly in the definition (the same values through the same chain give the same bytes)
        # and the lowest position keeps the tie; a BLAS product may differ in the last bit between them, so the lowest copy
        # among the row's columns is named here, not left to the rounding of G
        same = np.unique(x[idx], axis=0, return_inverse=True)[1].reshape(-1)
        copies = (same[None, :] == same[arg][:, None])
        arg = (copies & np.isfinite(cos)).argmax(1)
        top = cos[np.arange(len(idx)), arg]
        has = np.isfinite(top)
        best[idx[has]] = top[has]
        partner[idx[has]] = idx[arg[has]]
        second[idx] = np.where(copies, -np.inf, cos).max(1)  # the runner-up: the partner's copies are no rivals
    return best, partner, second


def brute_force(x, labels):
    """the three-line statement over all pairs, in float64"""
    x64, n = np.asarray(x, np.float64), len(labels)
    cos = lambda i, j: (x64[i] @ x64[j]) / np.sqrt((x64[i] @ x64[i]) * (x64[j] @ x64[j]))  # noqa: E731
    E = [[j for j in range(i) if labels[j] == labels[i] and x64[j].any() and x64[i].any()] for i in range(n)]
    pairs = [max(((cos(i, j), -j) for j in e), default=(-np.inf, 1)) for i, e in enumerate(E)]
    return np.array([p[0] for p in pairs]), np.array([-p[1] for p in pairs], np.int64)
