"""The numpy restatement of acav_rows_crossdup (include/acav_hip.h, clustering/dedup.py: nearest_in) and its error bound.

Per label: cos = X64 @ Y64.T / sqrt(outer(||x||^2, ||y||^2)), for every pool row the maximum over the held-out rows of its label,
the lowest argmax on ties; a zero row of y is never a partner, a zero row of x has none."""
import numpy as np

from tests import _neardup_np

bound = _neardup_np.bound  # the rounding operations are acav_rows_neardup's


def label_cosines(x, y):
    """float64 [nx, ny] cosines of the pool rows x and the held-out rows y of one label; the columns of zero rows of y and the
    rows of zero rows of x at -inf"""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx, ny = (x64 * x64).sum(1), (y64 * y64).sum(1)
    with np.errstate(invalid='ignore', divide='ignore'):
        cos = (x64 @ y64.T) / np.sqrt(np.outer(nx, ny))
    cos[(nx == 0)[:, None] | (ny == 0)[None, :]] = -np.inf
    return cos


def nearest_in(x, y, labels_x=None, labels_y=None):
    """(best float64 [n], partner int64 [n], second float64 [n]): second = the largest cosine to a held-out row of the label
    other than the partner and its bitwise copies among y (-inf when there is none) -- what the tests need to show that a
    partner is decided.  labels None: every pair"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    n, m = len(x), len(y)
    lx = np.zeros(n, np.int64) if labels_x is None else np.asarray(labels_x, np.int64)
    ly = np.zeros(m, np.int64) if labels_y is None else np.asarray(labels_y, np.int64)
    best, partner, second = np.full(n, -np.inf), np.full(n, -1, np.int64), np.full(n, -np.inf)
    for c in np.unique(lx):
        ix, iy = np.flatnonzero(lx == c), np.flatnonzero(ly == c)  # ascending input position
        if not len(iy):
            continue
        cos = label_cosines(x[ix], y[iy])
        arg = cos.argmax(1)
        # bitwise copies of the partner among y tie exactly in the definition and the lowest position keeps the tie; a BLAS
        # product may differ in the last bit between them, so the lowest copy is named here, not left to the rounding
        same = np.unique(y[iy], axis=0, return_inverse=True)[1].reshape(-1)
        copies = same[None, :] == same[arg][:, None]
        arg = (copies & np.isfinite(cos)).argmax(1)
        top = cos[np.arange(len(ix)), arg]
        has = np.isfinite(top)
        best[ix[has]] = top[has]
        partner[ix[has]] = iy[arg[has]]
        second[ix] = np.where(copies, -np.inf, cos).max(1)  # the runner-up: the partner's copies are no rivals
    return best, partner, second


def brute_force(x, y, labels_x, labels_y):
    """the three-line statement over all pairs, in float64"""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    cos = lambda a, b: (a @ b) / np.sqrt((a @ a) * (b @ b))  # noqa: E731
    E = [[j for j in range(len(y64)) if labels_y[j] == labels_x[i] and y64[j].any() and x64[i].any()] for i in range(len(x64))]
    pairs = [max(((cos(x64[i], y64[j]), -j) for j in e), default=(-np.inf, 1)) for i, e in enumerate(E)]
    return np.array([p[0] for p in pairs]), np.array([-p[1] for p in pairs], np.int64)
