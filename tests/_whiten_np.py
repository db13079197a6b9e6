"""Float64 restatement of clustering.whiten (acav100m_amd/clustering/whiten.py) for the tests: the definition, and the
per-segment tile / Chan form the device computes its moments in."""
import numpy as np

TILE = 256  # ACAV_COLSTATS_TILE (include/acav_hip.h)


def std_of(x):
    """-> (std fp32 [d] with zeros replaced by 1, number of replaced columns): the population std in float64, rounded to fp32"""
    s = np.asarray(x, np.float32).astype(np.float64).std(0).astype(np.float32)
    zero = s == 0
    s[zero] = np.float32(1.0)
    return s, int(zero.sum())


def whiten(x):
    """-> (x / std in fp32, std, zero columns)"""
    x = np.asarray(x, np.float32)
    s, nz = std_of(x)
    return x / s, s, nz


def chan(a, b):
    """(n, mean, M2) of the rows of a followed by those of b; an empty side leaves the other"""
    (na, ma, qa), (nb, mb, qb) = a, b
    if nb == 0:
        return a
    if na == 0:
        return b
    n = na + nb
    delta = mb - ma
    return n, ma + delta * (np.float64(nb) / np.float64(n)), (qa + qb) + (delta * delta) * (np.float64(na) * np.float64(nb) / np.float64(n))


def segment_moments(x, tile=TILE):
    """(n, mean, M2) of one segment: tiles of `tile` rows from its first row, each (mean, sum (x - mean)^2) in float64, folded in
    tile order"""
    x = np.asarray(x, np.float32).astype(np.float64)
    d = x.shape[1]
    acc = (0, np.zeros(d), np.zeros(d))
    for r in range(0, x.shape[0], tile):
        t = x[r:r + tile]
        m = t.sum(0) / np.float64(len(t))
        acc = chan(acc, (len(t), m, ((t - m) ** 2).sum(0)))
    return acc


def recipe(n, d, seed):
    """the test data: randn x per-column scale (log-uniform in [1e-3, 1e3]) + per-column offset (uniform in [-5, 5]) in fp32,
    then column 0 constant 0.1f, column 2 = 1e4 + 1e-2 randn, column 4 clipped at 0, column 6 = -3e5 + 0.5 randn (where d allows)"""
    rs = np.random.RandomState(seed)
    scale = np.exp(rs.uniform(np.log(1e-3), np.log(1e3), d))
    off = rs.uniform(-5, 5, d)
    x = (rs.randn(n, d) * scale + off).astype(np.float32)
    x[:, 0] = np.float32(0.1)
    if d > 2:
        x[:, 2] = (1e4 + 1e-2 * rs.randn(n)).astype(np.float32)
    if d > 4:
        x[:, 4] = np.maximum(x[:, 4], 0)
    if d > 6:
        x[:, 6] = (-3e5 + 0.5 * rs.randn(n)).astype(np.float32)
    return x


def ulp_diff(a, b):
    """distance in fp32 ulps between two finite fp32 arrays of the same sign pattern (0 for equal bits)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)
