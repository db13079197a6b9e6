"""numpy restatement of the row normalisation (acav_rows_normalize, include/acav_hip.h) and of spherical Lloyd k-means as the
clustering stage defines them (acav100m_amd/clustering/normalize.py, lloyd.py), written from the definitions and sharing no code
with the package:

  sumsq      256 float64 chains, chain q = the exact squares of the columns j = q, q + 256, ... in ascending order from +0.0;
             p_l = (c[4l] + c[4l+1]) + (c[4l+2] + c[4l+3]) for l = 0 .. 63; six butterfly steps p_l += p_{l xor m}, m = 1 .. 32
  normalize  norm = sqrt(ss), y_j = float32(float64(x_j) / norm); ss == 0: the row stays as it is and is counted
  spherical  tests/_lloyd_np.py's iteration on the normalised rows, with the centre table normalised after every update, and a
             cluster whose fp32 mean is the zero vector emptied in front of the empty-cluster rule"""
import numpy as np

from tests import _lloyd_np as L

CHAINS = 256


def sumsq(x):
    """x [n, d] or [d] fp32 -> float64 [n] (or a scalar): the stated chain, fold and butterfly order"""
    x = np.asarray(x, np.float32)
    one = x.ndim == 1
    x2 = x.reshape(1, -1) if one else x
    n, d = x2.shape
    blocks = -(-d // CHAINS)
    sq = np.zeros((n, blocks * CHAINS), np.float64)
    xd = x2.astype(np.float64)
    sq[:, :d] = xd * xd  # exact: 24-bit factors
    sq = sq.reshape(n, blocks, CHAINS)
    c = np.zeros((n, CHAINS), np.float64)
    for b in range(blocks):
        c = c + sq[:, b]
    p = (c[:, 0::4] + c[:, 1::4]) + (c[:, 2::4] + c[:, 3::4])
    lanes = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        p = p + p[:, lanes ^ m]
    assert (p == p[:, :1]).all() or not np.isfinite(p).all()
    return p[0, 0] if one else p[:, 0].copy()


def normalize(x):
    """-> (y fp32 [n, d], zero_rows); a row that is not finite is an error here as in the package's wrapper"""
    x = np.ascontiguousarray(x, np.float32)
    ss = sumsq(x)
    if not np.isfinite(ss).all():
        raise ValueError("a row is not finite")
    y = x.copy()
    ok = ss != 0
    with np.errstate(under='ignore'):
        y[ok] = (x[ok].astype(np.float64) / np.sqrt(ss[ok])[:, None]).astype(np.float32)
    return y, int((~ok).sum())


def spherical_update(x, labels, k, s):
    """-> (unit centers fp32, sizes after the splits, splits)"""
    sums, counts = L.sums_counts(x, labels, k, s)
    counts = np.array(counts, np.int64)
    centers = np.zeros(sums.shape, np.float32)
    ne = counts > 0
    centers[ne] = np.float32(sums[ne].astype(np.float64) * 2.0 ** -s / counts[ne, None])
    counts[~centers.any(axis=1)] = 0  # a mean that is the zero vector: the cluster counts as empty
    splits = L.split_empty(centers, counts)
    centers, zero = normalize(centers)
    assert zero == 0
    return centers, counts, splits


def spherical_loop(x, centers0, iters):
    """x: the rows ALREADY normalised; centers0: rows of x.  -> list per iteration of dict(labels, centers, sizes, splits,
    changed); stops after an iteration that changes no label"""
    x = np.ascontiguousarray(x, np.float32)
    n, k = len(x), len(centers0)
    s = L.shift_of(np.abs(x).max(), n)
    out, centers, prev = [], np.array(centers0, np.float32), None
    for _t in range(iters):
        labels = L.nearest(x, centers)
        changed = n if prev is None else int((labels != prev).sum())
        centers, sizes, splits = spherical_update(x, labels, k, s)
        out.append(dict(labels=labels, centers=centers.copy(), sizes=sizes, splits=splits, changed=changed))
        prev = labels
        if changed == 0:
            break
    return out
