"""numpy restatement of batch (Lloyd) k-means as the clustering stage defines it (acav100m_amd/clustering/lloyd.py), written
from the definition and sharing no code with the package:

  scale      (m, E) = frexp(absmax), s = 62 - ceil(log2(max(N, 2))) - E: every |x 2^s| < 2^62 / N
  quantise   q = rint(float64(x) * 2^s) as int64 (numpy's rint: round half to even; the product is exact)
  sums       np.add.at(sums, labels, q), counts = bincount(labels)
  centres    float32(float64(sums) * 2^-s / counts), then the empty clusters in ascending order: the currently largest cluster j
             (lowest index on ties) is split -- c_i = c_j, even columns of c_i times 1 + 1/1024 and of c_j times 1 - 1/1024, odd
             columns the other way round, i takes floor(count_j / 2) from j
  labels     oracle.KMeans.calc_best on a discount-free state: counts = N / K each and count = N, with N >= 10 K (its warm-up is
             over and no count lies below (count / K) ** 0.7) -- the first-index argmin of the canonical fp32 distance
  loop       initial centres = the rows randperm(N)[:K]; iteration t labels with the centres of t - 1 and moves them; stops after
             an iteration that changes no label"""
import math

import numpy as np


def shift_of(absmax, n):
    _m, e = math.frexp(float(absmax))
    return 62 - int(math.ceil(math.log2(max(int(n), 2)))) - e


def quantise(x, s):
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * 2.0 ** s).astype(np.int64)


def sums_counts(x, labels, k, s):
    x = np.asarray(x, np.float32)
    sums = np.zeros((k, x.shape[1]), np.int64)
    np.add.at(sums, np.asarray(labels, np.int64), quantise(x, s))
    return sums, np.bincount(labels, minlength=k).astype(np.int64)


def split_empty(centers, counts):
    """in place -> splits"""
    up, down = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    d = centers.shape[1]
    even = np.arange(d) % 2 == 0
    splits = 0
    for i in range(len(counts)):
        if counts[i] != 0:
            continue
        best = counts.max()
        j = min(q for q in range(len(counts)) if counts[q] == best)
        ci, cj = centers[j].copy(), centers[j].copy()
        ci[even], ci[~even] = ci[even] * up, ci[~even] * down
        cj[even], cj[~even] = cj[even] * down, cj[~even] * up
        centers[i], centers[j] = ci, cj
        counts[i] = counts[j] // 2
        counts[j] = counts[j] - counts[i]
        splits += 1
    return splits


def centers_of(sums, counts, s):
    """-> (centers fp32, sizes after the splits, splits)"""
    counts = np.array(counts, np.int64)
    centers = np.zeros(sums.shape, np.float32)
    ne = counts > 0
    centers[ne] = np.float32(sums[ne].astype(np.float64) * 2.0 ** -s / counts[ne, None])
    splits = split_empty(centers, counts)
    return centers, counts, splits


def update(x, labels, k, s):
    return centers_of(*sums_counts(x, labels, k, s), s)


def nearest(x, centers):
    """first-index argmin of the canonical fp32 distance, through the oracle on a discount-free state"""
    from oracle import oracle as O
    x = np.ascontiguousarray(x, np.float32)
    k, n = len(centers), len(x)
    assert n >= 10 * k, "the oracle's warm-up must be over"
    km = O.KMeans(x.shape[1], k, O.Rng(0), centers=np.ascontiguousarray(centers, np.float32))
    km.set_state(np.ascontiguousarray(centers, np.float32), np.full(k, n / k, np.float32), n)
    return km.calc_best(x)[0]


def loop(x, centers0, iters):
    """-> list per iteration of dict(labels, centers, sizes, splits, changed); stops after an iteration that changes no label"""
    x = np.ascontiguousarray(x, np.float32)
    n, k = len(x), len(centers0)
    s = shift_of(np.abs(x).max(), n)
    out, centers, prev = [], np.array(centers0, np.float32), None
    for _t in range(iters):
        labels = nearest(x, centers)
        changed = n if prev is None else int((labels != prev).sum())
        centers, sizes, splits = update(x, labels, k, s)
        out.append(dict(labels=labels, centers=centers.copy(), sizes=sizes, splits=splits, changed=changed))
        prev = labels
        if changed == 0:
            break
    return out
