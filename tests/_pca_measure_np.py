"""numpy restatement of the PCA selection measures (acav_pair_scores, acav_rank_desc, PCAOptim.run), written from the
definition: every operation an individually rounded fp32 operation (numpy's fp32 + - * / sqrt are correctly rounded, so the
GPU must agree bit for bit), every sum over the columns ONE chain from +0 with j ascending, the pairs added in pair order
starting AT the first distance, one division by float(P).  Plus a float64 version of every distance (the error-bound tests)."""
import itertools

import numpy as np

DISTANCES = ('inner_product', 'cosine_similarity', 'euclidean_diff_l1', 'euclidean_diff_l2')
EPS = np.float32(1e-8)
F = np.float32


def _chain(terms):
    """terms [V, p] fp32 -> [V]: ((0 + t_0) + t_1) + ... one fp32 addition at a time (vectorised over the clips)"""
    acc = np.zeros(terms.shape[0], F)
    for j in range(terms.shape[1]):
        acc = (acc + terms[:, j]).astype(F)
    return acc


def distance32(a, b, kind):
    """a, b [V, p] fp32 -> [V] fp32"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if kind == 'inner_product':
        return _chain((a * b).astype(F))
    if kind == 'cosine_similarity':
        dot = _chain((a * b).astype(F))
        na = np.maximum(np.sqrt(_chain((a * a).astype(F))).astype(F), EPS)
        nb = np.maximum(np.sqrt(_chain((b * b).astype(F))).astype(F), EPS)
        return (dot / (na * nb).astype(F)).astype(F)
    e = (a - b).astype(F)
    if kind == 'euclidean_diff_l1':
        return -_chain(np.abs(e))
    if kind == 'euclidean_diff_l2':
        return -_chain((e * e).astype(F))
    raise ValueError(kind)


def scores32(views, pairs, kind):
    """views: list of [V, p] fp32; pairs: [(c1, c2)] -> [V] fp32"""
    total = None
    for c1, c2 in pairs:
        d = distance32(views[c1], views[c2], kind)
        total = d if total is None else (total + d).astype(F)
    return (total / F(len(pairs))).astype(F)


def distance64(a, b, kind):
    """-> (distance [V] f64 in exact-ish float64 arithmetic, mass [V] f64 = sum_j |term_j| of the chain(s))"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if kind == 'inner_product':
        return (a * b).sum(1), np.abs(a * b).sum(1)
    if kind == 'cosine_similarity':
        na = np.maximum(np.sqrt((a * a).sum(1)), 1e-8)
        nb = np.maximum(np.sqrt((b * b).sum(1)), 1e-8)
        return (a * b).sum(1) / (na * nb), np.abs(a * b).sum(1) / (na * nb)
    if kind == 'euclidean_diff_l1':
        return -np.abs(a - b).sum(1), np.abs(a - b).sum(1)
    if kind == 'euclidean_diff_l2':
        return -((a - b) ** 2).sum(1), ((a - b) ** 2).sum(1)
    raise ValueError(kind)


def scores64(views, pairs, kind):
    """-> (score [V] f64, mass [V] f64 = (sum_pairs sum_j |term_j|) / P)"""
    s = m = 0.0
    for c1, c2 in pairs:
        d, mass = distance64(views[c1], views[c2], kind)
        s, m = s + d, m + mass
    return s / len(pairs), m / len(pairs)


def rank_desc(scores, k):
    """the k clips of largest score, descending by VALUE (-0.0 == +0.0), ties to the lower index; a score that is not finite
    raises"""
    scores = np.asarray(scores, F)
    if not np.isfinite(scores).all():
        raise ValueError("a score is not finite")
    value = scores + F(0)  # -0 + +0 = +0: one value for both zeros
    order = np.lexsort((np.arange(len(scores)), -value.astype(np.float64)))  # last key first: value descending, then index
    return order[:k].astype(np.int64)


def gain(scores, ids):
    top = [float(scores[i]) for i in ids]
    return [top[j] if j == 0 else top[j] + top[j - 1] for j in range(len(top))]


def run(views, pairs, kind, k):
    """-> (S, GAIN, LOOKUPS)"""
    s = scores32(views, pairs, kind)
    ids = rank_desc(s, k)
    return [int(i) for i in ids], gain(s, ids), [0] * len(ids)


def combination(D):
    return list(itertools.combinations(range(D), 2))


def bipartite(D):
    """the first half of the views against the second"""
    h = D // 2
    return list(itertools.product(range(h), range(h, D)))


def diagonal(D):
    h = D // 2
    return [(i, h + i) for i in range(h)]


def gamma(m):
    u = 2.0 ** -24
    return m * u / (1 - m * u)
