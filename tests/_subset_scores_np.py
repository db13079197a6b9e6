"""Pure float64 / Python-int restatement of the subset scores (include/acav_hip.h, "subset scoring") in numpy -- shared by the
golden generators (tests/golden/gen_subset_scores.py and gen_subset_scores_large.py, which record how far it is from sklearn)
and the tests.  It imports neither sklearn nor the library."""
import importlib.util
import math
import os

import numpy as np

NAMES = ('mutual_info', 'normalized_mutual_info', 'adjusted_mutual_info', 'adjusted_rand', 'fowlkes_mallows', 'rand')
EPS = float(np.finfo(np.float64).eps)
_LF = np.zeros(1)


def lf_table(kmax):
    """ln k! for k = 0 .. kmax (math.lgamma: the C library's, as the handle's host-built table)"""
    global _LF
    if len(_LF) <= kmax:
        _LF = np.array([0.0] + [math.lgamma(k + 1.0) for k in range(1, kmax + 1)])
    return _LF


def table(assign, ids, d1, d2, C):
    N = np.zeros((C, C), np.int64)
    np.add.at(N, (assign[ids, d1], assign[ids, d2]), 1)
    return N


def emi_terms(N):
    """the terms of the exact expected mutual information, one vector element per (cell, n_ij), G added in sklearn's order"""
    n = int(N.sum())
    b, a = N.sum(1), N.sum(0)
    rows, cols = np.nonzero(b)[0], np.nonzero(a)[0]
    bi = np.repeat(b[rows], len(cols)).astype(np.int64)
    aj = np.tile(a[cols], len(rows)).astype(np.int64)
    start = np.maximum(1, aj + bi - n)
    end = np.minimum(aj, bi)
    length = end - start + 1
    cell = np.repeat(np.arange(len(bi)), length)
    first = np.cumsum(length) - length
    nij = start[cell] + (np.arange(len(cell)) - first[cell])
    B, A = bi[cell], aj[cell]
    lf = lf_table(n)
    ln = np.log(np.maximum(np.arange(n + 1), 1).astype(np.float64))
    G = ((((((((lf[B] + lf[A]) + lf[n - B]) + lf[n - A]) - lf[n]) - lf[nij]) - lf[B - nij]) - lf[A - nij])
         - lf[n - B - A + nij])
    t2 = ((ln[n] + ln[nij]) - ln[B]) - ln[A]
    return ((nij / float(n)) * t2) * np.exp(G)


def emi(N):
    """exact expected mutual information: the sum of emi_terms"""
    return float(np.sum(emi_terms(N)))


def raw_stats(N, with_emi=True):
    """one pair's raw values from its contingency table: the fields of acav_score_stats"""
    n = int(N.sum())
    b, a = N.sum(1), N.sum(0)
    i, j = np.nonzero(N)
    v = N[i, j].astype(np.float64)
    ln_n = math.log(n)
    x = v / n
    t = x * (np.log(v) - ln_n) + x * ((-np.log(b[i]) - np.log(a[j])) + 2.0 * ln_n)
    t = np.where(np.abs(t) < EPS, 0.0, t)
    mi = max(float(t.sum()), 0.0)

    def entropy(m):
        m = m[m > 0].astype(np.float64)
        return float(-np.sum((m / n) * (np.log(m) - ln_n)))

    def c2(m):
        return int(sum(int(k) * (int(k) - 1) // 2 for k in np.ravel(m)))

    tp = c2(N[i, j])
    fp, fn = c2(a) - tp, c2(b) - tp
    return dict(mi=mi, h_row=entropy(b), h_col=entropy(a), emi=emi(N) if with_emi else float('nan'), tp=tp, fp=fp, fn=fn,
                tn=n * (n - 1) // 2 - tp - fp - fn, n_rows=int((b > 0).sum()), n_cols=int((a > 0).sum()), n=n)


def compose(s):
    """raw values -> the six scores, the arithmetic of the header's definition (Python floats and ints)"""
    one = s['n_rows'] == 1 and s['n_cols'] == 1
    mean_h = (s['h_row'] + s['h_col']) / 2.0
    mi = s['mi']
    nmi = 1.0 if one else 0.0 if mi == 0 else mi / max(mean_h, EPS)
    if one:
        ami = 1.0
    elif s['n_rows'] == 1 or s['n_cols'] == 1:
        ami = 0.0
    else:
        den = mean_h - s['emi']
        den = min(den, -EPS) if den < 0 else max(den, EPS)
        num = mi - s['emi']
        num = min(num, -EPS) if num < 0 else max(num, EPS)
        ami = num / den
    tp, fp, fn, tn = (int(s[k]) for k in ('tp', 'fp', 'fn', 'tn'))
    ari = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    fm = 0.0 if tp == 0 else math.sqrt(float(tp) / float(tp + fp)) * math.sqrt(float(tp) / float(tp + fn))
    all_pairs = tp + fp + fn + tn
    rand = 1.0 if all_pairs == 0 else float(tp + tn) / float(all_pairs)
    return dict(zip(NAMES, (mi, nmi, ami, ari, fm, rand)))


# ------------------------------------------------------------------------------------------------ the large cases
def large_inputs(seed, V, D, C, n, repeats):
    """-> assign [V, D] int64, ids [n] int64 of a case of tests/golden/subset_scores_large.npz, which records these six numbers
    and not the arrays: make_assign of tests/golden/gen_subset_scores.py on RandomState(seed), then the ids from the same stream"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_subset_scores.py")
    spec = importlib.util.spec_from_file_location("_gen_subset_scores", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rs = np.random.RandomState(seed)
    assign = gen.make_assign(rs, V, D, C).astype(np.int64)
    ids = rs.randint(0, V, n) if repeats else rs.choice(V, n, replace=False)
    return assign, ids.astype(np.int64)


def ami_reorder_bound(N, s):
    """how far two float64 evaluations of adjusted_mutual_info can be apart when they add the same EMI terms in different
    orders: any order of T terms is within (T - 1) 2^-53 sum|term| of exact, so two orders differ by at most
    de = T 2^-52 sum|term| (charged in full); AMI = (mi - e) / (h - e) with h = the mean entropy has d AMI / d e =
    (mi - h) / (h - e)^2, and on the segment between the two values of e the denominator is at least |h - e| - de, hence
    |d AMI| <= de |h - mi| / (|h - e| (|h - e| - de)).  s: raw_stats(N).  -> de, the bound (inf when the guard leaves no room)"""
    t = emi_terms(N)
    de = len(t) * 2.0 ** -52 * float(np.abs(t).sum())
    h = (s['h_row'] + s['h_col']) / 2.0
    den = abs(h - s['emi'])
    return de, (de * abs(h - s['mi']) / (den * (den - de)) if den > de else float('inf'))
