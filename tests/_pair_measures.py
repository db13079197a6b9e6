"""numpy float64 restatement of the exact greedy's pair-counting scores (fm / rand / arand) and of the ami / nmi
average methods -- the test oracle of these measures.

Pair counting (correspondence_retrieval/code/measures/efficient_pair.py), canonical form of the library's kernel:
  per pair p the running sums T_ab = sum C(N,2), T_a = sum C(a,2), T_b = sum C(b,2); TP = T_ab, FP = T_a - T_ab,
  FN = T_b - T_ab, TN = C(n,2) - T_a - T_b + T_ab.  The reference's fp32 tables start at float64 eps (2^-52): a zero cell
  of N holds eps, a zero marginal C eps.  Each running quantity is (integer I, residue count R), valued I if I > 0 else
  R eps; a sum drops R as soon as an integer part is >= 1.  A candidate at cell (i, j) adds dTP = N_ij (R 1 if 0),
  dFP = a_j - N_ij (R C - 1 if a_j = 0), dFN = b_i - N_ij (R C - 1 if b_i = 0), dTN = n - a_j - b_i + N_ij.
  FM = sqrt(TP/(TP+FP) * TP/(TP+FN)), Rand = (TP+TN)/(TP+FP+FN+TN) -- the denominator C(n+1, 2) is the same for every pair,
  so the pair mean is sum(TP+TN) / (P C(n+1, 2)), which keeps equal Rand indices exactly tied; ARI on cache + candidate:
  (Nc - ac bc/nc) / ((ac+bc)/2 - ac bc/nc), NaN when 0/0.  Mean over the pairs summed in pair order; the greedy takes the
  first NaN if there is one, else the first maximum.  Only +, -, *, / and sqrt: the kernel computes the same doubles.
"""
import numpy as np

EPS = 2.0 ** -52
PAIR_MEASURES = {"fm": 4, "rand": 5, "arand": 6}


def c2(x):
    x = np.asarray(x, np.int64)
    return x * (x - 1) // 2


def _val(I, R):
    return np.where(I > 0, I.astype(np.float64), R.astype(np.float64) * EPS)


def greedy_argmax(scores):
    """torch's max(dim=0) on the reference's scores: the first NaN, else the first maximum"""
    nan = np.isnan(scores)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(scores))


class PairGreedy:
    """the integer tables of one selection plus the running pair sums (the kernel's PairStat)"""

    def __init__(self, assignments, pairs, C):
        self.a = np.asarray(assignments, np.int64)
        self.pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        self.C = int(C)
        P = len(self.pairs)
        self.N = np.zeros((P, self.C, self.C), np.int64)
        self.A = np.zeros((P, self.C), np.int64)
        self.B = np.zeros((P, self.C), np.int64)
        self.n = 0
        self.reset_stats()

    def reset_stats(self):
        """init_pair_stats: sums from the tables, residues 0"""
        self.tab = c2(self.N).sum(axis=(1, 2))
        self.ta = c2(self.A).sum(axis=1)
        self.tb = c2(self.B).sum(axis=1)
        P = len(self.pairs)
        self.rtp = np.zeros(P, np.int64)
        self.rfp = np.zeros(P, np.int64)
        self.rfn = np.zeros(P, np.int64)

    def _cells(self, ids, p):
        ids = np.asarray(ids, np.int64)
        i = self.a[ids, self.pairs[p, 0]]
        j = self.a[ids, self.pairs[p, 1]]
        return i, j, self.N[p, i, j], self.A[p, j], self.B[p, i]

    def add_samples(self, ids):
        for w in ids:
            self._commit_tables(int(w))
        self.reset_stats()

    def _commit_tables(self, w):
        for p in range(len(self.pairs)):
            i, j = self.a[w, self.pairs[p, 0]], self.a[w, self.pairs[p, 1]]
            self.N[p, i, j] += 1
            self.A[p, j] += 1
            self.B[p, i] += 1
        self.n += 1

    def pair_stats(self):
        n2 = self.n * (self.n - 1) // 2
        return dict(TP=self.tab.copy(), FP=self.ta - self.tab, FN=self.tb - self.tab,
                    TN=((n2 - self.ta) - self.tb) + self.tab)

    def pair_scores(self, ids, measure):
        """[P, W] float64 scores of cache + each candidate"""
        n, C = self.n, self.C
        out = []
        with np.errstate(invalid="ignore", divide="ignore"):
            for p in range(len(self.pairs)):
                _, _, cN, ca, cb = self._cells(ids, p)
                tab, ta, tb = self.tab[p], self.ta[p], self.tb[p]
                if measure == "arand":
                    Nc2 = (tab + cN).astype(np.float64)
                    ac2 = (ta + ca).astype(np.float64)
                    bc2 = (tb + cb).astype(np.float64)
                    nc2 = np.float64(n * (n + 1) // 2)
                    chance = (ac2 * bc2) / nc2
                    out.append((Nc2 - chance) / (0.5 * (ac2 + bc2) - chance))
                    continue
                tpI = tab + cN
                fpI = (ta - tab) + (ca - cN)
                fnI = (tb - tab) + (cb - cN)
                tnI = ((n * (n - 1) // 2 - ta) - tb + tab) + (((n - ca) - cb) + cN)
                tpR = np.where(tpI > 0, 0, self.rtp[p] + 1)
                fpR = np.where(fpI > 0, 0, self.rfp[p] + np.where(ca == 0, C - 1, 0))
                fnR = np.where(fnI > 0, 0, self.rfn[p] + np.where(cb == 0, C - 1, 0))
                tp = _val(tpI, tpR)
                if measure == "fm":
                    out.append(np.sqrt((tp / _val(tpI + fpI, tpR + fpR)) * (tp / _val(tpI + fnI, tpR + fnR))))
                else:  # Rand's numerator; the denominator C(n+1, 2) is shared by every pair (scores())
                    out.append(_val(tpI + tnI, tpR))
        return np.array(out)

    def scores(self, ids, measure):
        ps = self.pair_scores(ids, measure)
        tot = np.zeros(ps.shape[1], np.float64)
        for p in range(ps.shape[0]):
            tot = tot + ps[p]
        if measure == "rand":
            return tot / (np.float64(ps.shape[0]) * np.float64(self.n * (self.n + 1) // 2))
        return tot / np.float64(ps.shape[0])

    def commit(self, w):
        """one pick: the running sums (with their residues), then the tables"""
        C = self.C
        for p in range(len(self.pairs)):
            i, j = self.a[w, self.pairs[p, 0]], self.a[w, self.pairs[p, 1]]
            cN, ca, cb = int(self.N[p, i, j]), int(self.A[p, j]), int(self.B[p, i])
            self.tab[p] += cN
            self.ta[p] += ca
            self.tb[p] += cb
            self.rtp[p] = 0 if self.tab[p] else self.rtp[p] + 1
            self.rfp[p] = 0 if self.ta[p] - self.tab[p] else self.rfp[p] + (C - 1 if ca == 0 else 0)
            self.rfn[p] = 0 if self.tb[p] - self.tab[p] else self.rfn[p] + (C - 1 if cb == 0 else 0)
        self._commit_tables(int(w))

    def run(self, candidates, subset, ns, measure, forced_idx=None):
        """the exact greedy after the start clips are in the tables: subset - 1 - ns picks.  forced_idx: positions among
        the REMAINING candidates to commit instead of the argmax.  -> dict(S, GAIN, scores (list of rows by remaining
        position), argmax)"""
        alive = [int(c) for c in candidates]
        iters = max(0, min(int(subset) - 1 - int(ns), len(alive)))
        S, GAIN, rows, am = [], [], [], []
        for t in range(iters):
            sc = self.scores(alive, measure)
            k = greedy_argmax(sc)
            rows.append(sc)
            am.append(k)
            if forced_idx is not None:
                k = int(forced_idx[t])
            S.append(alive[k])
            GAIN.append(sc[k])
            self.commit(alive[k])
            alive.pop(k)
        return dict(S=S, GAIN=np.array(GAIN, np.float64), scores=rows, argmax=am)


def golden_pair_run(g, measure, forced=True):
    """replay a pair_<case>_<measure>.npz golden with the restatement: candidates = every id but the start, in order"""
    a, C, start, subset = g["assignments"].astype(np.int64), int(g["C"]), int(g["start"]), int(g["subset"])
    m = PairGreedy(a, g["pairs"], C)
    m.add_samples([start])
    cand = [i for i in range(a.shape[0]) if i != start]
    return m.run(cand, subset, 1, measure, forced_idx=g["idx"] if forced else None)


# ------------------------------------------------------------------ ami / nmi with an average_method (dense float64)
def _xlogx_sum(x, n):
    p = x / n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(x > 0, p * np.log(np.where(x > 0, p, 1.0)), 0.0)
    return -t.sum(axis=-1)


def mi_family_scores(assignments, pairs, C, tables, ids, measure, method):
    """calc_AMI / calc_NMI (subset_selection measures/mi.py:212-271) of tables + each candidate, mean over the pairs, over
    integer counts (no eps): valid while neither clustering of a pair is degenerate"""
    from scipy.special import gammaln
    N0, A0, B0, n0 = tables
    a = np.asarray(assignments, np.int64)
    ids = np.asarray(ids, np.int64)
    n = float(n0 + 1)
    tot = np.zeros(len(ids))
    for p, (d0, d1) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
        i, j = a[ids, d0], a[ids, d1]
        W = len(ids)
        N = np.repeat(N0[p][None].astype(np.float64), W, 0)
        N[np.arange(W), i, j] += 1
        A = np.repeat(A0[p][None].astype(np.float64), W, 0)
        A[np.arange(W), j] += 1
        B = np.repeat(B0[p][None].astype(np.float64), W, 0)
        B[np.arange(W), i] += 1
        Ab, Bb = A[:, None, :], B[:, :, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.where(N > 0, np.log(np.where(N > 0, N, 1.0)) + np.log(n) - np.log(np.maximum(Ab, 1)) - np.log(np.maximum(Bb, 1)), 0.0)
        mi = (N / n * lg).sum(axis=(1, 2))
        ha, hb = _xlogx_sum(A, n), _xlogx_sum(B, n)
        norm = {"arithmetic": (ha + hb) / 2, "max": np.maximum(ha, hb), "min": np.minimum(ha, hb)}[method]
        if measure == "nmi":
            s = 2 * mi / np.maximum(norm, np.finfo(np.float64).eps)
        else:
            t1 = N / n * lg
            l2 = (gammaln(Ab + 1) + gammaln(Bb + 1) + gammaln(n - Ab + 1) + gammaln(n - Bb + 1)
                  - (gammaln(n + 1) + gammaln(N + 1) + gammaln(np.maximum(Ab - N, 0) + 1) + gammaln(np.maximum(Bb - N, 0) + 1)
                     + gammaln(np.maximum(n - Ab - Bb + N, 0) + 1)))
            emi = np.where(N > 0, t1 * np.exp(l2), 0.0).sum(axis=(1, 2))
            s = (mi - emi) / np.maximum(norm - emi, np.finfo(np.float64).eps)
        tot = tot + s
    return tot / len(pairs)


def golden_avg_run(g, measure, method):
    """teacher-forced replay of a mi_avg_<measure>_<method>_<case>.npz golden -> list of score rows"""
    a, C = g["assignments"].astype(np.int64), int(g["C"])
    pairs = np.asarray(g["pairs"], np.int64)
    P = len(pairs)
    N = np.zeros((P, C, C), np.int64)
    A = np.zeros((P, C), np.int64)
    B = np.zeros((P, C), np.int64)
    n = 0

    def add(w):
        nonlocal n
        for p, (d0, d1) in enumerate(pairs):
            N[p, a[w, d0], a[w, d1]] += 1
            A[p, a[w, d1]] += 1
            B[p, a[w, d0]] += 1
        n += 1

    for w in g["seeds"]:
        add(int(w))
    alive = [int(c) for c in g["candidates"]]
    rows = []
    for k in g["idx"]:
        rows.append(mi_family_scores(a, pairs, C, (N, A, B, n), alive, measure, method))
        add(alive[int(k)])
        alive.pop(int(k))
    return rows
