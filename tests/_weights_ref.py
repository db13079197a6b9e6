"""numpy float64 restatement of the weighted MI greedy (clustering pairs weighted per layer, `weight_type`) -- the test oracle
of acav_mi_set_pair_weights.

The library's canonical score of candidate w for pair p (acav_mi.hip mi_pair_score, oracle/acav_oracle.c "canon"): with
phi(k) = k ln k over the integer tables and the running sums SN = sum phi(N), Sa = sum phi(a), Sb = sum phi(b),
  s_p = (((SN - phi(N_ij) + phi(N_ij + 1)) - (Sa - phi(a_j) + phi(a_j + 1))) - (Sb - phi(b_i) + phi(b_i + 1)) + phi(n + 1)) / (n + 1)
and the weighted score is (sum over p in pair order of s_p * (double)w_p, from 0.0) / P, w_p the fp32-rounded weight.  A commit
updates the sums pick by pick, pair by pair, in the same order as the kernels.  phi comes from math.log (the C library's log,
as the library's host table), every other step is one IEEE double operation, so the numbers match bit for bit.
"""
import math

import numpy as np


def phi_table(n):
    out = np.zeros(n + 2, np.float64)
    for k in range(1, n + 2):
        out[k] = float(k) * math.log(float(k))
    return out


def fp32_weights(weights):
    """torch.tensor(weights).float(), back in float64"""
    return np.asarray(weights, np.float64).astype(np.float32).astype(np.float64)


class WeightedMI:
    def __init__(self, assignments, pairs, C, weights=None, phi=None):
        self.a = np.asarray(assignments, np.int64)
        self.pairs = np.asarray([tuple(p)[:2] for p in pairs], np.int64).reshape(-1, 2)
        self.C = int(C)
        P = len(self.pairs)
        self.w = None if weights is None else fp32_weights(weights)
        assert self.w is None or self.w.shape == (P,)
        self.phi = phi_table(len(self.a)) if phi is None else phi
        self.N = np.zeros((P, self.C, self.C), np.int64)
        self.A = np.zeros((P, self.C), np.int64)   # a: column sums, indexed by the second clustering's label
        self.B = np.zeros((P, self.C), np.int64)   # b: row sums, indexed by the first clustering's label
        self.SN = np.zeros(P, np.float64)
        self.Sa = np.zeros(P, np.float64)
        self.Sb = np.zeros(P, np.float64)
        self.n = 0

    def commit(self, ids):
        phi = self.phi
        for w in ids:
            w = int(w)
            for p in range(len(self.pairs)):
                i, j = self.a[w, self.pairs[p, 0]], self.a[w, self.pairs[p, 1]]
                cN, ca, cb = self.N[p, i, j], self.A[p, j], self.B[p, i]
                self.N[p, i, j] = cN + 1
                self.A[p, j] = ca + 1
                self.B[p, i] = cb + 1
                self.SN[p] = self.SN[p] - phi[cN] + phi[cN + 1]
                self.Sa[p] = self.Sa[p] - phi[ca] + phi[ca + 1]
                self.Sb[p] = self.Sb[p] - phi[cb] + phi[cb + 1]
            self.n += 1

    def scores(self, ids):
        """the weighted (or plain) pair mean of every candidate in ids, float64"""
        ids = np.asarray(ids, np.int64)
        phi, n = self.phi, self.n
        tot = np.zeros(len(ids), np.float64)
        for p in range(len(self.pairs)):
            i, j = self.a[ids, self.pairs[p, 0]], self.a[ids, self.pairs[p, 1]]
            cN, ca, cb = self.N[p, i, j], self.A[p, j], self.B[p, i]
            sN = (self.SN[p] - phi[cN]) + phi[cN + 1]
            sa = (self.Sa[p] - phi[ca]) + phi[ca + 1]
            sb = (self.Sb[p] - phi[cb]) + phi[cb + 1]
            s = (((sN - sa) - sb) + phi[n + 1]) / float(n + 1)
            tot = tot + (s * self.w[p] if self.w is not None else s)
        return tot / float(len(self.pairs))

    # ------------------------------------------------------------------ greedy loops
    def run_exact(self, candidates, iters):
        """EfficientMI.run_greedy (subset_selection mi.py:150-192): all remaining candidates, first maximum"""
        alive = list(int(c) for c in candidates)
        S, G = [], []
        for _ in range(iters):
            sc = self.scores(alive)
            b = int(np.argmax(sc))
            S.append(alive[b])
            G.append(float(sc[b]))
            self.commit([alive[b]])
            alive.pop(b)
        return S, G

    def select(self, batch, k):
        """one batch-greedy iteration on the given batch: top k by (score desc, position asc), committed in that order"""
        sc = self.scores(batch)
        order = np.lexsort((np.arange(len(batch)), -sc))[:k]
        picks = [int(batch[r]) for r in order]
        self.commit(picks)
        return picks, [float(sc[r]) for r in order], sc, [int(r) for r in order]

    def run_batch_traced(self, start, trace_ids, k):
        """the batch greedy on the batches a GPU run traced (its permutation stream)"""
        self.commit(start)
        S, G, SC, POS = [], [], [], []
        for batch in trace_ids:
            p, g, sc, pos = self.select(batch, k)
            S += p
            G += g
            SC.append(sc)
            POS.append(pos)
        return S, G, np.array(SC), np.array(POS)

    def run_batch(self, candidates, start, subset, B, k, rng, keep_unselected=True):
        """the whole batch greedy (subset_selection batch.py:195-260) with the permutations of rng (torch.randperm)"""
        self.commit(start)
        cand = np.asarray(candidates, np.int64)
        S, G = [], []
        while len(S) < subset:
            cand = cand[rng.randperm(len(cand))]
            batch, cand = cand[:B], cand[B:]
            p, g, _, _ = self.select(batch, k)
            S += p
            G += g
            if keep_unselected:
                cand = np.concatenate([cand, np.sort(np.setdiff1d(batch, p))])
        return S[:subset], G
