"""numpy restatement of the exact greedy with a CELF lazy phase (celf_ratio) -- the test oracle of acav_mi_run_celf.

The algorithm (correspondence_retrieval's EfficientMI.run with celf_ratio, in the canonical form of DESIGN.md "CELF"):
  * the first round(niters * (1 - celf_ratio)) picks are the plain exact greedy: score every remaining candidate, take the
    first NaN if there is one, else the first maximum; GAIN is that score, LOOKUPS 1;
  * then the queue is filled with the ABSOLUTE scores of every remaining candidate, in candidate order, and
    gain = the last greedy GAIN (0.0 if there was none);
  * a lazy pick repeats: count a lookup, re-score the head against the current tables, d = score - gain, give the head the
    value d; the head is accepted when it is still the head.  Then gain = gain + d, GAIN is gain, the clip joins the tables.
  * the queue is totally ordered by (value descending, stamp descending), NaN above every number; an entry never re-scored
    carries the stamp -(its position in the candidate list when the queue was filled), an entry re-scored at the run's t-th
    lookup carries t.
It is written with a literal priority queue (heapq), one re-scoring per lookup, nothing speculative.  The scores come from
the restatements the other tests already use: tests/_weights_ref.py (the MI closed form, weighted or not),
tests/_pair_measures.py (fm / rand / arand) and the C oracle's canonical `ami`; `nmi` and `constant` are restated here on the
running sums of the MI closed form.
"""
import heapq
import math

import numpy as np

from tests import _pair_measures as PM
from tests._weights_ref import WeightedMI

EXACT_MEASURES = ("mi", "mem_mi", "ami", "nmi", "constant", "fm", "rand", "arand")
ADDS_START = ("fm", "rand", "arand")  # EfficientMI.run of the stage they come from puts the start clips into the tables
F64_EPS = 2.220446049250313e-16


class _MI:
    """mi / mem_mi (optionally pair-weighted), nmi (arithmetic mean) and constant on the running sums of WeightedMI"""

    def __init__(self, a, pairs, C, measure, weights=None):
        self.m = WeightedMI(a, pairs, C, weights=weights if measure in ("mi", "mem_mi") else None)
        self.measure = measure

    def add_samples(self, ids):
        self.m.commit(ids)

    def commit(self, w):
        self.m.commit([w])

    def scores(self, ids):
        if self.measure in ("mi", "mem_mi"):
            return self.m.scores(ids)
        ids = np.asarray(ids, np.int64)
        if self.measure == "constant":
            return np.ones(len(ids), np.float64)
        m = self.m
        phi, n1 = m.phi, m.n + 1
        ln_n, ln_c, ln_eps, C = math.log(float(n1)), math.log(float(m.C)), -36.043653389117154, float(m.C)
        tot = np.zeros(len(ids), np.float64)
        for p in range(len(m.pairs)):
            i, j = m.a[ids, m.pairs[p, 0]], m.a[ids, m.pairs[p, 1]]
            cN, ca, cb = m.N[p, i, j], m.A[p, j], m.B[p, i]
            sN = (m.SN[p] - phi[cN]) + phi[cN + 1]
            sa = (m.Sa[p] - phi[ca]) + phi[ca + 1]
            sb = (m.Sb[p] - phi[cb]) + phi[cb + 1]
            mi = (((sN - sa) - sb) + phi[n1]) / float(n1)
            ha, hb = ln_n - sa / float(n1), ln_n - sb / float(n1)
            den = np.maximum((ha + hb) / 2.0, F64_EPS)
            s = (2.0 * mi) / den
            num = (C - 1.0) * ((ln_n - ln_eps) - 2.0 * ln_c) - 2.0 * ln_c  # every sample in one cell
            s = np.where(cN + 1 == n1, (2.0 * num) / (C * ((ln_n - ln_c) - ln_eps)), s)
            tot = tot + s
        return tot / float(len(m.pairs))


class _AMI:
    """the canonical `ami` of the C oracle (oracle/acav_oracle.c ami_score_canon)"""

    def __init__(self, a, pairs, C):
        from oracle import oracle as O
        self.m = O.BatchMI(np.asarray(a, np.int64), C, np.asarray(pairs, np.int32).reshape(-1, 2))
        self.m.set_measure("ami")

    def add_samples(self, ids):
        self.m.add_samples([int(i) for i in ids])

    def commit(self, w):
        self.m.add_samples([int(w)])

    def scores(self, ids):
        return self.m.scores_ami([int(i) for i in ids])


class _Pair:
    def __init__(self, a, pairs, C, measure):
        self.m = PM.PairGreedy(a, pairs, C)
        self.measure = measure

    def add_samples(self, ids):
        self.m.add_samples(ids)

    def commit(self, w):
        self.m.commit(int(w))

    def scores(self, ids):
        return self.m.scores(ids, self.measure)


def scorer(measure, assignments, pairs, C, weights=None):
    pairs = [tuple(p)[:2] for p in np.asarray(pairs).tolist()] if not isinstance(pairs, list) else [tuple(p)[:2] for p in pairs]
    if measure in ADDS_START:
        return _Pair(assignments, pairs, C, measure)
    if measure == "ami":
        return _AMI(assignments, pairs, C)
    return _MI(assignments, pairs, C, measure, weights)


def _key(val, stamp):
    """heapq pops the smallest: NaN first, then value descending, then stamp descending"""
    return (0, 0.0, -stamp) if val != val else (1, -val, -stamp)


def run(sc, candidates, subset, ns, celf_ratio=0, trace_cap=64):
    """the picks after the start clips (which the caller has put into the tables where the measure wants them).
    -> dict(S, GAIN float64, LOOKUPS, lookup_ids / lookup_values: per lazy pick, the first trace_cap lookups, queue: {clip:
    value} at the end, greedy_picks)"""
    if not 0 <= celf_ratio <= 1:
        raise ValueError("celf_ratio must lie in [0, 1]")
    alive = [int(c) for c in candidates]
    niters = max(0, min(int(subset) - 1 - int(ns), len(alive)))
    ngreedy = round(niters * (1 - celf_ratio))
    S, GAIN, LOOKUPS, tr_ids, tr_vals = [], [], [], [], []
    for _ in range(ngreedy):
        s = sc.scores(alive)
        k = PM.greedy_argmax(s)
        S.append(alive[k])
        GAIN.append(np.float64(s[k]))
        LOOKUPS.append(1 if celf_ratio else 0)
        sc.commit(alive[k])
        alive.pop(k)
    queue = {}
    if niters > ngreedy:
        gain = GAIN[-1] if GAIN else np.float64(0.0)
        vals = np.asarray(sc.scores(alive), np.float64)
        value = {c: np.float64(v) for c, v in zip(alive, vals)}
        stamp = {c: -pos for pos, c in enumerate(alive)}
        heap = [_key(value[c], stamp[c]) + (c,) for c in alive]
        heapq.heapify(heap)
        t = 0
        for _ in range(niters - ngreedy):
            lookup, ids, dvals = 0, [], []
            while True:
                lookup += 1
                t += 1
                head = heapq.heappop(heap)[-1]
                d = np.float64(sc.scores([head])[0]) - gain
                value[head], stamp[head] = d, t
                if lookup <= trace_cap:
                    ids.append(head)
                    dvals.append(d)
                heapq.heappush(heap, _key(d, t) + (head,))
                if heap[0][-1] == head:
                    break
            heapq.heappop(heap)
            with np.errstate(invalid="ignore"):
                gain = gain + value[head]
            S.append(head)
            GAIN.append(gain)
            LOOKUPS.append(lookup)
            tr_ids.append(ids)
            tr_vals.append(dvals)
            sc.commit(head)
            del value[head], stamp[head]
        queue = value
    return dict(S=S, GAIN=np.array(GAIN, np.float64), LOOKUPS=LOOKUPS, lookup_ids=tr_ids, lookup_values=tr_vals, queue=queue,
                greedy_picks=ngreedy)


def run_measure(measure, assignments, pairs, C, candidates, start, subset, celf_ratio=0, weights=None, trace_cap=64):
    """a whole selection as the measure classes run it: the pair-counting measures add the start clips to the tables"""
    sc = scorer(measure, assignments, pairs, C, weights)
    if measure in ADDS_START:
        sc.add_samples([int(s) for s in start])
        gone = set(int(s) for s in start)
        candidates = [int(c) for c in candidates if int(c) not in gone]
    return run(sc, candidates, subset, len(start), celf_ratio, trace_cap)
