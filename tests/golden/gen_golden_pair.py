#!/usr/bin/env python3
"""Generate the golden vectors of the pair-counting measures and of the ami / nmi average methods by running the
REFERENCE itself (only where the reference is mounted; what is committed is the data it produced).

    python tests/golden/gen_golden_pair.py            # both groups
    python tests/golden/gen_golden_pair.py pair|avg

pair  pair_<case>_<measure>.npz: correspondence_retrieval's FowlkesMallowsScore / RandScore / AdjustedRandScore
      (measures/efficient_pair.py) on the CPU through EfficientMI.run (efficient.py:240-302), candidates = range(V),
      one start clip.  Per iteration: the fp32 score vector by remaining position (scores.mean(-1), row t holds L - t
      values, NaN-padded), the argmax, and the fp32 gap between the best and the second-best distinct score
      (margin; NaN where the best is NaN); then S and GAIN.
avg   mi_avg_<measure>_<method>_<case>.npz: subset_selection's EfficientAMI / EfficientNMI (measures/mi.py:212-271)
      with average_method max and min, constructed directly: init(pairs, candidates), add_samples(seed clips) so that no
      clustering of a pair is degenerate, then run_greedy(subset, seeds).  Same records.

The two reference stages have clashing top-level module names (`measures`), so each group runs in its own interpreter.
"""
import itertools
import os
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
STUBS = os.path.join(HERE, "_stubs")

# name: (seed, V, D, C, start clip, subset)
PAIR_CASES = {
    "a": (0, 200, 2, 40, 5, 42),      # P = 1, C large against the picks: the eps-residue regime; ARI mostly NaN
    "b": (1, 200, 3, 40, 17, 42),     # P = 3, residue regime
    "c": (2, 150, 3, 12, 33, 60),     # P = 3
    "d": (3, 120, 4, 6, 71, 50),      # P = 6
    "e": (4, 330, 3, 8, 101, 302),    # 300 picks
}
PAIR_MEASURES = ("fm", "rand", "arand")

# name: (seed, V, D, C, number of seed clips, subset)
AVG_CASES = {
    "a": (10, 160, 2, 6, 12, 50),
    "b": (11, 200, 3, 8, 16, 56),
}


def correlated(seed, v, dd, c):
    """clusterings that agree on about half of the clips (the layout of gen_golden.py gen_mi_nmi)"""
    rs = np.random.RandomState(700 + seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    a = np.stack(cols, 1).astype(np.int64)
    a[0] = c - 1
    return a


def _recorder(cls):
    """wrap cls.calc_score: record scores.mean(-1) (fp32), the argmax and the top-two margin of every iteration"""
    import torch
    rec = dict(scores=[], idx=[], margin=[])

    def calc_score(self, *a, **k):
        sc = self._calc_score(*a, **k).mean(dim=-1)
        score, idx = sc.max(dim=0)
        v = sc.cpu().numpy().astype(np.float32).copy()
        rec["scores"].append(v)
        rec["idx"].append(int(idx.item()))
        if np.isnan(v[int(idx.item())]):
            rec["margin"].append(np.nan)
        else:
            u = np.unique(v[~np.isnan(v)])
            rec["margin"].append(float(u[-1]) - float(u[-2]) if len(u) > 1 else np.inf)
        return score.item(), idx.item()

    return rec, calc_score, torch


def _pack(rec):
    w0 = len(rec["scores"][0])
    sc = np.full((len(rec["scores"]), w0), np.nan, np.float32)
    for t, row in enumerate(rec["scores"]):
        sc[t, :len(row)] = row
    return sc, np.array(rec["idx"], np.int64), np.array(rec["margin"], np.float64)


def gen_pair():
    sys.path.insert(0, STUBS)
    sys.path.insert(0, os.path.join(REF, "correspondence_retrieval", "code"))
    from measures.efficient import EfficientMI  # noqa: E402  (the reference)
    from measures.efficient_pair import AdjustedRandScore, FowlkesMallowsScore, RandScore  # noqa: E402
    classes = dict(fm=FowlkesMallowsScore, rand=RandScore, arand=AdjustedRandScore)
    for name, (seed, v, dd, c, start, subset) in PAIR_CASES.items():
        a = correlated(seed, v, dd, c)
        pairs = list(itertools.combinations(range(dd), 2))
        for mname in PAIR_MEASURES:
            cls = classes[mname]
            rec, calc_score, torch = _recorder(cls)
            orig = EfficientMI.calc_score
            EfficientMI.calc_score = calc_score
            try:
                clusterings = [types.SimpleNamespace(ncentroids=c, ind2cen=a[:, d].tolist()) for d in range(dd)]
                m = cls(clusterings)
                m.device = "cpu"
                m.init(pairs, list(range(v)))
                S, GAIN, _, _ = m.run_greedy(subset, [start])
            finally:
                EfficientMI.calc_score = orig
            sc, idx, margin = _pack(rec)
            out = os.path.join(HERE, f"pair_{name}_{mname}.npz")
            np.savez_compressed(out, assignments=a.astype(np.int16), pairs=np.array(pairs, np.int64), C=c, start=start,
                                subset=subset, S=np.array(S, np.int64), GAIN=np.array(GAIN, np.float64), scores=sc, idx=idx,
                                margin=margin)
            g = np.array(GAIN)
            print(f"{os.path.basename(out)}: {len(S)} selected, {np.isnan(g).sum()} NaN gains, "
                  f"{os.path.getsize(out)} bytes")


def gen_avg():
    sys.path.insert(0, STUBS)
    sys.path.insert(0, os.path.join(REF, "subset_selection", "code"))
    from measures.mi import EfficientAMI, EfficientMI, EfficientNMI  # noqa: E402  (the reference)
    classes = dict(ami=EfficientAMI, nmi=EfficientNMI)
    for name, (seed, v, dd, c, nseed, subset) in AVG_CASES.items():
        a = correlated(seed, v, dd, c)
        pairs = list(itertools.combinations(range(dd), 2))
        rs = np.random.RandomState(900 + seed)
        seeds = [int(i) for i in rs.choice(np.arange(1, v), nseed, replace=False)]
        for d in range(dd):
            assert len(set(a[seeds, d].tolist())) > 1, "a seed set with one label in some clustering"
        cand = [i for i in range(v) if i not in set(seeds)]
        for mname, method in itertools.product(("ami", "nmi"), ("max", "min", "arithmetic")):
            cls = classes[mname]
            rec, calc_score, torch = _recorder(cls)
            orig = EfficientMI.calc_score
            EfficientMI.calc_score = calc_score
            try:
                m = cls(a, average_method=method, ncentroids=c)
                m.device = "cpu"
                m.init(pairs, cand)
                m.add_samples(seeds)
                S, GAIN, _, _ = m.run_greedy(subset, list(seeds))
            finally:
                EfficientMI.calc_score = orig
            sc, idx, margin = _pack(rec)
            out = os.path.join(HERE, f"mi_avg_{mname}_{method}_{name}.npz")
            np.savez_compressed(out, assignments=a.astype(np.int16), pairs=np.array(pairs, np.int64), C=c,
                                seeds=np.array(seeds, np.int64), candidates=np.array(cand, np.int64), subset=subset,
                                S=np.array(S, np.int64), GAIN=np.array(GAIN, np.float64), scores=sc, idx=idx, margin=margin)
            print(f"{os.path.basename(out)}: {len(S)} selected, {os.path.getsize(out)} bytes")


GROUPS = {"pair": gen_pair, "avg": gen_avg}

if __name__ == "__main__":
    which = sys.argv[1:] or list(GROUPS)
    if len(which) > 1:  # one interpreter per group
        for w in which:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), w])
    else:
        GROUPS[which[0]]()
