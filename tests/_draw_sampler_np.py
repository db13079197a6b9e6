"""Restatement of batch.sampler=draw (include/acav_hip.h: acav_mi_run_draw) in plain numpy -- test infrastructure.

Per chunk: the candidate array r[0 .. L0) as handed in and a window start lo = 0; the live list is r[lo .. L0).  An iteration
  1. draws: for t < B: z = w % (L - t), swap r[lo+t] and r[lo+t+z] (L = L0 - lo at the start of the iteration; w = the
     generator's next tempered word; exactly B words, also where L - t = 1); batch position b is r[lo+b]
  2. scores the batch, ranks it (score descending, NaN as -inf, ties to the lower batch position) and commits the k best in
     pick order
  3. shrinks: keep_unselected: the unselected ids, in batch order, go to r[lo+k .. lo+B), lo += k; else lo += B.
The draws, the scores and the commits come from the caller (the oracle's, or a second device handle's for weighted pairs).
"""
import math

import numpy as np


def draw_batch(r, lo, B, u32):
    """step 1 on r (in place); u32() -> the next generator word.  -> the batch, a copy of r[lo : lo + B]"""
    L = len(r) - lo
    assert L >= B
    for t in range(B):
        z = (int(u32()) & 0xFFFFFFFF) % (L - t)
        r[lo + t], r[lo + t + z] = r[lo + t + z], r[lo + t]
    return r[lo:lo + B].copy()


def rank_batch(scores, k):
    """step 2's order: -> the batch positions of the k best, in pick order"""
    s = np.asarray(scores, np.float64)
    key = np.where(np.isnan(s), -np.inf, s)
    return np.argsort(-key, kind='stable')[:k].astype(np.int32)


def shrink(r, lo, B, pos, keep_unselected):
    """step 3 on r (in place); pos: the committed batch positions.  -> the new window start"""
    k = len(pos)
    if not keep_unselected:
        return lo + B
    picked = set(int(p) for p in pos)
    rest = [r[lo + b] for b in range(B) if b not in picked]
    r[lo + k:lo + B] = rest
    return lo + k


def plan(L0, subset, B, k, keep_unselected, max_iters=-1):
    """-> (iterations, generator words), or ('short', candidates left) when the list falls below a batch before the subset
    is full: the permutation loop's condition with the list shrinking by k (keep_unselected) or B"""
    iters = math.ceil(subset / k)
    if max_iters >= 0:
        iters = min(iters, max_iters)
    step = k if keep_unselected else B
    for it in range(iters):
        if L0 - it * step < B:
            return 'short', L0 - it * step
    return iters, iters * B


def run_draw(candidates, subset, B, k, keep_unselected, u32, score, commit, max_iters=-1):
    """the whole loop (the start indices are the caller's: commit them first).  score(ids) -> float64 [B]; commit(ids) adds
    them to the tables in order.  -> dict(ids [iters, B], scores [iters, B], pos [iters, k], S, GAIN, r, lo)"""
    r = np.array(candidates, np.int64)
    iters, _ = plan(len(r), subset, B, k, keep_unselected, max_iters)
    assert iters != 'short'
    lo = 0
    ids = np.empty((iters, B), np.int64)
    scores = np.empty((iters, B), np.float64)
    pos = np.empty((iters, k), np.int32)
    S, GAIN = [], []
    for it in range(iters):
        batch = draw_batch(r, lo, B, u32)
        sc = np.asarray(score(batch), np.float64)
        p = rank_batch(sc, k)
        ids[it], scores[it], pos[it] = batch, sc, p
        commit(batch[p])
        S.extend(int(i) for i in batch[p])
        GAIN.extend(float(g) for g in sc[p])
        lo = shrink(r, lo, B, p, keep_unselected)
    return dict(ids=ids, scores=scores, pos=pos, S=np.array(S[:subset], np.int64), GAIN=np.array(GAIN, np.float64), r=r, lo=lo,
                iters=iters)
