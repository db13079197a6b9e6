"""FowlkesMallowsScore / RandScore / AdjustedRandScore -- the pair-counting agreement scores of the reference's
correspondence_retrieval stage (correspondence_retrieval/code/measures/efficient_pair.py), which its supplement ranks
subsets by beside AMI (search_targets/supplements/scores.json: efficient_fm, efficient_rand, efficient_arand).

They sit on the same contingency tables and the same exact greedy as `mi` (one kernel launch per pick, every remaining
candidate scored): measures 4, 5 and 6 of acav_mi_set_measure.  Per pair the kernel keeps the pair sums
T_ab = sum C(N,2), T_a = sum C(a,2), T_b = sum C(b,2), so a score is O(1) per candidate and pair, in float64:
  FM    sqrt(TP/(TP+FP) * TP/(TP+FN))          (efficient_pair.py:102-105)
  Rand  (TP+TN) / (TP+FP+FN+TN)                (efficient_pair.py:111-113)
  ARI   (Nc - ac bc/nc) / ((ac+bc)/2 - ac bc/nc)   on cache + candidate, NaN (0/0) while degenerate (efficient_pair.py:121-135)
FM and Rand reproduce the float64-eps residues of the reference's fp32 tables; ARI ranks NaN above
every number and takes the first NaN, as torch's max(dim=0) does.

Protocol (EfficientMI.run, efficient.py:240-302): the start clips are added to the tables before the first pick -- unlike
subset_selection's `mi`.  The reference removes them from its candidate list by position, which is only right for
candidates == range(V); here they are removed by id, so the pipeline's candidate list (without the start clip) works.
"""
import ctypes as C

import numpy as np

from ... import _lib
from .mi import EfficientMI


class _PairCountingMeasure(EfficientMI):
    _measure_id = None
    _takes_weights = False  # the reference's pair-counting classes override _calc_score: pair weights are ignored

    def init(self, clustering_combinations, candidates):
        super().init(clustering_combinations, candidates)
        _lib.check(_lib._lib.acav_mi_set_measure(self._h, self._measure_id))

    def pair_stats(self):
        """{'TP','FP','FN','TN'} int64 [P] of the current tables: per pair, sklearn's pair_confusion_matrix / 2 with the
        pair's first clustering as the truth (TP + FP + FN + TN = n (n - 1) / 2)."""
        out = {k: np.empty(self._npairs, np.int64) for k in ('TP', 'FP', 'FN', 'TN')}
        _lib.check(_lib._lib.acav_mi_get_pair_stats(self._h, _lib.ptr(out['TP']), _lib.ptr(out['FP']), _lib.ptr(out['FN']),
                                                    _lib.ptr(out['TN'])))
        return out

    def add_samples(self, ids):
        """add_samples (efficient.py:224-237): the clips join the tables and leave the candidate list (by id here)."""
        ids = np.ascontiguousarray([int(i) for i in ids], np.int64)
        super().add_samples(ids)
        gone = np.isin(self.candidate_ids, ids)
        if gone.any():
            self.candidate_ids = np.ascontiguousarray(self.candidate_ids[~gone])

    def run_greedy(self, subset_size, start_indices, intermediate_target=None, verbose=False, log_every=1,
                   log_times=None, node_rank=None, pid=None, record_trace=False, forced_pos=None, celf_ratio=0):
        """EfficientMI.run (efficient.py:240-302): add the start clips to the tables, then the exact greedy, the last
        round(niters * celf_ratio) picks of it as CELF lazy greedy (EfficientMI.run_greedy).
        forced_pos: positions in the candidate list as it stands after the start clips left it."""
        start = [int(i) for i in start_indices]
        self.add_samples(start)
        return super().run_greedy(subset_size, start, intermediate_target, verbose=verbose, log_every=log_every,
                                  log_times=log_times, node_rank=node_rank, pid=pid, record_trace=record_trace,
                                  forced_pos=forced_pos, celf_ratio=celf_ratio)

    @staticmethod
    def run_greedy_multi(measures, subset_sizes, start_indices_list, verbose=False):
        """run_greedy for several chunks in lockstep: every chunk's start clips join its tables first, as in run_greedy, then
        EfficientMI.run_greedy_multi.  The arguments are checked before the first table changes."""
        EfficientMI._check_lockstep(measures, subset_sizes, start_indices_list)
        starts = [[int(i) for i in s] for s in start_indices_list]
        for m, s in zip(measures, starts):
            m.add_samples(s)
        return EfficientMI.run_greedy_multi(measures, subset_sizes, starts, verbose=verbose)


class FowlkesMallowsScore(_PairCountingMeasure):
    """efficient_pair.py:22-105 ('fm', 'efficient_fm'): the Fowlkes-Mallows index of the selection, mean over the pairs."""
    _measure_id = 4

    @property
    def cache(self):
        """the tables plus the running pair counts TP / FP / FN / TN [P] (efficient_pair.py:23-27), as integers: the
        reference's float64-eps residues on top of a zero count are part of the kernel's state, not of these."""
        c = super().cache
        c.update(self.pair_stats())
        return c


class RandScore(FowlkesMallowsScore):
    """efficient_pair.py:107-113 ('rand', 'efficient_rand'): the Rand index of the selection, mean over the pairs."""
    _measure_id = 5


class AdjustedRandScore(_PairCountingMeasure):
    """efficient_pair.py:116-135 ('arand', 'efficient_arand'): the adjusted Rand index of the selection, mean over the
    pairs; NaN while some pair is degenerate (0/0), and a NaN candidate is taken first."""
    _measure_id = 6
