"""EfficientMI / EfficientMemMI -- the reference's exact-greedy measures 'mi' and 'mem_mi'
(subset_selection/code/measures/mi.py:14-207, 284-412; registry measures/__init__.py:5-14).

Every iteration scores ALL remaining candidates against the current contingency tables, commits the first
maximum and removes it (mi.py:76-114).  The reference evaluates this densely -- `mi` on [W,P,C,C] fp32 tensors,
`mem_mi` through running fp32 n-log-n sums -- and its two measures already disagree with each other on near-ties
(tests/golden/gen_golden.py: S equivalence 12-66 %).  Both are the same function of the integer tables; here that
function is the canonical float64 closed form of libacav_hip.so (one kernel launch per iteration, all candidates
scored in parallel on the GPU).  Same constructor / init / run_greedy surface as the reference, so
run_greedy._run_greedy drives it unchanged.  No CPU path.
"""
import ctypes as C
import time

import numpy as np

from ... import _lib
from .batch import EfficientBatchMI


class EfficientMI(EfficientBatchMI):
    """ this implementation requires the users to use the same ncentroids for all clusterings """

    def __init__(self, assignments, measure_type='mutual_info', average_method='arithmetic', ncentroids=20,
                 device='cuda', **kwargs):
        kwargs.pop('batch_size', None)
        kwargs.pop('selection_size', None)
        kwargs.pop('keep_unselected', None)
        super().__init__(assignments, measure_type=measure_type, average_method=average_method,
                         ncentroids=ncentroids, batch_size=1, selection_size=1, device=device, **kwargs)

    # calc_measure (mi.py:108-114) for callers that step the greedy themselves
    def calc_measure(self):
        S, G = self._run(2, 0, None, False)
        return G[0], S[0]

    def _run(self, subset_size, ns, forced_pos, record_trace):
        cand = self.candidate_ids
        L = len(cand)
        niters = max(0, min(int(subset_size) - 1 - int(ns), L))
        S = np.empty(niters + 1, np.int64)
        G = np.empty(niters + 1, np.float64)
        fp = None if forced_pos is None else np.ascontiguousarray(forced_pos, np.int64)
        tr_sc = np.empty((niters, L), np.float64) if record_trace else None
        tr_am = np.empty(niters + 1, np.int64) if record_trace else None
        nsel = C.c_int64(0)
        _lib.check(_lib._lib.acav_mi_run_exact(self._h, _lib.ptr(cand), L, int(ns), int(subset_size), _lib.ptr(S),
                                               _lib.ptr(G), C.byref(nsel), _lib.ptr(fp), _lib.ptr(tr_sc),
                                               _lib.ptr(tr_am)))
        n = nsel.value
        if record_trace:
            self.trace = dict(scores=tr_sc[:n], argmax=tr_am[:n].copy())
        # the candidate list of the reference shrinks as it goes (remove_idx_all, mi.py:104-106)
        picked = set(S[:n].tolist())
        if picked:
            self.candidate_ids = np.ascontiguousarray([c for c in cand.tolist() if c not in picked], np.int64)
        return S[:n].tolist(), G[:n].tolist()

    CELF_TRACE_CAP = 64  # lookups recorded per CELF pick by record_trace

    def _run_celf(self, subset_size, ns, celf_ratio, record_trace):
        """acav_mi_run_celf: the exact greedy, then CELF lazy greedy (correspondence_retrieval efficient.py:140-196)."""
        cand = self.candidate_ids
        L = len(cand)
        niters = max(0, min(int(subset_size) - 1 - int(ns), L))
        S = np.empty(niters + 1, np.int64)
        G = np.empty(niters + 1, np.float64)
        K = np.zeros(niters + 1, np.int64)
        cap = self.CELF_TRACE_CAP if record_trace else 0
        tr_ids = np.empty((niters + 1, cap), np.int64) if record_trace else None
        tr_vals = np.empty((niters + 1, cap), np.float64) if record_trace else None
        queue = np.empty(L, np.float64) if record_trace else None
        nsel = C.c_int64(0)
        _lib.check(_lib._lib.acav_mi_run_celf(self._h, _lib.ptr(cand), L, int(ns), int(subset_size), float(celf_ratio),
                                              _lib.ptr(S), _lib.ptr(G), _lib.ptr(K), C.byref(nsel), cap, _lib.ptr(tr_ids),
                                              _lib.ptr(tr_vals), _lib.ptr(queue)))
        n = nsel.value
        if record_trace:
            ngreedy = int(round(n * (1 - celf_ratio)))
            self.trace = dict(lookup_ids=tr_ids[:n - ngreedy], lookup_values=tr_vals[:n - ngreedy], queue=queue,
                              greedy_picks=ngreedy)
        picked = set(S[:n].tolist())
        if picked:
            self.candidate_ids = np.ascontiguousarray([c for c in cand.tolist() if c not in picked], np.int64)
        return S[:n].tolist(), G[:n].tolist(), K[:n].tolist()

    def run(self, subset_size, start_indices, intermediate_target=None, celf_ratio=0):
        """EfficientMI.run of the correspondence_retrieval stage (efficient.py:240-299), same signature."""
        return self.run_greedy(subset_size, start_indices, intermediate_target, celf_ratio=celf_ratio)

    def run_greedy(self, subset_size, start_indices, intermediate_target=None, verbose=False, log_every=1,
                   log_times=None, node_rank=None, pid=None, record_trace=False, forced_pos=None, celf_ratio=0):
        """mi.py:150-192: returns (S, GAIN, timelapse, LOOKUPS) with S = start_indices + the picks.
        forced_pos: ORIGINAL positions (indices into the candidate list given to init) to commit instead of the
        argmax -- replays a recorded run.
        celf_ratio (efficient.py:240-299): the last round(niters * celf_ratio) picks are CELF lazy greedy -- a queue of stale
        gains of which only the head is re-scored until it stays on top; GAIN is then the accumulated gain and LOOKUPS the
        number of re-scorings (1 per greedy pick).  0 is the plain greedy, LOOKUPS all 0 as before.  The queue order among
        equal values is pinned ("CELF"): a free-running lazy selection equals the reference's up to its first
        exact tie."""
        if not 0 <= celf_ratio <= 1:
            raise ValueError("celf_ratio must lie in [0, 1], got {!r}".format(celf_ratio))
        start = list(start_indices)
        if celf_ratio:
            if forced_pos is not None:
                raise ValueError("forced_pos replays the plain greedy only: celf_ratio must be 0")
            t0 = time.time()
            S, GAIN, LOOKUPS = self._run_celf(subset_size, len(start), celf_ratio, record_trace)
            elapsed = time.time() - t0
            if verbose:
                print("(LEN: {}, MEASURE: {})".format(len(start) + len(S), GAIN[-1] if GAIN else float('nan')))
                print("Time Consumed: {} seconds".format(elapsed))
            return (start + S, GAIN, [elapsed / max(len(S), 1)] * len(S), LOOKUPS)
        t0 = time.time()
        S, GAIN = self._run(subset_size, len(start), forced_pos, record_trace)
        elapsed = time.time() - t0
        n = len(S)
        if verbose:
            msg = "(LEN: {}, MEASURE: {})".format(len(start) + n, GAIN[-1] if GAIN else float('nan'))
            if node_rank is not None:
                msg = 'Node: {}, '.format(node_rank) + msg
            print(msg)
            print("Time Consumed: {} seconds".format(elapsed))
        return (start + S, GAIN, [elapsed / max(n, 1)] * n, [0] * n)

    # ------------------------------------------------------------ several chunks in lockstep
    @staticmethod
    def _check_lockstep(measures, subset_sizes, start_indices_list):
        """what run_greedy_multi requires of its arguments; ValueError before any device call"""
        n = len(measures)
        if n == 0 or len(subset_sizes) != n or len(start_indices_list) != n:
            raise ValueError("run_greedy_multi needs one subset size and one start list per measure, and at least one measure")
        m0 = measures[0]
        for i, m in enumerate(measures):
            if type(m) is not type(m0):
                raise ValueError("chunks run in lockstep must share their measure: chunk 0 is {}, chunk {} is {}"
                                 .format(type(m0).__name__, i, type(m).__name__))
            if m.average_method != m0.average_method:
                raise ValueError("chunks run in lockstep must share their average_method: chunk 0 has {!r}, chunk {} has {!r}"
                                 .format(m0.average_method, i, m.average_method))
        if len({id(m) for m in measures}) != n:
            raise ValueError("the same measure object appears twice: every chunk needs its own")

    @staticmethod
    def run_greedy_multi(measures, subset_sizes, start_indices_list, verbose=False):
        """run_greedy for several independent exact-greedy measures (one per chunk) with ONE kernel launch per pick
        (acav_mi_run_exact_multi).  Element i of the result is, bit for bit, what
        measures[i].run_greedy(subset_sizes[i], start_indices_list[i]) returns (the timelapse holds equal shares of the
        call's wall time), and every measure's candidate list shrinks by its picks.  All measures are of one class with one
        average_method (ValueError otherwise, before any device call); at most 64 per call.  No CELF, no forced positions
        and no traces: those stay with run_greedy."""
        EfficientMI._check_lockstep(measures, subset_sizes, start_indices_list)
        n = len(measures)
        cands = [m.candidate_ids for m in measures]
        starts = [list(s) for s in start_indices_list]
        niters = [max(0, min(int(sub) - 1 - len(s), len(c))) for sub, s, c in zip(subset_sizes, starts, cands)]
        S = [np.empty(it + 1, np.int64) for it in niters]
        G = [np.empty(it + 1, np.float64) for it in niters]

        def parr(ptrs):
            return (C.c_void_p * n)(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])

        L = np.array([len(c) for c in cands], np.int64)
        ns = np.array([len(s) for s in starts], np.int32)
        sub = np.array([int(s) for s in subset_sizes], np.int64)
        nsel = np.zeros(n, np.int64)
        t0 = time.time()
        _lib.check(_lib._lib.acav_mi_run_exact_multi(parr([m._h for m in measures]), n, parr([_lib.ptr(c) for c in cands]),
                                                     _lib.ptr(L), _lib.ptr(ns), _lib.ptr(sub), parr([_lib.ptr(a) for a in S]),
                                                     parr([_lib.ptr(a) for a in G]), _lib.ptr(nsel)))
        elapsed = time.time() - t0
        if verbose:
            print("Time Consumed: {} seconds for {} chunks in lockstep".format(elapsed, n))
        out = []
        for i, m in enumerate(measures):
            k = int(nsel[i])
            picks = S[i][:k].tolist()
            picked = set(picks)
            if picked:  # the candidate list shrinks as in _run
                m.candidate_ids = np.ascontiguousarray([c for c in cands[i].tolist() if c not in picked], np.int64)
            out.append((starts[i] + picks, G[i][:k].tolist(), [elapsed / max(k, 1)] * k, [0] * k))
        return out


class EfficientMemMI(EfficientMI):
    """mi.py:284-412: the memory-lean formulation of the same greedy; identical here."""


# generalized_mean (mi.py:201-209): the normaliser of the two entropies -> acav_mi_set_average_method
AVERAGE_METHODS = {'arithmetic': 0, 'max': 1, 'min': 2}


class EfficientAMI(EfficientMI):
    """adjusted MI (mi.py:212-259; 'ami' in measures/__init__.py:5-14): the exact greedy on
    (MI - EMI) / max(normaliser - EMI, eps), EMI being the reference's own one-term-per-cell expression (calc_EMI).
    Same kernel as `mi` with the adjusted score (acav_mi_set_measure); float64 over integer counts, within 4e-7 relative of
    the reference's fp32 scores (tests/golden/mi_ami_*.npz).  average_method (generalized_mean, mi.py:201-209): the
    normaliser is the 'arithmetic' mean (the reference default), the 'max' or the 'min' of the two entropies.
    Pair weights are accepted and ignored, with a warning: the reference's calc_AMI replaces the weighted _calc_score."""
    _measure_id = 1
    _takes_weights = False

    def __init__(self, assignments, measure_type='mutual_info', average_method='arithmetic', ncentroids=20,
                 device='cuda', **kwargs):
        method = str(average_method).lower()
        if method not in AVERAGE_METHODS:
            raise ValueError("average_method must be one of {}, got {!r}".format(sorted(AVERAGE_METHODS), average_method))
        super().__init__(assignments, measure_type=measure_type, average_method=method, ncentroids=ncentroids,
                         device=device, **kwargs)

    def init(self, clustering_combinations, candidates):
        EfficientMI.init(self, clustering_combinations, candidates)
        _lib.check(_lib._lib.acav_mi_set_measure(self._h, self._measure_id))
        _lib.check(_lib._lib.acav_mi_set_average_method(self._h, AVERAGE_METHODS[self.average_method]))


class EfficientNMI(EfficientAMI):
    """normalised MI (mi.py:262-271): the exact greedy on 2 MI / max(normaliser, eps).  The reference defines the class but
    its registry (measures/__init__.py:5-14) does not name it; here it is reachable as 'nmi'.  Same kernel, score 2
    (acav_mi_set_measure); float64 over integer counts, pinned on the reference class's own run (tests/golden/mi_nmi_*.npz).
    average_method as for EfficientAMI."""
    _measure_id = 2


class ConstantMeasure(EfficientMI):
    """mi.py:274-281: every candidate scores 1, so the exact greedy takes the first remaining candidate every iteration and
    every gain is 1.0 -- the reference's "no measure" control ('constant' here; not in the reference's registry either)."""
    _takes_weights = False

    def init(self, clustering_combinations, candidates):
        super().init(clustering_combinations, candidates)
        _lib.check(_lib._lib.acav_mi_set_measure(self._h, 3))
