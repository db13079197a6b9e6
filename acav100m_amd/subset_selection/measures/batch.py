"""EfficientBatchMI -- drop-in for subset_selection/code/measures/batch.py:10-260 (on top of
EfficientMI, measures/mi.py:14-148).

Same constructor / init / run_greedy surface as the reference so run_greedy._run_greedy
(run_greedy.py:31-53) drives it unchanged.  The contingency tables, the per-iteration
permutation of the candidate list (torch.randperm semantics on the same MT19937 stream), the
delta-MI scoring, top-k, cache update and re-queue all run on the GPU inside libacav_hip.so; see
acav100m_amd/csrc/acav_mi.hip.  No CPU path.
"""
import ctypes as C
import math
import time
import warnings

import numpy as np

from ... import _lib
from ...rng import default_generator


def _device_index(device):
    s = str(device)
    if s == "cpu":
        raise _lib.AcavError("acav100m_amd EfficientBatchMI has no CPU path: use device='cuda'")
    if ":" in s:
        return int(s.split(":")[1])
    try:
        import torch
        return torch.cuda.current_device()
    except Exception:
        return 0


# the scores of a given subset (score_subset), in the order of the library's ACAV_SCORE_* bits; the names are sklearn's
# (sklearn.metrics.<name>_score).  They are scores of a finished selection, not selection measures: get_measure does not know them.
SCORE_NAMES = ('mutual_info', 'normalized_mutual_info', 'adjusted_mutual_info', 'adjusted_rand', 'fowlkes_mallows', 'rand')
# acav_score_stats of include/acav_hip.h
SCORE_STATS_DTYPE = np.dtype([('mi', 'f8'), ('h_row', 'f8'), ('h_col', 'f8'), ('emi', 'f8'), ('tp', 'i8'), ('fp', 'i8'),
                              ('fn', 'i8'), ('tn', 'i8'), ('n_rows', 'i8'), ('n_cols', 'i8'), ('n', 'i8')])


def score_mask(measures=None):
    """names -> (tuple of names in library order without repeats, bit mask); None = all six.  ValueError for an unknown name
    or an empty list -- before anything touches a device."""
    if measures is None:
        measures = SCORE_NAMES
    if isinstance(measures, str):
        measures = [m for m in measures.split(',') if m]
    names = [str(m).strip().lower() for m in measures]
    unknown = [m for m in names if m not in SCORE_NAMES]
    if unknown:
        raise ValueError("unknown subset score(s) {}: choose from {}".format(unknown, list(SCORE_NAMES)))
    if not names:
        raise ValueError("no subset score asked for: choose from {}".format(list(SCORE_NAMES)))
    mask = 0
    for m in names:
        mask |= 1 << SCORE_NAMES.index(m)
    return tuple(m for m in SCORE_NAMES if m in names), mask


def compose_scores(stats):
    """one pair's raw values (a SCORE_STATS_DTYPE record or a dict of its fields) -> {name: score}: the host-only
    acav_score_compose, usable without a GPU"""
    rec = np.zeros(1, SCORE_STATS_DTYPE)
    for f in SCORE_STATS_DTYPE.names:
        rec[f] = stats[f]
    out = np.empty(len(SCORE_NAMES), np.float64)
    _lib.check(_lib.load_library().acav_score_compose(_lib.ptr(rec), _lib.ptr(out)))
    return dict(zip(SCORE_NAMES, out.tolist()))


# how batch_mi draws an iteration's batch (batch.sampler)
SAMPLERS = ('permutation', 'draw')


def draw_form(L, subset, B, k, keep_unselected, max_iters=-1, pmax=1, dmax=2, weighted=False):
    """what a sampler='draw' selection of this shape launches, without a GPU (acav_mi_draw_form): L, subset: one entry per
    chunk.  -> dict; a refused shape has 'code' != 0 (-5: a list falls below a batch; -1: the LDS does not fit)."""
    L = np.ascontiguousarray(np.atleast_1d(L), dtype=np.int64)
    sub = np.ascontiguousarray(np.atleast_1d(subset), dtype=np.int64)
    n = len(L)
    form = np.zeros(16 + 2 * n, np.int64)
    _lib.check(_lib.load_library().acav_mi_draw_form(n, _lib.ptr(L), _lib.ptr(sub), int(B), int(k), int(bool(keep_unselected)),
                                                      int(max_iters), int(pmax), int(dmax), int(bool(weighted)), _lib.ptr(form)))
    names = ('code', 'refusal', 'chunk', 'left', 'step', 'wide', 'mode', 'lds', 'group', 'group_max', 'launches', 'iters_max',
             'sel_lds', 'threads')
    out = {name: int(form[i]) for i, name in enumerate(names)}
    out['iters'], out['draws'] = form[16:16 + n].tolist(), form[16 + n:16 + 2 * n].tolist()
    return out


class EfficientBatchMI:
    """ this implementation requires the users to use the same ncentroids for all clusterings """
    _takes_weights = True  # the MI score multiplies by the pair weights; the measures that override it ignore them

    def __init__(self, assignments, measure_type='mutual_info', average_method='arithmetic',
                 ncentroids=20, batch_size=1, selection_size=1, device='cpu', keep_unselected=False,
                 generator=None, sampler='permutation', **kwargs):
        """sampler (ours): 'permutation' (default) shuffles the whole candidate list every iteration on the reference's generator
        stream; 'draw' performs only the first batch_size steps of that shuffle (acav_mi_run_draw) -- the same distribution of
        every batch for O(batch_size) instead of O(candidates) work per iteration, on a generator stream of its own."""
        if sampler not in SAMPLERS:
            raise ValueError("sampler={!r}: choose from {}".format(sampler, list(SAMPLERS)))
        self.sampler = sampler
        self.average_method = average_method.lower()
        self.ncentroids = int(ncentroids)
        self.assignments = np.ascontiguousarray(assignments, dtype=np.int64)  # V x D
        self.eps = np.finfo('float64').eps
        self.B = batch_size
        self.k = selection_size
        self.device = device
        self.keep_unselected = keep_unselected
        self._generator = generator if generator is not None else default_generator
        self._h = None
        self.trace = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:  # module globals die first at interpreter exit
            _lib._lib.acav_mi_destroy(h)

    # ------------------------------------------------------------------ init (mi.py:27-39)
    def init(self, clustering_combinations, candidates):
        """clustering_combinations: the pair list, or the reference's weighted form {'pairing': pairs, 'weights': one float
        per pair} (correspondence_retrieval measures/efficient.py:29-33, pairing.get_cluster_pairing with a weight_type):
        every pair's score is multiplied by its weight, rounded to fp32, before the mean over the pairs."""
        self.pair_weights = None
        if isinstance(clustering_combinations, dict):
            self.combinations = clustering_combinations['pairing']
            self.pair_weights = list(clustering_combinations['weights'])
            if not self._takes_weights:
                warnings.warn("{} does not weight its pairs (the reference's class overrides _calc_score): the pair weights "
                              "are ignored".format(type(self).__name__), UserWarning, stacklevel=2)
        else:
            self.combinations = clustering_combinations
        self.init_cache()
        self.init_candidates(candidates)

    def init_cache(self):
        lib = _lib.load_library()
        if self._h is not None:
            lib.acav_mi_destroy(self._h)
            self._h = None
        # the reference only ever uses columns 0 and 1 of a combination (pair_ids[:, 0], pair_ids[:, 1], batch.py:47-48):
        # bipartite pairing over three or more model groups yields longer tuples
        combos = [tuple(c) for c in self.combinations]
        if not combos or any(len(c) < 2 for c in combos):
            raise ValueError("every clustering combination needs at least two clustering indices, got {}".format(combos[:4]))
        pairs = np.ascontiguousarray([c[:2] for c in combos], dtype=np.int32)
        self._npairs = len(pairs)
        v, d = self.assignments.shape
        h = C.c_void_p()
        _lib.check(lib.acav_mi_create(C.byref(h), _device_index(self.device), _lib.ptr(self.assignments), v, d,
                                      self.ncentroids, _lib.ptr(pairs), len(pairs), None))
        self._h = h
        weights = getattr(self, 'pair_weights', None)
        if weights is not None and self._takes_weights:
            # torch.tensor(self.pair_weights).float() (efficient.py:98): float64 -> fp32, round to nearest
            w32 = np.ascontiguousarray(np.asarray(weights, np.float64).astype(np.float32))
            if w32.shape != (len(pairs),):
                raise ValueError("{} pair weights for {} clustering pairs".format(w32.size, len(pairs)))
            _lib.check(lib.acav_mi_set_pair_weights(h, _lib.ptr(w32), len(pairs)))

    def init_candidates(self, candidates):
        self.candidate_ids = np.ascontiguousarray(candidates, dtype=np.int64)

    @property
    def cache(self):
        """{'N','a','b','n'} integer contingency tables (the reference holds them as fp32 + eps)."""
        p, c = self._npairs, self.ncentroids
        N = np.empty((p, c, c), np.int32)
        a = np.empty((p, c), np.int32)
        b = np.empty((p, c), np.int32)
        n = C.c_int64(0)
        _lib.check(_lib._lib.acav_mi_get_counts(self._h, _lib.ptr(N), _lib.ptr(a), _lib.ptr(b), C.byref(n)))
        return {'N': N, 'a': a, 'b': b, 'n': n.value}

    def add_samples(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        _lib.check(_lib._lib.acav_mi_add_samples(self._h, _lib.ptr(ids), len(ids)))

    def score_batch(self, ids):
        """scores.mean(-1) of operate_block for the given candidate ids (batch.py:123-130,144)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        out = np.empty(len(ids), np.float64)
        _lib.check(_lib._lib.acav_mi_score_batch(self._h, _lib.ptr(ids), len(ids), _lib.ptr(out)))
        return out

    def score_subset(self, ids, measures=None, prefixes=None, per_pair=False, return_stats=False):
        """How well the clusterings agree on the clips `ids` (repeats count as often as they occur): sklearn's scores of
        every clustering pair's two label columns restricted to ids, averaged over the pairs without weights --
        MutualInformation.get_measure (correspondence_retrieval/code/measures/mutual_information.py:74-85).  Usable after
        init(); it leaves the tables, the measure and the generator of the handle alone.
        measures: names out of SCORE_NAMES (default: all six).  prefixes: strictly increasing sizes; the result then holds one
        value per prefix ids[:k] (a trailing len(ids) is added when missing), arrays instead of floats.
        -> {name: float | array [len(prefixes)]}; per_pair=True adds 'per_pair': {name: array [..., P]}, return_stats=True
        adds 'stats': the raw values per (prefix, pair) (SCORE_STATS_DTYPE)."""
        names, mask = score_mask(measures)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.ndim != 1 or len(ids) < 1:
            raise ValueError("score_subset needs a non-empty list of clip ids")
        if self._h is None:
            raise _lib.AcavError("score_subset before init(): the handle does not exist yet")
        curve = prefixes is not None
        pre = np.ascontiguousarray(list(prefixes) if curve else [len(ids)], dtype=np.int64)
        if curve and (len(pre) == 0 or pre[-1] != len(ids)):
            pre = np.append(pre, len(ids)).astype(np.int64)
        if len(pre) > 1 and np.any(np.diff(pre) <= 0) or pre[0] < 1:
            raise ValueError("prefixes must increase strictly from at least 1 to at most len(ids)")
        q, p = len(pre), self._npairs
        scores = np.empty((q, len(SCORE_NAMES)), np.float64)
        pp = np.empty((q, len(SCORE_NAMES), p), np.float64) if per_pair else None
        stats = np.zeros((q, p), SCORE_STATS_DTYPE) if return_stats else None
        _lib.check(_lib._lib.acav_mi_score_subset(self._h, _lib.ptr(ids), len(ids), _lib.ptr(pre), q, mask, _lib.ptr(scores),
                                                  _lib.ptr(pp), _lib.ptr(stats)))
        nq = q if curve and len(prefixes) == q else q - 1 if curve else 1

        def pick(a):
            return a[:nq].copy() if curve else a[0].copy() if a.ndim > 1 else float(a[0])

        out = {m: pick(scores[:, SCORE_NAMES.index(m)]) for m in names}
        if per_pair:
            out['per_pair'] = {m: pick(pp[:, SCORE_NAMES.index(m), :]) for m in names}
        if return_stats:
            out['stats'] = stats[:nq] if curve else stats[0]
        return out

    def get_batch_ranges(self):
        return [[0, self.B]]  # batch.py:56-87: the O(1) scoring never needs GPU-memory chunking

    def modify_k(self, subset_size):
        """batch.py:173-188"""
        D = self.assignments.shape[0]
        S, K, B = subset_size, self.k, self.B
        term = B * S / D
        if K < term and not self.keep_unselected:
            print("k={} is too small to get {} samples from {} datapoints with batch_size {}".format(K, S, D, B))
            K = math.ceil(term)
            print("resizing k to {}".format(K))
        return K

    # ---------------------------------------------------------- run_greedy (batch.py:195-260)
    def run_greedy(self, subset_size, start_indices, intermediate_target=None, verbose=False, log_every=1,
                   log_times=None, node_rank=None, pid=None, record_trace=False, forced_pos=None,
                   max_iters=-1):
        print('using {} blocks per iter for gpu computation'.format(len(self.get_batch_ranges())))
        self.k = self.modify_k(subset_size)
        B, k = int(self.B), int(self.k)
        start = np.ascontiguousarray(start_indices, dtype=np.int64)
        cand = self.candidate_ids
        niters = math.ceil(subset_size / k) if max_iters < 0 else min(math.ceil(subset_size / k), int(max_iters))
        S = np.empty(niters * k + k, np.int64)
        G = np.empty(niters * k + k, np.float64)
        tr_ids = np.empty((niters, B), np.int64) if record_trace else None
        tr_sc = np.empty((niters, B), np.float64) if record_trace else None
        tr_pos = np.empty((niters, k), np.int32) if record_trace else None
        fp = None if forced_pos is None else np.ascontiguousarray(forced_pos, dtype=np.int32)
        if self.sampler == 'draw' and fp is not None:
            raise ValueError("forced_pos replays a trace of the permutation sampler: sampler='draw' has no teacher forcing")
        nsel, nit = C.c_int64(0), C.c_int64(0)
        greedy_start_time = time.time()
        if self.sampler == 'draw':
            nsel, nit = self._run_draw([self], [subset_size], [start], [S], [G], [(tr_ids, tr_sc, tr_pos)], max_iters)[0]
            nsel, nit = C.c_int64(nsel), C.c_int64(nit)
        else:
            _lib.check(_lib._lib.acav_mi_run_greedy(
                self._h, _lib.ptr(cand), len(cand), _lib.ptr(start), len(start), int(subset_size), B, k,
                int(bool(self.keep_unselected)), self._generator.handle, _lib.ptr(S), _lib.ptr(G), C.byref(nsel),
                C.byref(nit), _lib.ptr(tr_ids), _lib.ptr(tr_sc), _lib.ptr(tr_pos), _lib.ptr(fp), int(max_iters)))
        elapsed = time.time() - greedy_start_time
        nit, nsel = nit.value, nsel.value
        if record_trace:
            self.trace = dict(ids=tr_ids[:nit], scores=tr_sc[:nit], pos=tr_pos[:nit])
        S_list = S[:nsel].tolist()  # S = S[:subset_size]  (batch.py:258)
        GAIN = G[:nit * k].tolist()
        timelapse = [elapsed / max(nit, 1)] * nit
        LOOKUPS = [1] * nit
        if verbose:
            msg = "(LEN: {}/{}, MEASURE: {})".format(len(S_list), subset_size,
                                                     float(np.mean(GAIN[-k:])) if GAIN else float('nan'))
            if node_rank is not None:
                msg = 'Node: {}, '.format(node_rank) + msg
            print(msg)
        print("Time Consumed: {} seconds".format(elapsed))
        return (S_list, GAIN, timelapse, LOOKUPS)


    # ------------------------------------------------------------ sampler='draw': one chunk or several
    @staticmethod
    def _run_draw(measures, subset_sizes, starts, S, G, traces, max_iters):
        """acav_mi_run_draw for the measures (a chunk each; they share B, k and keep_unselected), results into the S / G arrays
        and the (ids, scores, pos) trace arrays (or Nones) of every chunk.  -> [(n_selected, n_iters)] per chunk."""
        n = len(measures)
        m0 = measures[0]

        def parr(ptrs):
            return (C.c_void_p * n)(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])

        cands = [m.candidate_ids for m in measures]
        L = np.array([len(c) for c in cands], np.int64)
        ns = np.array([len(s) for s in starts], np.int32)
        sub = np.array([int(s) for s in subset_sizes], np.int64)
        nsel, nit = np.zeros(n, np.int64), np.zeros(n, np.int64)
        _lib.check(_lib._lib.acav_mi_run_draw(
            parr([m._h for m in measures]), n, parr([_lib.ptr(c) for c in cands]), _lib.ptr(L),
            parr([_lib.ptr(s) if len(s) else None for s in starts]), _lib.ptr(ns), _lib.ptr(sub), int(m0.B), int(m0.k),
            int(bool(m0.keep_unselected)), parr([m._generator.handle for m in measures]), parr([_lib.ptr(a) for a in S]),
            parr([_lib.ptr(a) for a in G]), _lib.ptr(nsel), _lib.ptr(nit), parr([_lib.ptr(t[0]) for t in traces]),
            parr([_lib.ptr(t[1]) for t in traces]), parr([_lib.ptr(t[2]) for t in traces]), int(max_iters)))
        return [(int(a), int(b)) for a, b in zip(nsel, nit)]

    # ------------------------------------------------------------ several chunks in lockstep
    @staticmethod
    def run_greedy_multi(measures, subset_sizes, start_indices_list, verbose=False):
        """run_greedy for several independent measures (one per chunk, chunk.py:21-53) with ONE set of kernel
        launches per iteration (acav_mi_run_greedy_multi).  Every measure needs its own generator and must share
        batch_size / selection_size / keep_unselected; element i of the result is what
        measures[i].run_greedy(subset_sizes[i], start_indices_list[i]) returns."""
        n = len(measures)
        assert n > 0 and len(subset_sizes) == n and len(start_indices_list) == n
        m0 = measures[0]
        for m, sub in zip(measures, subset_sizes):
            m.k = m.modify_k(sub)
        B, k = int(m0.B), int(m0.k)
        assert all(int(m.B) == B and int(m.k) == k and bool(m.keep_unselected) == bool(m0.keep_unselected)
                   for m in measures), "chunks run in lockstep must share batch_size / selection_size / keep_unselected"
        assert len({id(m._generator) for m in measures}) == n, "every chunk needs its own generator"
        cands = [m.candidate_ids for m in measures]
        starts = [np.ascontiguousarray(s, dtype=np.int64) for s in start_indices_list]
        niters = [math.ceil(int(s) / k) for s in subset_sizes]
        S = [np.empty(it * k + k, np.int64) for it in niters]
        G = [np.empty(it * k + k, np.float64) for it in niters]

        def parr(ptrs):
            return (C.c_void_p * n)(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])

        h_arr = parr([m._h for m in measures])
        c_arr = parr([_lib.ptr(c) for c in cands])
        s_arr = parr([_lib.ptr(s) if len(s) else None for s in starts])
        r_arr = parr([m._generator.handle for m in measures])
        S_arr = parr([_lib.ptr(a) for a in S])
        G_arr = parr([_lib.ptr(a) for a in G])
        L = np.array([len(c) for c in cands], np.int64)
        ns = np.array([len(s) for s in starts], np.int32)
        sub = np.array([int(s) for s in subset_sizes], np.int64)
        nsel = np.zeros(n, np.int64)
        nit = np.zeros(n, np.int64)
        samplers = {getattr(m, 'sampler', 'permutation') for m in measures}
        assert len(samplers) == 1, "chunks run together must share batch.sampler"
        t0 = time.time()
        if samplers == {'draw'}:  # one launch of n workgroups, a chunk each
            for i, (a, b) in enumerate(EfficientBatchMI._run_draw(measures, subset_sizes, starts, S, G, [(None,) * 3] * n, -1)):
                nsel[i], nit[i] = a, b
        else:
            _lib.check(_lib._lib.acav_mi_run_greedy_multi(h_arr, n, c_arr, _lib.ptr(L), s_arr, _lib.ptr(ns), _lib.ptr(sub), B, k,
                                                          int(bool(m0.keep_unselected)), r_arr, S_arr, G_arr, _lib.ptr(nsel),
                                                          _lib.ptr(nit)))
        elapsed = time.time() - t0
        if verbose:
            print("Time Consumed: {} seconds for {} chunks in lockstep".format(elapsed, n))
        out = []
        for i in range(n):
            it = int(nit[i])
            out.append((S[i][:int(nsel[i])].tolist(), G[i][:it * k].tolist(), [elapsed / max(it, 1)] * it, [1] * it))
        return out
