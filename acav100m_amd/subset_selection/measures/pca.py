"""The PCA selection measures -- the paper's PCA baseline (the reference's correspondence_retrieval/code/measures/pca.py:
PCAOptim): every clip is scored by how well its views agree in PCA space, the subset_size clips of largest score are kept.

Definition, for D projected views y_c [V, p] fp32 and P clustering pairs (c1, c2); a = y_c1[v], b = y_c2[v]:
  inner_product      (pca, pca_ip)  sum_j a_j b_j
  cosine_similarity  (pca_cs)       sum_j a_j b_j / (max(|a|, 1e-8) max(|b|, 1e-8))
  euclidean_diff_l1  (pca_l1)       -sum_j |a_j - b_j|
  euclidean_diff_l2  (pca_l2)       -sum_j (a_j - b_j)^2
  score[v] = (the distances of the pairs, added in pair order) / float(P)
every operation one rounded fp32 operation, every sum one chain over j ascending (acav_pair_scores; include/acav_hip.h).
ids = the k clips of largest score in descending order, -0.0 == +0.0, ties to the lower clip index (acav_rank_desc; torch.topk
leaves the tie order open).  S = ids, GAIN[0] = score[ids[0]], GAIN[j] = score[ids[j]] + score[ids[j-1]] (the reference adds the
PREVIOUS score, not a running total), LOOKUPS = [0] * k.  A score that is not finite is refused.  There is no CPU path."""
import ctypes as C
import time

import numpy as np

from ... import _lib
from ...clustering.sgd_clustering import _device_index

DISTANCES = {
    'pca': 'inner_product',
    'pca_ip': 'inner_product',
    'pca_cs': 'cosine_similarity',
    'pca_l1': 'euclidean_diff_l1',
    'pca_l2': 'euclidean_diff_l2',
}
# acav_hip.h: ACAV_PAIR_INNER_PRODUCT, ACAV_PAIR_COSINE, ACAV_PAIR_L1, ACAV_PAIR_L2
DISTANCE_CODES = {'inner_product': 0, 'cosine_similarity': 1, 'euclidean_diff_l1': 2, 'euclidean_diff_l2': 3}


def _pair_list(pairing):
    """clustering pairs -> int32 [P, 2]; a group of another size than two (a `diagonal` layer that one view lacks) is refused"""
    if isinstance(pairing, dict):
        raise ValueError("the pca measures take no pair weights (clustering.weight_type)")
    pairs = [tuple(int(c) for c in pair) for pair in pairing]
    if not pairs or any(len(pair) != 2 for pair in pairs):
        raise ValueError("the pca measures need a non-empty list of clustering PAIRS, got {}".format(list(pairing)))
    return np.ascontiguousarray(pairs, dtype=np.int32)


def pair_scores(views, pairs, distance, device="cuda"):
    """acav_pair_scores on device tensors views[c] [V, p] (contiguous fp32, one device) -> the device score vector [V]"""
    import torch
    V, p = (int(s) for s in views[0].shape)
    for y in views:
        if tuple(y.shape) != (V, p):
            raise ValueError("the projected views differ in shape: {} and {}".format((V, p), tuple(y.shape)))
    pairs = _pair_list(pairs)
    dev = views[0].device
    scores = torch.empty(V, dtype=torch.float32, device=dev)
    table = (C.c_void_p * len(views))(*[y.data_ptr() for y in views])
    torch.cuda.synchronize(dev)  # whatever torch still has queued for the views lands first
    lib = _lib.load_library()
    _lib.check(lib.acav_pair_scores(dev.index, C.cast(table, C.c_void_p), len(views), V, p, _lib.ptr(pairs), len(pairs),
                                    DISTANCE_CODES[distance], _lib.ptr(scores), None))
    return scores


def rank_desc(scores, k):
    """acav_rank_desc: -> (ids int64 [k], top fp32 [k]) on the scores' device"""
    import torch
    n, k = int(scores.shape[0]), int(k)
    if not 0 <= k <= n:
        raise ValueError("cannot take the best {} of {} clips".format(k, n))
    ids = torch.empty(k, dtype=torch.int64, device=scores.device)
    top = torch.empty(k, dtype=torch.float32, device=scores.device)
    torch.cuda.synchronize(scores.device)
    lib = _lib.load_library()
    _lib.check(lib.acav_rank_desc(scores.device.index, _lib.ptr(scores), n, k, _lib.ptr(ids) if k else None,
                                  _lib.ptr(top) if k else None, None))
    return ids, top


class PCAOptim:
    """pcas: {key: [V, p]} or a list of [V, p] arrays -- numpy, or torch tensors on the host or the device -- in clustering
    order (a dict: in the order of its keys as given); measure_type: one of DISTANCE_CODES (None: the class's own, which the
    registry's names set: bound())."""
    measure_type = 'inner_product'

    def __init__(self, pcas, measure_type=None, device="cuda", **_ignored):
        import torch
        if measure_type is not None:
            self.measure_type = measure_type
        if self.measure_type not in DISTANCE_CODES:
            raise ValueError("measure_type {!r}: one of {}".format(self.measure_type, sorted(DISTANCE_CODES)))
        mats = list(pcas.values()) if isinstance(pcas, dict) else list(pcas)
        if not mats:
            raise ValueError("no projected views")
        on_device = [m for m in mats if hasattr(m, "is_cuda") and m.is_cuda]
        if on_device:
            self.device = on_device[0].device
        else:
            if str(device) == "cpu" or not torch.cuda.is_available():
                raise _lib.AcavError("the pca measures score on the GPU (there is no CPU path)")
            self.device = torch.device("cuda:{}".format(_device_index(device)))
        self.views = []
        for m in mats:
            if not hasattr(m, "data_ptr"):
                m = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))
            m = m.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if m.dim() != 2:
                raise ValueError("a projected view is a [V, p] matrix, got shape {}".format(tuple(m.shape)))
            self.views.append(m)
        self.pairs = None
        self.candidates = None

    def init(self, clustering_combinations, candidates=None):
        """candidates: kept for the reference's surface; every clip is scored and ranked, as there"""
        self.pairs = _pair_list(clustering_combinations)
        self.candidates = candidates
        return self

    def score_all(self):
        assert self.pairs is not None, "init(clustering_combinations, candidates) first"
        return pair_scores(self.views, self.pairs, self.measure_type)

    def calc_measure(self, subset_size):
        """-> (scores, ids): the subset_size largest scores, descending, and their clips (device tensors)"""
        scores = self.score_all()
        ids, top = rank_desc(scores, subset_size)
        return top, ids

    def run(self, subset_size, start_indices=None, intermediate_target=None, celf_ratio=0, **_ignored):
        """-> (S, GAIN, timelapse, LOOKUPS); start_indices and intermediate_target are ignored, as in the reference"""
        if celf_ratio:
            raise ValueError("celf_ratio={!r}: the pca measures rank once, there is no greedy loop to make lazy".format(celf_ratio))
        tic = time.time()
        top, ids = self.calc_measure(subset_size)
        S = [int(i) for i in ids.cpu().tolist()]
        top = [float(s) for s in top.cpu().tolist()]
        GAIN = [top[j] if j == 0 else top[j] + top[j - 1] for j in range(len(top))]
        timelapse = [time.time() - tic] * len(S)
        return S, GAIN, timelapse, [0] * len(S)

    run_greedy = run  # the name the greedy measures' drivers call


def bound(name):
    """the class a registry name stands for: PCAOptim with that name's distance as its default measure_type"""
    return type('PCAOptim_' + name, (PCAOptim,), {'measure_type': DISTANCES[name], '__doc__': PCAOptim.__doc__})
