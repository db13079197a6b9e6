"""Clustering-pair selection -- subset_selection/code/pairing.py:5-41, plus the single-layer pairings and the layer
weights of correspondence_retrieval/code/cluster_pairing.py:7-40 and pair_weights.py:4-50.

keys: the sorted (model_key, layer) tuples of dataloader.format_assignments (dataloader.py:43-53);
returns index pairs into the D columns of the assignment matrix, or -- with a weight_type -- the reference's dict
{'pairing': pairs, 'weights': one float per pair}.
"""
import itertools
from collections import OrderedDict

import numpy as np


def _group_indices(keys, field):
    groups = OrderedDict()
    for idx, key in enumerate(keys):
        groups.setdefault(key[field], []).append(idx)
    return list(groups.values())


def get_combination(keys):
    """every unordered pair of clusterings, audio-audio included (pairing.py:16-20)"""
    return list(itertools.combinations(range(len(keys)), 2))


def get_bipartite(keys):
    """one clustering from every model_key group (pairing.py:23-30)"""
    return list(itertools.product(*_group_indices(keys, 0)))


def get_diagonal(keys):
    """clusterings that share a layer name (pairing.py:33-41)"""
    return _group_indices(keys, 1)


def get_single_layer(keys, layer=-1):
    """the one `diagonal` group of the layer-th sorted layer name (cluster_pairing.py:25-36)"""
    groups = OrderedDict()
    for idx, key in enumerate(keys):
        groups.setdefault(key[1], []).append(idx)
    names = sorted(groups)
    if not -len(names) <= layer < len(names):
        raise ValueError("layer {} out of range: the keys hold {} layer names".format(layer, len(names)))
    return [groups[names[layer]]]


def get_penultimate(keys):
    """cluster_pairing.py:39-40: the fifth layer name"""
    return get_single_layer(keys, layer=4)


_PAIRINGS = {'diagonal': get_diagonal, 'bipartite': get_bipartite, 'combination': get_combination,
             'penultimate': get_penultimate}
_LAYERS = {'layer_{}'.format(i): i for i in range(5)}  # cluster_pairing.py:14


def get_cluster_pairing(keys, cluster_pairing, weight_type=None):
    cluster_pairing = cluster_pairing.lower()
    if cluster_pairing in _LAYERS:
        pairing = get_single_layer(keys, _LAYERS[cluster_pairing])
    else:
        assert cluster_pairing in _PAIRINGS, f"invalid cluster pairing type: {cluster_pairing}"
        pairing = _PAIRINGS[cluster_pairing](keys)
    return get_weights(keys, pairing, weight_type)


# ------------------------------------------------------------------------ layer weights (pair_weights.py:4-50)
_FUNCS = {
    'linear': lambda x: x,
    'log': lambda x: np.log(x),
    'exp': lambda x: np.exp(x),
}


def get_weights(keys, pairing, weight_type=None):
    """pair_weights.py:4-13: n_layer = (largest clustering index + 1) // 2, one weight per layer shared by both views
    (the per-layer vector is concatenated twice), a pair weighs the product of its two clusterings' weights."""
    if weight_type is None:
        return pairing
    n_layer = (int(np.array(pairing).max()) + 1) // 2
    weights = _get_weights(n_layer, weight_type)
    weights = np.concatenate([weights, weights])
    for v in pairing:
        if max(v[0], v[1]) >= len(weights):
            raise ValueError("weight_type {!r}: pair {} indexes clustering {} but the pairing yields {} layer(s) per view "
                             "(indices up to {})".format(weight_type, tuple(v), max(v[0], v[1]), n_layer, 2 * n_layer - 1))
    pairing_weights = [weights[v[0]] * weights[v[1]] for v in pairing]
    if not np.isfinite(np.array(pairing_weights, np.float64)).all() or \
            not np.isfinite(np.array(pairing_weights, np.float32)).all():
        raise ValueError("weight_type {!r} gives non-finite pair weights: {}".format(weight_type, pairing_weights))
    return {'pairing': pairing, 'weights': pairing_weights}


def _get_weights(n_layer, weight_type):
    """pair_weights.py:16-50: `linear|log|exp[_<coeff>]` -> f((x coeff + 1) - min + 2) / median, x = the layer index
    centred on (1 + n_layer) / 2; `onehot_<i>` -> the 0/1 vector of layer i, not normalised."""
    parts = str(weight_type).split('_')
    func_name = parts[0]
    if func_name == 'onehot':
        if len(parts) != 2:
            raise ValueError("weight_type {!r}: onehot needs a layer index, e.g. onehot_4".format(weight_type))
        i = int(parts[1])
        if not -n_layer <= i < n_layer:
            raise ValueError("weight_type {!r}: layer {} out of range for {} layer(s)".format(weight_type, i, n_layer))
        weights = np.array([float(0)] * n_layer)
        weights[i] = 1
        return weights
    if func_name not in _FUNCS:
        raise ValueError("weight_type {!r}: unknown function {!r} (one of {} or onehot)".format(
            weight_type, func_name, sorted(_FUNCS)))
    coeff = 1.0
    if len(parts) == 2:
        coeff = float(parts[1])
    mean = (1 + n_layer) / 2
    x = np.arange(float(n_layer)) - mean
    weights = x * coeff + 1
    minv = weights.min()
    weights = weights - minv + 2  # for log stabilization
    with np.errstate(over='ignore', invalid='ignore'):
        weights = _FUNCS[func_name](weights)
        weights = weights / np.median(weights)
    return weights
