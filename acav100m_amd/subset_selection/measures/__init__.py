"""Measure registry: the names the reference's `get_measure` knows (subset_selection/code/measures/__init__.py:5-14).

'batch_mi' is the pipeline default (config.py:45); 'mi' and 'mem_mi' are the exact-greedy measures (SURVEY.md 8(f)
rank 2) and 'ami' their adjusted-MI variant (mi.py:212-259), 'contrastive' the baseline selector;
'nmi' / 'constant' are the reference's EfficientNMI / ConstantMeasure (mi.py:262-281), which its registry leaves out.
'fm' / 'rand' / 'arand' are the pair-counting scores of the reference's correspondence_retrieval stage (efficient_pair.py),
also under the names its supplement grid uses (search_targets/supplements/scores.json: efficient_fm, efficient_rand,
efficient_arand).
'pca' / 'pca_ip' / 'pca_cs' / 'pca_l1' / 'pca_l2' are that stage's PCA baseline (measures/pca.py: PCAOptim) with its four distances;
they read projected FEATURES, not cluster assignments (run_pca.py).
"""
from .batch import EfficientBatchMI
from .contrastive import Contrastive
from .mi import ConstantMeasure, EfficientAMI, EfficientMI, EfficientMemMI, EfficientNMI
from .pca import DISTANCES as _PCA_DISTANCES, PCAOptim, bound as _pca
from .pair import AdjustedRandScore, FowlkesMallowsScore, RandScore

_REGISTRY = {
    'batch_mi': EfficientBatchMI,
    'mi': EfficientMI,
    'mem_mi': EfficientMemMI,
    'ami': EfficientAMI,
    'nmi': EfficientNMI,            # classes of the reference (mi.py:262-281) that its own registry does not name
    'constant': ConstantMeasure,
    'contrastive': Contrastive,
    'fm': FowlkesMallowsScore,      # correspondence_retrieval/code/measures/efficient_pair.py
    'rand': RandScore,
    'arand': AdjustedRandScore,
    'efficient_fm': FowlkesMallowsScore,
    'efficient_rand': RandScore,
    'efficient_arand': AdjustedRandScore,
}
# The measures over projected FEATURES (correspondence_retrieval/code/measures/pca.py) -- a table of their own: _REGISTRY holds
# the measures over an assignment matrix, whose drivers (run_greedy, the lockstep groups) do not apply to these (run_pca.py).
_FEATURE_REGISTRY = {name: _pca(name) for name in _PCA_DISTANCES}
PCA_MEASURES = tuple(_PCA_DISTANCES)


def get_measure(measure_name):
    key = measure_name.lower()
    assert key in _REGISTRY or key in _FEATURE_REGISTRY, "no measure named {}".format(measure_name)
    return _REGISTRY[key] if key in _REGISTRY else _FEATURE_REGISTRY[key]
