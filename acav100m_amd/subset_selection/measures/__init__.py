"""Measure registry: the names the reference's `get_measure` knows (subset_selection/code/measures/__init__.py:5-14).

'batch_mi' is the pipeline default (config.py:45); 'mi' and 'mem_mi' are the exact-greedy measures (SURVEY.md 8(f)
rank 2) and 'ami' their adjusted-MI variant (mi.py:212-259), 'contrastive' the baseline selector;
'nmi' / 'constant' are the reference's EfficientNMI / ConstantMeasure (mi.py:262-281), which its registry leaves out.
'fm' / 'rand' / 'arand' are the pair-counting scores of the reference's correspondence_retrieval stage (efficient_pair.py),
also under the names its supplement grid uses (search_targets/supplements/scores.json: efficient_fm, efficient_rand,
efficient_arand).
"""
from .batch import EfficientBatchMI
from .contrastive import Contrastive
from .mi import ConstantMeasure, EfficientAMI, EfficientMI, EfficientMemMI, EfficientNMI
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


def get_measure(measure_name):
    key = measure_name.lower()
    assert key in _REGISTRY, "no measure named {}".format(measure_name)
    return _REGISTRY[key]
