"""Driver of one selection: the public functions of subset_selection/code/run_greedy.py (`_run_greedy`, `run_greedy`,
same positional arguments) on top of the GPU measures.

Plan of a run (reference run_greedy.py:9-74):
  C            = max label + 1                      (not K: labels never used by a clustering are not counted)
  subset size  = given, or round(ratio * V)
  B, k         = batch.batch_size clamped to V - 1, batch.selection_size clamped to B
  candidates   = 0..V-1, shuffled with Python's `random` when asked; the first one becomes the start index
  measure      = get_measure(name)(...); measure.init(pairs, candidates); measure.run_greedy(...)
  celf_ratio   = share of the picks an exact-greedy measure takes lazily (CELF; correspondence_retrieval's celf_ratio)
  weight_type  = None, or a layer weighting of the pairs (pairing.get_weights; correspondence_retrieval's weight_type) for
                 the measures that weight their pairs (WEIGHTED_MEASURES)
`_prepare` builds everything up to the measure call so that several chunks can be prepared first and then selected
in lockstep (run.py).
"""
import numpy as np

from .measures import get_measure
from .measures.batch import SAMPLERS  # batch.sampler: how batch_mi draws an iteration's batch
from .pairing import get_cluster_pairing

# the measures whose score the pair weights scale (correspondence_retrieval: EfficientMI / EfficientMemMI / EfficientBatchMI);
# the others override the weighted _calc_score there, so a weight_type would be dropped without a word
WEIGHTED_MEASURES = ('mi', 'mem_mi', 'batch_mi')


def check_weight_type(measure_name, weight_type):
    if weight_type is not None and str(measure_name).lower() not in WEIGHTED_MEASURES:
        raise ValueError("clustering.weight_type={!r} needs one of the measures {}, not {!r}: the others ignore pair weights"
                         .format(weight_type, list(WEIGHTED_MEASURES), measure_name))


# the measures that cannot run CELF: the reference asserts efficient_greedy for celf_ratio and its batch measure drops the value
NO_CELF_MEASURES = ('batch_mi', 'contrastive', 'pca', 'pca_ip', 'pca_cs', 'pca_l1', 'pca_l2')  # (pca*: one ranking, no greedy loop)


def check_celf_ratio(measure_name, celf_ratio):
    ratio = 0 if celf_ratio is None else celf_ratio
    if not 0 <= ratio <= 1:
        raise ValueError("celf_ratio must lie in [0, 1], got {!r}".format(celf_ratio))
    if ratio != 0 and str(measure_name).lower() in NO_CELF_MEASURES:
        raise ValueError("celf_ratio={!r} needs an exact-greedy measure, not {!r}: it has no lazy variant"
                         .format(celf_ratio, measure_name))
    return ratio


def check_sampler(measure_name, sampler):
    """-> the sampler's name ('permutation' for None); ValueError for an unknown one, and for 'draw' with any measure but
    batch_mi (the exact measures draw nothing, the others have no batch)"""
    name = 'permutation' if sampler is None else sampler
    if name not in SAMPLERS:
        raise ValueError("batch.sampler={!r}: choose from {}".format(sampler, list(SAMPLERS)))
    if name == 'draw' and str(measure_name).lower() != 'batch_mi':
        raise ValueError("batch.sampler='draw' needs measure_name=batch_mi, not {!r}: only its greedy loop draws batches"
                         .format(measure_name))
    return name


def batch_sampler(args):
    """batch.sampler of a configuration; the key has no entry in the defaults and reads as None ('permutation') when missing"""
    batch = args.batch
    return batch.get('sampler') if hasattr(batch, 'get') else getattr(batch, 'sampler', None)


class _Plan:
    """sizes of one selection, derived once from the assignment matrix and the `batch` options"""

    def __init__(self, args, assignments, subset_size, subset_ratio):
        self.rows = int(assignments.shape[0])
        self.ncentroids = int(assignments.max()) + 1
        self.subset = round(subset_ratio * self.rows) if subset_size is None else subset_size
        self.batch = min(args.batch.batch_size, self.rows - 1)
        self.select = min(args.batch.selection_size, self.batch)

    def candidate_order(self, shuffle):
        if shuffle:
            print("shuffling candidates")
            from ..rng import python_shuffled_range
            return python_shuffled_range(self.rows)  # random.shuffle: Python's generator, not torch's (run_greedy.py:40)
        return np.arange(self.rows, dtype=np.int64)


def _prepare(args, assignments, clustering_types, subset_size, subset_ratio, measure_name='mi',
             cluster_pairing='combination', shuffle_candidates=True, verbose=False, generator=None, weight_type=None, celf_ratio=0):
    """-> (measure ready to run, start_indices, subset_size)"""
    sampler = check_sampler(measure_name, batch_sampler(args))  # before any device work, like the two below
    check_weight_type(measure_name, weight_type)
    check_celf_ratio(measure_name, celf_ratio)  # checked here, before any device work; it is run_greedy's keyword, not init's
    plan = _Plan(args, assignments, subset_size, subset_ratio)
    if verbose:
        print("extracting {} samples from {} total datapoints".format(plan.subset, plan.rows))
    options = dict(ncentroids=plan.ncentroids, batch_size=plan.batch, selection_size=plan.select,
                   device=args.computation.device, keep_unselected=args.batch.keep_unselected)
    if generator is not None:
        options['generator'] = generator
    if sampler != 'permutation':
        options['sampler'] = sampler
    measure = get_measure(measure_name)(assignments, **options)
    order = plan.candidate_order(shuffle_candidates)
    head, rest = order[:1], order[1:]  # a singleton start: it seeds the tables, it is never selected (batch.py:205-206)
    measure.init(get_cluster_pairing(clustering_types, cluster_pairing, weight_type), rest)
    return measure, head, plan.subset


def _run_greedy(args, assignments, clustering_types, subset_size, subset_ratio, measure_name='mi',
                cluster_pairing='combination', shuffle_candidates=True, verbose=False, weight_type=None, celf_ratio=0):
    ratio = check_celf_ratio(measure_name, celf_ratio)
    measure, head, subset = _prepare(args, assignments, clustering_types, subset_size, subset_ratio, measure_name,
                                     cluster_pairing, shuffle_candidates, verbose, weight_type=weight_type, celf_ratio=ratio)
    lazy = dict(celf_ratio=ratio) if ratio else {}  # only the exact measures take the keyword
    picked, gains, seconds, _lookups = measure.run_greedy(subset, head, None, verbose=verbose,
                                                         log_every=args.log_every, log_times=args.log_times,
                                                         node_rank=args.node_rank, pid=args.parent_pid, **lazy)
    return picked, gains, seconds


def run_greedy(args, assignments, shard_names, filenames, clustering_types, subset_size, subset_ratio,
               measure_name='mi', cluster_pairing='combination', shuffle_candidates=True, verbose=False, weight_type=None,
               celf_ratio=0):
    """-> rows {'filename', 'shard_name'} of the selected clips, ordered by clip index (run_greedy.py:72)"""
    picked, _, _ = _run_greedy(args, assignments, clustering_types, subset_size, subset_ratio, measure_name,
                               cluster_pairing, shuffle_candidates, verbose, weight_type=weight_type, celf_ratio=celf_ratio)
    return [dict(filename=filenames[i], shard_name=shard_names[i]) for i in sorted(picked)]
