"""`cli.py evaluate`: how good is a finished selection?

The selection stage builds subsets; this module scores one: for every clustering partition, the agreement of the
clusterings on the selected clips -- sklearn's mutual_info / normalized_mutual_info / adjusted_mutual_info / adjusted_rand /
fowlkes_mallows / rand scores of every clustering pair's two label columns restricted to the selection, averaged over the
pairs (MutualInformation.get_measure, correspondence_retrieval/code/measures/mutual_information.py:11-17,74-85; the
quantities the reference's README states its results in).  Beside it: the same scores of the whole partition and of R
uniformly drawn subsets of the same size.  The tables, the per-pair sums and the exact expected mutual information are
computed on the GPU (EfficientBatchMI.score_subset, acav_mi_score_subset); there is no CPU path.

Scores are per partition: labels of different clustering runs are not comparable.

    python -m acav100m_amd.subset_selection.cli evaluate --shards_path=<brace glob .pkl> --meta_path=<dir> \\
        --selection_path=<output.csv> [--evaluate.measures=a,b] [--evaluate.random_baselines=R] \\
        [--evaluate.out_path=scores.json]

Defaults: all six scores, R = 0, no file.  Draw r of the baseline is random.Random(computation.random_seed + r).sample.
"""
import csv
import json
import random
from pathlib import Path

import numpy as np

from .. import shards as io
from .measures.batch import SCORE_NAMES, EfficientBatchMI, score_mask
from .pairing import get_cluster_pairing


def read_selection(csv_path):
    """rows of an output.csv -> [(shard_name, filename)] in file order (repeats kept: `run` appends)"""
    rows = []
    with open(csv_path, newline='') as f:
        for rec in csv.reader(f):
            if not rec:
                continue
            if len(rec) < 2:
                raise ValueError("{}: row {!r} has no (shard_name, filename)".format(csv_path, rec))
            rows.append((rec[0], rec[1]))
    return rows


def map_selection(rows, shard_names, filenames):
    """[(shard_name, filename)] of a selection -> (distinct clip rows in order of first appearance, number of repeated rows,
    rows that match no clip of this partition).  A clip is identified by (shard_name, filename)."""
    index = {}
    for i, key in enumerate(zip(shard_names, filenames)):
        index.setdefault((str(key[0]), str(key[1])), i)
    ids, seen, repeats, unknown = [], set(), 0, []
    for key in rows:
        i = index.get((str(key[0]), str(key[1])))
        if i is None:
            unknown.append(key)
        elif i in seen:
            repeats += 1
        else:
            seen.add(i)
            ids.append(i)
    return ids, repeats, unknown


def _measure(assignments, clustering_types, pairing, device):
    assignments = np.ascontiguousarray(assignments, dtype=np.int64)
    m = EfficientBatchMI(assignments, ncentroids=int(assignments.max()) + 1, device=device)
    m.init(get_cluster_pairing(clustering_types, pairing), [])
    return m


def score_selection(assignments, clustering_types, ids, pairing='combination', measures=None, prefixes=None, device='cuda:0'):
    """scores of the clips `ids` of one partition's assignment matrix [V, D] -> {name: float | array over prefixes}"""
    score_mask(measures)  # an unknown name raises before the device is touched
    return _measure(assignments, clustering_types, pairing, device).score_subset(ids, measures=measures, prefixes=prefixes)


def evaluate_partition(assignments, clustering_types, ids, pairing='combination', measures=None, baselines=0, seed=0,
                       device='cuda:0'):
    """-> {'n', 'total', 'selection', 'whole', 'random': [...], 'random_mean'} for one partition"""
    names, _ = score_mask(measures)
    m = _measure(assignments, clustering_types, pairing, device)
    total = int(np.shape(assignments)[0])
    report = {'n': len(ids), 'total': total,
              'selection': m.score_subset(ids, measures=names),
              'whole': m.score_subset(np.arange(total, dtype=np.int64), measures=names),
              'random': [], 'random_mean': None}
    for r in range(int(baselines)):
        draw = random.Random(int(seed) + r).sample(range(total), len(ids))
        report['random'].append(m.score_subset(draw, measures=names))
    if report['random']:
        report['random_mean'] = {k: float(np.mean([d[k] for d in report['random']])) for k in names}
    return report


def format_report(report):
    lines = []
    for part, rep in report['partitions'].items():
        lines.append("partition {}: {} of {} clips selected ({} repeated csv rows scored once)".format(
            part, rep['n'], rep['total'], rep['repeated_rows']))
        cols = ['selection', 'whole'] + (['random_mean'] if rep['random_mean'] else [])
        lines.append("  {:<24}".format('score') + ''.join("{:>14}".format(c) for c in cols))
        for name in report['measures']:
            lines.append("  {:<24}".format(name) + ''.join("{:>14.6f}".format(rep[c][name]) for c in cols))
    return '\n'.join(lines)


def evaluate(args):
    """the `evaluate` verb: load the partitions as `run` does, map the csv rows to clips, score; prints a table, writes the
    report as json when evaluate.out_path is given, returns it"""
    from .run import load_data
    opts = args.get('evaluate') or {}
    names, _ = score_mask(opts.get('measures'))  # before any shard is read
    baselines = int(opts.get('random_baselines') or 0)
    out_path = opts.get('out_path')
    if args.get('selection_path') is None:
        raise ValueError("evaluate needs --selection_path=<output.csv of a run>")
    rows = read_selection(args.selection_path)
    partitions, _ = load_data(args.data.path, args.data.meta.path, args.verbose)
    if not partitions:
        raise ValueError("no assignment shards under {}".format(args.data.path))
    seed = int(args.computation.random_seed or 0)
    device = 'cuda:0' if str(args.computation.device) == 'cuda' else str(args.computation.device)
    loaded, matched = {}, set()
    for k in sorted(partitions):
        assignments, clustering_types, shard_names, filenames = io.load_assignment_shards(partitions[k])
        ids, repeats, unknown = map_selection(rows, shard_names, filenames)
        matched.update(set(rows) - set(unknown))
        loaded[k] = (assignments, clustering_types, ids, repeats)
    missing = [r for r in rows if r not in matched]
    if missing:
        raise ValueError("{}: {} row(s) match no clip of the shards, the first is shard_name={!r} filename={!r}".format(
            args.selection_path, len(missing), missing[0][0], missing[0][1]))
    report = {'selection_path': str(args.selection_path), 'measures': list(names), 'pairing': args.clustering.pairing,
              'random_baselines': baselines, 'random_seed': seed, 'partitions': {}}
    for k, (assignments, clustering_types, ids, repeats) in loaded.items():
        if not ids:
            continue  # the selection holds no clip of this partition
        rep = evaluate_partition(assignments, clustering_types, ids, args.clustering.pairing, names, baselines, seed, device)
        rep['repeated_rows'] = repeats
        report['partitions'][str(k)] = rep
    print(format_report(report))
    if out_path is not None:
        out_path = Path(out_path)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        with open(out_path, 'w') as f:
            json.dump(report, f, indent=1)
    return report
