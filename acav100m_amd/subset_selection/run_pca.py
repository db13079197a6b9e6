"""The PCA baseline's drivers: `run_single_pca` / `run_chunks_pca` for the measures pca, pca_ip, pca_cs, pca_l1 and pca_l2
(measures/pca.py).  These measures read FEATURE shards, not assignment shards -- in the reference
(correspondence_retrieval/code/clustering.py:54-78, run_clusterings) the whiten + PCA front-end replaces k-means exactly when
'pca' is in the measure's name, and the projected views go to measures/pca.py: PCAOptim.

Plan of a run: load the feature shards; every view in key order ((model_key, layer) sorted, the order of the assignment
columns); optionally whiten (pca.whiten: x / std(x, axis=0)); pca_features(views, pca.dim) -- dim None: the smallest view
width; a view narrower than dim, or V <= dim, raises ValueError before any kernel runs; the clustering pairs of
clustering.pairing over the keys; PCAOptim; k = subset.size or round(subset.ratio * V); the rows {'filename', 'shard_name'} of
sorted(S) appended to output.csv.  Chunked: every chunk fits its own PCA and selects from its own clips, one process per GPU,
into the cache files `reduce_csvs` / `reduce_pkls` merge (run.run_chunks)."""
from pathlib import Path

from .. import shards as io
from .chunks import plan_chunks, save_chunk, shard_paths
from .measures import PCA_MEASURES, get_measure
from .pairing import get_cluster_pairing


def projected_views(args, table):
    """-> (keys [(model_key, layer)] sorted, {key: device tensor [V, dim]}): the whiten + PCA front-end on every view"""
    from ..clustering.pca import pca_features
    from ..clustering.whiten import whiten
    by_key = {}
    for (kind, model_key, layer), mat in table.views.items():
        by_key[(model_key, layer)] = mat
    keys = sorted(by_key)
    if not keys:
        raise ValueError("no feature views in the shards")
    cfg = args.pca or {}
    dim = cfg.get('dim')
    V = len(table)
    want = min(int(by_key[k].shape[1]) for k in keys) if dim is None else int(dim)
    for k in keys:  # before any kernel runs
        if int(by_key[k].shape[1]) < want:
            raise ValueError("view {}/{} has {} columns: narrower than pca.dim={}".format(k[0], k[1], by_key[k].shape[1], want))
    if V <= want:
        raise ValueError("{} clips cannot carry {} principal components (N <= p)".format(V, want))
    device = args.computation.device
    views = {k: by_key[k] for k in keys}
    if cfg.get('whiten', True):
        views = {k: whiten(v, device=device)[0] for k, v in views.items()}
    return keys, pca_features(views, want, device)


def select(args, table):
    """-> (S, rows of sorted(S)) for the clips of `table`"""
    keys, views = projected_views(args, table)
    pairs = get_cluster_pairing(keys, args.clustering.pairing, None)
    measure = get_measure(args.measure_name)([views[k] for k in keys], device=args.computation.device)
    measure.init(pairs, list(range(len(table))))
    V = len(table)
    k = round(args.subset.ratio * V) if args.subset.size is None else min(int(args.subset.size), V)
    if args.verbose:
        print("extracting {} samples from {} total datapoints".format(k, V))
    S, _, _, _ = measure.run(k, None)
    return S, [dict(filename=table.filename[i], shard_name=table.shard_name[i]) for i in sorted(S)]


def _run(args, paths):
    paths = [Path(p) for p in paths]
    table = io.load_feature_shards(paths)
    metas = io.load_metas(paths, args.data.meta.path)
    if len(table) == 0:
        return [], metas
    return select(args, table)[1], metas


def run_single_pca(args):
    rows, metas = _run(args, shard_paths(args))
    out_path, count = io.append_output_csv(rows, metas, args.data.output.path)
    if args.verbose:
        print("Saved Results: added {} lines to {}".format(count, out_path))
    return out_path, count


def run_chunks_pca(args):
    """run.run_chunks for THIS process's rank (one process per GPU): chunk after chunk, the same cache file names"""
    plan, chunk_args = plan_chunks(args)
    written = []
    for i, (num, chunk) in enumerate(plan.mine):
        print("running chunk {}".format(num))
        rows, metas = _run(chunk_args, chunk)
        written.append(save_chunk(args, plan, i, rows, metas))
    return written


def is_pca_measure(name):
    return str(name).lower() in PCA_MEASURES
