"""`cli.py evaluate`: how good is a trained clustering?

The clustering stage writes assignment shards and nothing that says whether they are any good: the one figure the
reference computes -- the mean min-distance KMeans.add returns -- is thrown away by its train loop
(clustering/code/run_clustering.py:171-175).  This module reports, per view and cached epoch, what a second sweep over
the rows finds (KMeans.quality, acav_kmeans_quality: float64 distances on the GPU, there is no CPU path):

  for a row x_i with label l_i (calc_best's, under-used-centre discount included):
    a2_i = ||x_i - c_{l_i}||^2, b2_i = min_{k != l_i} ||x_i - c_k||^2 (+inf when K = 1),
    displaced_i = (b2_i < a2_i): the discount put the row somewhere other than its nearest centre,
    s_i = (sqrt b2_i - sqrt a2_i) / max(sqrt a2_i, sqrt b2_i): the centroid ("simplified") silhouette, 0 when both are 0 or K = 1
  per cluster: count, sum a2, sum sqrt a2, sum s, displaced rows, sum min(a2, b2)
  from those (compose): sizes and empty clusters, inertia = sum a2 / n, nearest_inertia = sum min(a2, b2) / n, the
  displaced share, the mean silhouette, Davies-Bouldin with the trained centres (S_k = sum sqrt a2 / count,
  M_kl = ||c_k - c_l||, DB = mean_k max_{l != k} (S_k + S_l) / M_kl over the non-empty clusters, coincident pairs skipped),
  and the clusters the discount is active for in that state (fp32 counts < fp32((count / K) ** p)).

    python -m acav100m_amd.clustering.cli evaluate --feature_path=<brace glob .pkl> --meta_path=<dir> \\
        --out_path=<dir of a cluster run> --clustering.cached_epoch=<e | [e0,e1,...]> \\
        [--evaluate.out_path=quality.json] [--evaluate.rows_path=<dir>] [--evaluate.silhouette_sample=M [--evaluate.silhouette_seed=S]]

Reads cache_epoch_{e}_{name} like a resumed `cluster` run (cache.py: locate, read, find), reads the rows once per row group
(row_groups.py, data.resident_bytes) and evaluates every listed epoch on them while they are on the device.  Writes no assignment
shard and no log file.
A cache that holds `whiten_std` (a `cluster --clustering.whiten=True` run) has its rows divided by it on their way to the
device, like the run itself (frontend.py: FrontEnd): the report and the rows_path values are then in whitened space, and the view's report carries
"whitened": true and "zero_variance_columns" (divisors that are exactly 1).  Epochs that disagree on it are refused.
A cache that holds `pca_components` (a `cluster --clustering.pca_dim=P` run) has its rows projected through the same helper,
after the division: the view is judged in projected space and its report carries "pca_dim" and
"pca_explained_variance_ratio" (the kept share of the total variance).  Epochs that disagree on a view's projection are refused.
A cache that holds `normalize` (a `cluster --clustering.normalize=True` or `--clustering.spherical=True` run) has its rows divided
by their L2 norms last, through the same helper: the view's report carries "normalized": true, and `silhouette_sampled` is then a
silhouette of chord distances (||x - y||^2 = 2 - 2 cos for unit rows).  A spherical state (unit centres too) also gets
"mean_cosine" = 1 - inertia / 2, the mean cosine between a row and its centre, exact for unit rows and unit centres.
evaluate.rows_path: one <shard>.quality.npz per shard with `filename`, `epochs` and, per view, "<model_key>/<layer>" ->
float64 [epochs, rows, 2] = (a2, b2) -- an outlier or low-margin filter downstream.  One process, one GPU.
evaluate.silhouette_sample=M (default: off) adds the exact silhouette on a seeded sample (silhouette.py, acav_rows_silhouette):
the rows sample_indices(total rows, M, evaluate.silhouette_seed) -- sklearn's silhouette_score(sample_size=M, random_state=seed)
draw, in the global row order the row groups deliver, one set for all views and epochs -- are gathered after the front-end while
the one pass goes by; afterwards every (epoch, view) labels them with calc_best (a row's label is a pure function of the row and
the state: these are the labels the pass gave them) and the report gains silhouette_sampled, silhouette_sample,
silhouette_negative_share and silhouette_by_cluster (silhouette_undefined with the reason, and nan, when the sample has fewer
than two non-empty clusters).  Neither a centre nor a scale enters: it is the figure to compare runs that differ in whiten,
pca_dim, algorithm, init or K.  Without the key the report is what it was.
"""
import json
from collections import OrderedDict
from pathlib import Path

import numpy as np

from . import cache
from .frontend import FrontEnd
from .sgd_clustering import QUALITY_COLS

COUNT, SUM_A2, SUM_SQRT_A2, SUM_S, DISPLACED, SUM_MIN = range(QUALITY_COLS)  # ACAV_QUALITY_* (include/acav_hip.h)


def compose(cluster_stats, centers, counts, count, reinit=(.7, 5.0)):
    """[K, QUALITY_COLS] per-cluster sums + the state they were taken in -> the report dict (pure numpy, float64)"""
    cs = np.asarray(cluster_stats, np.float64)
    centers = np.asarray(centers, np.float32)
    K = cs.shape[0]
    if cs.shape != (K, QUALITY_COLS) or centers.shape[0] != K:
        raise ValueError("cluster_stats {} / centers {} do not belong together".format(cs.shape, centers.shape))
    sizes = np.rint(cs[:, COUNT]).astype(np.int64)
    n = int(sizes.sum())
    nan = float('nan')
    per_row = lambda col: float(cs[:, col].sum() / n) if n else nan  # noqa: E731
    # Davies-Bouldin over the non-empty clusters; centre distances in the difference form (coincident centres give exactly 0)
    ne = np.flatnonzero(sizes > 0)
    db = nan
    if len(ne) >= 2:
        S = cs[ne, SUM_SQRT_A2] / cs[ne, COUNT]
        C = centers[ne].astype(np.float64)
        worst = []
        for i in range(len(ne)):
            M = np.sqrt(((C - C[i]) ** 2).sum(-1))
            ok = M > 0
            ok[i] = False
            if ok.any():
                worst.append(((S[i] + S[ok]) / M[ok]).max())
        db = float(np.mean(worst)) if worst else nan
    p = float(reinit[0])
    thr = np.float32((float(count) / K) ** p)
    under = np.flatnonzero(np.asarray(counts, np.float32) < thr)
    displaced = int(np.rint(cs[:, DISPLACED].sum()))
    return {
        'n': n, 'K': int(K),
        'empty': int((sizes == 0).sum()), 'empty_clusters': [int(k) for k in np.flatnonzero(sizes == 0)],
        'sizes': [int(v) for v in sizes], 'size_min': int(sizes.min()), 'size_median': float(np.median(sizes)), 'size_max': int(sizes.max()),
        'inertia': per_row(SUM_A2), 'nearest_inertia': per_row(SUM_MIN),
        'displaced': displaced, 'displaced_share': (displaced / n) if n else nan,
        'silhouette': per_row(SUM_S), 'davies_bouldin': db,
        'underused': int(len(under)), 'underused_clusters': [int(k) for k in under],
    }


def format_report(report):
    head = "{:<32}{:>6}{:>10}{:>6}{:>7}{:>11}{:>14}{:>14}{:>11}{:>10}{:>10}".format(
        'view', 'epoch', 'n', 'K', 'empty', 'underused', 'inertia', 'nearest', 'displaced', 'silh', 'DB')
    sampled = any('silhouette_sampled' in rep for per_epoch in report['views'].values() for rep in per_epoch.values())
    lines = [head + ("{:>13}".format('silh_sampled') if sampled else '')]  # one more column with evaluate.silhouette_sample
    for name, per_epoch in report['views'].items():
        for epoch, rep in per_epoch.items():
            lines.append("{:<32}{:>6}{:>10}{:>6}{:>7}{:>11}{:>14.6g}{:>14.6g}{:>10.2f}%{:>10.4f}{:>10.4f}".format(
                name, epoch, rep['n'], rep['K'], rep['empty'], rep['underused'], rep['inertia'], rep['nearest_inertia'],
                100.0 * rep['displaced_share'], rep['silhouette'], rep['davies_bouldin'])
                + ("{:>13.4f}".format(rep['silhouette_sampled']) if sampled else ''))
    return '\n'.join(lines)


def _epochs(value):
    if value is None:
        raise ValueError("evaluate needs --clustering.cached_epoch=<e | [e0,e1,...]>: the epoch(s) of the cluster run to judge")
    epochs = [value] if isinstance(value, int) else list(value)
    if not epochs or not all(isinstance(e, int) and not isinstance(e, bool) for e in epochs):
        raise ValueError("clustering.cached_epoch must be an epoch or a list of epochs, not {!r}".format(value))
    return epochs


def load_states(args, epochs):
    """{epoch: {(kind, model_key, layer): attrs}} of the listed epochs, refusing -- before any shard is read -- a cache that
    is missing, unreadable, without a clustering of one of args.models, or still in its warm-up"""
    states = OrderedDict()
    for e in epochs:
        path = cache.locate(args, e)
        if not path.is_file():
            raise FileNotFoundError("no clustering cache of epoch {}: {} does not exist".format(e, path))
        saved = cache.read(path)
        if not saved:
            raise ValueError("clustering cache {} holds no clustering".format(path))
        for mk in (args.models or []):
            if not any(key[1] == mk for key in saved):
                raise ValueError("clustering cache {} lacks a view of model {!r} (it has {})".format(
                    path, mk, sorted({key[1] for key in saved})))
        for key, dt in saved.items():
            K, rounds, count = dt['centers'].shape[0], int(dt.get('initial_rounds', 10)), int(dt.get('count', 0))
            if count < rounds * K:
                raise ValueError("clustering cache {}: view {} is still in its warm-up, count = {} < {}*K = {}: its labels are "
                                 "random draws, train it further first".format(path, '/'.join(key[1:]), count, rounds, rounds * K))
        states[e] = saved
    # one set of rows serves every listed epoch: they have to agree on the space the rows are judged in
    first = next(iter(states.values()), {})
    for e, saved in states.items():
        for key in set(first) | set(saved):
            what = FrontEnd.from_attrs(cache.find(first, key)).differs(FrontEnd.from_attrs(cache.find(saved, key)))
            if what is not None:
                raise ValueError("the clustering caches of epochs {} and {} disagree on {} of view {}: evaluate them in "
                                 "separate runs".format(epochs[0], e, what, '/'.join(key[1:])))
    return states


def evaluate(args):
    """the `evaluate` verb: prints one line per view and epoch, writes the report as json when evaluate.out_path is given,
    returns it"""
    from .. import shards as io
    from .row_groups import current_device, open_row_groups, probe_shards
    from .sgd_clustering import KMeans
    from . import silhouette
    opts = args.get('evaluate') or {}
    sil_m, sil_seed = silhouette.check_options(opts)  # refused before any cache or shard is read
    epochs = _epochs(args.clustering.cached_epoch)
    states = load_states(args, epochs)
    out_path, rows_path = opts.get('out_path'), opts.get('rows_path')

    paths = [Path(p) for p in sorted(io.brace_expand(args.data.path))]
    sizes = io.shard_sizes_from_meta(paths, args.data.meta.path, use_cache=True)
    paths = [p for p in paths if p.stem in sizes]
    _probe, view_dims = probe_shards(args, paths)
    if view_dims is None:
        raise ValueError("none of the {} shards of {} could be read".format(len(paths), args.data.path))
    dev = current_device(args)
    # a whitened run's centres live in x / whiten_std space, a projected run's in the space of its components (after the
    # division, if there is one): the rows go through the same front-end on their way to the device as the run's own
    fronts = OrderedDict((v, FrontEnd.from_attrs(cache.find(states[epochs[0]], v))) for v in view_dims)
    for v, f in fronts.items():
        f.check_width(v, view_dims[v])
    cl = OrderedDict()
    for e, saved in states.items():
        for v, d in view_dims.items():
            dt = cache.find(saved, v)
            d = fronts[v].width_out(d)
            if dt is None or dt['centers'].shape[1] != d:
                raise ValueError("the clustering cache of epoch {} lacks view {} (width {})".format(e, '/'.join(v[1:]), d))
            km = KMeans.load(dt)
            km.args = None  # one process, one GPU, whatever run wrote the cache
            cl[e, v] = km.to(dev)
    groups = open_row_groups(args, paths, sizes, view_dims)
    groups.add_front_ends(fronts)
    acc = OrderedDict((key, np.zeros((km.centers.shape[0], QUALITY_COLS), np.float64)) for key, km in cl.items())
    if rows_path is not None:
        Path(rows_path).mkdir(parents=True, exist_ok=True)
    if sil_m is not None:  # the sample: one set of global row numbers for all views and epochs, gathered while the pass goes by
        import torch
        n_total = sum(int(sizes[p.stem]) for p in paths) if groups.streamed else len(groups.resident_table())
        picks = silhouette.sample_indices(n_total, sil_m, sil_seed)
        if len(picks) < 2:
            raise ValueError("evaluate.silhouette_sample: the shards hold {} rows, a silhouette needs two".format(n_total))
        sample, base = OrderedDict(), 0
    for _gi, table, rows in groups.iterate():
        if sil_m is not None:
            n_g = next(iter(rows.values())).shape[0]
            lo, hi = (int(i) for i in np.searchsorted(picks, (base, base + n_g)))
            for v in view_dims:
                x = rows[v]
                if v not in sample:
                    sample[v] = torch.empty((len(picks), x.shape[1]), dtype=torch.float32, device=x.device)
                if hi > lo:
                    sample[v][lo:hi] = x[torch.from_numpy(picks[lo:hi] - base).to(x.device)]
            base += n_g
        per_row = {}
        for (e, v), km in cl.items():  # every epoch's centres on the rows while they are on the device
            labels, _ = km.calc_best(rows[v], need_mean=False)
            res = km.quality(rows[v], labels, rows=rows_path is not None)
            if rows_path is not None:
                res, per_row[e, v] = res
            acc[e, v] += res  # row groups in group order
        if rows_path is not None:
            for shard, ids in table.shard_rows.items():
                if not ids:
                    continue
                ids = np.asarray(ids, np.int64)
                arrays = {'/'.join(v[1:]): np.stack([per_row[e, v][ids] for e in epochs]) for v in view_dims}
                np.savez(Path(rows_path) / (shard + '.quality.npz'), filename=np.array([table.filename[i] for i in ids]),
                         epochs=np.asarray(epochs, np.int64), **arrays)

    if sil_m is not None and base != n_total:
        raise RuntimeError("the shards delivered {} rows, their metadata states {}: fix the metadata or drop the unreadable shards "
                           "from the list".format(base, n_total))
    report = {'feature_path': str(args.data.path), 'clusters_path': str(args.data.output.path), 'epochs': epochs,
              'views': OrderedDict()}
    for (e, v), km in cl.items():
        centers, counts, count, _fb = km.state_arrays()
        rep = compose(acc[e, v], centers, counts, count, km.reinit)
        std, fit = fronts[v].std, fronts[v].pca
        if std is not None:  # every figure of this view is in whitened space; a zero-variance column's divisor is exactly 1
            rep['whitened'] = True
            rep['zero_variance_columns'] = int((std == np.float32(1.0)).sum())
        if fit is not None:  # every figure of this view is in projected space
            tv = float(fit['total_variance'])
            rep['pca_dim'] = int(fit['components'].shape[0])
            rep['pca_explained_variance_ratio'] = float(fit['explained_variance'].sum() / tv) if tv > 0 else float('nan')
        if fronts[v].normalize:  # every figure of this view is about directions
            rep['normalized'] = True
        if km.spherical:  # unit rows and unit centres: ||x - c||^2 = 2 - 2 cos(x, c)
            rep['mean_cosine'] = 1.0 - rep['inertia'] / 2.0
        if sil_m is not None:  # the sample's labels in this state, then every pairwise distance of it
            K = km.centers.shape[0]
            labels, _ = km.calc_best(sample[v], need_mean=False)
            A, B, s = silhouette.silhouette_samples(sample[v], labels, k=K)
            sil = silhouette.summarise(A, B, s, labels.cpu().numpy(), K)
            if 'silhouette_undefined' not in sil and not np.isfinite(sil['silhouette_sampled']):
                raise ValueError("view {}, epoch {}: the sampled silhouette is {!r}: the rows of the sample are not all "
                                 "finite".format('/'.join(v[1:]), e, sil['silhouette_sampled']))
            rep.update(sil)
        report['views'].setdefault('/'.join(v[1:]), OrderedDict())[str(e)] = rep
    print(format_report(report))
    if out_path is not None:
        out_path = Path(out_path)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        with open(out_path, 'w') as f:
            json.dump(report, f, indent=1)
    return report
