"""Clustering stage: train_clusters + assign_clusters (clustering/code/run_clustering.py:25-272),
restructured for a 288 GB-HBM GPU: the feature shards are read once into resident [N,d] matrices
(one per (model, layer) view), every KMeans trains on its matrix with the bulk C-ABI call (no host
synchronisation per step), then one assign sweep per view labels all rows; the reference's per-row
dict / pkl schema only exists at the file boundary (acav100m_amd/shards.py).

Same observable behaviour as the reference:
  * KMeans objects are created in args.models order, layer by layer (RNG order of run_clustering.py:32-44)
  * the training batches are the ones the reference's DataLoader delivers for the configured computation.num_workers
    (default 40: whole batches round-robin over worker shard subsets, data/clustering.py:17-66,212-228; 0: one stream),
    every stream cut / cycled to get_length() samples (parallel/row_plan.py: loader_stream; data.loader_order / loader_tail)
  * per batch, every clustering takes one add() -- the warm-up draws are
    interleaved across clusterings exactly like the reference's per-batch loop (:229-241)
  * lr = 0.1 ** (2 + epoch // 5), drop_last batches; several GPUs: clustering.multi_gpu (config.py) -- `views` keeps the
    one-GPU batch stream and epoch count, `reference` is the reference's own N-GPU stream with ceil(epochs / num_gpus) epochs
  * cache_epoch_{e}_{name} checkpoints, skip of already written shards, log_*.json manifest
clustering.algorithm=lloyd (ours; clustering/lloyd.py) trains with batch k-means instead: train_clusters branches once, to
_train_clusters_lloyd; the caches, cached_epoch, the assign sweep and `evaluate` are the ones above.
This module is the stage and its three training loops.  Beside it: cache.py (the cache_epoch files: locate, read, save, find),
frontend.py (FrontEnd: a view's whiten / PCA / row-normalisation stages, their cache keys, checks and application), row_groups.py (_RowGroups, the
device budget, the loader settings, the shard probe) and options.py (multi_gpu_mode and the refusals of check_options).
"""
from collections import OrderedDict
from pathlib import Path

import numpy as np

from .. import shards as io
from ..parallel import world
from . import cache
from .cache import path as _cache_path, read as _read_cache  # noqa: F401  (the names of before the cache module)
from .frontend import PCA_KEYS, FrontEnd, pca_of as _pca_of  # noqa: F401
from .kmeanspp import check_init
from .lloyd import check_algorithm
from .options import check_normalize, check_pca, check_whiten, multi_gpu_mode
from . import row_groups
from .row_groups import current_device as _device, loader_settings, open_row_groups, probe_shards  # noqa: F401
from .sgd_clustering import KMeans


def _RowGroups(*a, **kw):
    """row_groups._RowGroups with the rows going where this module's _device says (the name and the hook of before the move)"""
    return row_groups._RowGroups(*a, device=lambda args: _device(args), **kw)


def check_options(args, world_size):
    """the refusals that need no device and no file, before anything is created or read"""
    check_whiten(args, world_size)
    check_pca(args, world_size)
    check_normalize(args, world_size)
    check_algorithm(args, world_size, merges=('rows',))  # (_train_clusters_lloyd all-reduces the tables in that mode)
    check_init(args)


def init_clusterings(args, table, widths=None):
    """run_clustering.py:32-52 -- one KMeans per view, created in view order (RNG order).  widths: {view: columns} of the views
    that are not trained at the width of their stored rows (clustering.pca_dim: a projected view has d = p)."""
    cl = OrderedDict()
    for view, mat in table.views.items():
        cl[view] = KMeans(args, (widths or {}).get(view, mat.shape[1]), args.clustering.ncentroids)
    return _to_device(args, cl)


def _to_device(args, cl):
    dev = _device(args)
    for km in cl.values():
        km.to(dev)
        km.initialize()
    return cl


def load_clusterings(args, table, widths=None, cached=None):
    """run_clustering.py:55-107: resume from cache_epoch_{e}_{name} (or a cache trained on a subset of
    these shards) when --clustering.cached_epoch is set.  cached: _cached_attrs' (the file is read once per run)."""
    if isinstance(args.clustering.cached_epoch, int):
        path, saved = cached if cached is not None else _cached_attrs(args)
        if saved is not None:
            saved = {v: cache.find(saved, v) for v in table.views}
            if all(x is not None for x in saved.values()):
                print("loading from clustering cache: {}".format(path))
                cl = OrderedDict((v, KMeans.load(saved[v])) for v in table.views)
                for km in cl.values():
                    km.args = args
                return _to_device(args, cl), True
            print("clustering cache features does not match with the given models")
        print("no clustering cache found.")
    return init_clusterings(args, table, widths), False


def save_clusterings(args, epoch, cl, whiten_std=None, pca=None):
    """cache.save with the front-ends stated as {view: std} and {view: projection | None}"""
    views = set(whiten_std or ()) | set(pca or ())
    cache.save(args, epoch, cl, {v: FrontEnd((whiten_std or {}).get(v), (pca or {}).get(v)) for v in views})


def _cached_attrs(args):
    """(cache file, {(kind, model_key, layer): attrs} | None when it is unreadable) of the cache that clustering.cached_epoch
    names (cache.locate), read once -- or (None, None) when there is no file"""
    epoch = args.clustering.cached_epoch
    path = cache.locate(args, epoch) if isinstance(epoch, int) else None
    if path is None or not path.is_file():
        return None, None
    return path, cache.read(path)


def _usable(args, cached):
    """(cache file, attrs) of a cache that holds clusterings, else (None, {})"""
    path, saved = cached if cached is not None else _cached_attrs(args)
    return (path, saved) if saved else (None, {})


def check_cached_algorithm(args, cached=None):
    """clustering.resume_training continues a cache with the algorithm that trained it: refused (ValueError) when the cache
    clustering.cached_epoch names was trained by the other one ('algorithm' in its states; none: sgd).  No device."""
    path, saved = _usable(args, cached)
    if path is None or not args.clustering.resume_training:
        return
    want = args.clustering.algorithm or 'sgd'
    for key, dt in saved.items():
        have = dt.get('algorithm') or 'sgd'
        if have != want:
            raise ValueError("clustering.resume_training with clustering.algorithm={}, but view {} of the clustering cache {} was "
                             "trained by {}: a run continues with the algorithm it started with".format(want, '/'.join(key[1:]), path, have))
        if args.clustering.spherical and not dt.get('spherical'):
            raise ValueError("clustering.resume_training with clustering.spherical=True, but view {} of the clustering cache {} is "
                             "not a spherical state: its centres are plain cluster means, and a run continues what it started "
                             "as".format('/'.join(key[1:]), path))


def cached_normalization(args, cached=None, normalize=False):
    """(cache file, {(model_key, layer)} of the views whose rows the cache says are L2-normalised), like cached_whitening: the
    cache is authoritative.  normalize (the run's switch, clustering.spherical included) against a cache without the key is the
    ValueError of a cached run that names the file."""
    path, saved = _usable(args, cached)
    found = {key[1:] for key, dt in saved.items() if dt.get('normalize')}
    if normalize and path is not None and not found:
        raise ValueError("clustering.normalize=True (or clustering.spherical=True), but the clustering cache {} holds no 'normalize' "
                         "key: its centres were trained on rows that were not normalised".format(path))
    return path, found


def cached_whitening(args, cached=None):
    """(cache file, {(model_key, layer): whiten_std}) of the cache that clustering.cached_epoch names -- the file
    load_clusterings will load -- or (None, {}) when there is none.  The cache is authoritative: its std is used as it is, so
    new shards are assigned in the space the centres were trained in."""
    path, saved = _usable(args, cached)
    return path, {key[1:]: dt['whiten_std'] for key, dt in saved.items() if dt.get('whiten_std') is not None}


def cached_projection(args, cached=None):
    """(cache file, {(model_key, layer): projection}) of that cache, like cached_whitening: nothing is recomputed.  Raises the two
    ValueErrors of a cached run that names the file: clustering.pca_dim set against a cache without the keys, and a pca_dim
    that disagrees with the cached p."""
    path, saved = _usable(args, cached)
    found = {key[1:]: _pca_of(dt) for key, dt in saved.items() if _pca_of(dt) is not None}
    dim = args.clustering.pca_dim
    if dim is not None and path is not None:
        if not found:
            raise ValueError("clustering.pca_dim={}, but the clustering cache {} holds no pca_components: its centres were trained "
                             "on unprojected rows".format(dim, path))
        for key, f in found.items():
            if f['components'].shape[0] != dim:
                raise ValueError("clustering.pca_dim={}, but view {} of the clustering cache {} was projected to {} columns".format(
                    dim, '/'.join(key), path, f['components'].shape[0]))
    return path, found


def _shard_prefix(table):
    """the row offsets of a group's non-empty shards in shard order, each a run of consecutive table rows"""
    prefix = [0]
    for stem, ids in table.shard_rows.items():
        if not ids:
            continue
        if ids[0] != prefix[-1] or ids[-1] - ids[0] != len(ids) - 1:
            raise RuntimeError("shard {} is not a run of consecutive table rows".format(stem))
        prefix.append(ids[-1] + 1)
    return prefix


def compute_pca(groups, dim):
    """The pre-pass of clustering.pca_dim, after the whitening is set: one pass over the row groups, per view one
    acav_rows_scatter call per group with the group's shards as segments, into float64 accumulators on the device
    (pca.ScatterMoments) -> {view: dict(mean, components, explained_variance, total_variance) | None}.  The shift is the
    fp32-rounded column mean of the view's first non-empty shard (one ColumnMoments.update on it).  A view with d <= dim is left
    alone (None).  Resident data: the pass uploads the rows training keeps using.  Streamed data: one extra read of every shard."""
    from .pca import ScatterMoments, components_from_scatter
    from .whiten import ColumnMoments
    if groups.streamed:
        print("pca: the scatter matrices take one extra read of every shard ({} groups stream)".format(len(groups.groups)))
    moments, widths = OrderedDict(), OrderedDict()
    for _gi, table, rows in groups.iterate():
        prefix = _shard_prefix(table)
        for v, x in rows.items():
            widths[v] = x.shape[1]
            if x.shape[1] <= dim or len(prefix) < 2:
                continue
            if v not in moments:
                cm = ColumnMoments(x.shape[1], x.device)
                cm.update(x[prefix[0]:prefix[1]])
                moments[v] = ScatterMoments(x.shape[1], cm.mean.astype(np.float32), x.device)
            moments[v].update(x[:prefix[-1]], prefix)
        del rows
    fits = OrderedDict()
    for v, d in widths.items():
        name = '/'.join(v[1:])
        sm = moments.pop(v, None)
        if sm is None:
            fits[v] = None
            print("pca {}: {} columns <= pca_dim {}: left alone".format(name, d, dim))
            continue
        n, mean, S = sm.finish()
        del sm
        f = fits[v] = components_from_scatter(n, mean, S, dim, what="view {}".format(name))
        w = f['explained_variance']
        gap = float(((w[:-1] - w[1:]) / w[:-1]).min()) if len(w) > 1 and w[-2] > 0 else float('nan')
        ratio = float(w.sum() / f['total_variance']) if f['total_variance'] > 0 else float('nan')
        print("pca {}: {} rows, {} of {} columns, explained variance ratio {:.6g}, smallest relative gap between kept "
              "eigenvalues {:.3g}".format(name, n, dim, d, ratio, gap))
    return fits


def compute_whitening(groups, shard_stems=None, view_dims=None):
    """The stats pre-pass of clustering.whiten: one pass over the row groups, per view one acav_colstats call per group with
    the group's shards as segments, merged in shard order (whiten.ColumnMoments) -> {view: std fp32 [d]}.  Resident data: the
    pass uploads the rows training keeps using.  Streamed data: one extra read of every shard.
    shard_stems (lloyd + clustering.multi_gpu=rows): the stems of ALL shards in list order, `groups` holding this rank's.  Every
    rank keeps the (n, mean, M2) of its shards per shard; the ranks exchange them bit for bit (parallel/lloyd_rows.py: one
    collective for the counts, one per view of view_dims, whatever a rank's rows look like) and replay add_segment in global
    shard order: the one-GPU run's sequence of Chan merges, hence its std bytes."""
    from .whiten import ColumnMoments
    if groups.streamed:
        print("whitening: the column moments take one extra read of every shard ({} groups stream)".format(len(groups.groups)))
    moments = OrderedDict()
    index = None if shard_stems is None else {stem: i for i, stem in enumerate(shard_stems)}
    per_shard, shard_n = OrderedDict(), {}  # partitioned: {view: float64 [S, 2, d]} and {global shard: rows}, this rank's part
    if index is not None:
        for v, d in view_dims.items():
            per_shard[v] = np.zeros((len(index), 2, d), np.float64)
    for _gi, table, rows in groups.iterate():
        prefix = _shard_prefix(table)
        stems = [stem for stem, ids in table.shard_rows.items() if ids]  # the segments: the non-empty shards, in order
        for v, x in rows.items():
            if v not in moments:
                moments[v] = ColumnMoments(x.shape[1], x.device)
            if len(prefix) > 1 and x.shape[1] > 0:
                seg = moments[v].update(x[:prefix[-1]], prefix)
                if index is not None:
                    per_shard[v][[index[stem] for stem in stems]] = seg
        if index is not None:
            for si, stem in enumerate(stems):
                shard_n[index[stem]] = prefix[si + 1] - prefix[si]
        del rows
    if index is not None:
        from ..parallel import lloyd_rows
        counts = lloyd_rows.exchange_counts(shard_n, len(index))
        for v, d in view_dims.items():
            moments[v] = lloyd_rows.replay_moments(d, counts, lloyd_rows.exchange_bits(per_shard[v]))
    stds = OrderedDict()
    for v, cm in moments.items():
        stds[v] = cm.std()
        print("whitening {}: {} rows, {} zero-variance columns of {} (divided by 1), std min {:.6g} max {:.6g}".format(
            '/'.join(v[1:]), cm.n, cm.zero_columns, cm.d, float(stds[v].min()) if cm.d else 0.0, float(stds[v].max()) if cm.d else 0.0))
    return stds


def _draw_loader_seed(cl):
    """`for batch in dataloader` (run_clustering.py:235) creates a DataLoader iterator, which draws its 64-bit base seed from the
    global CPU generator (torch/utils/data/dataloader.py, _BaseDataLoaderIter.__init__: torch.empty((), dtype=int64).random_())
    = two mt19937 words per epoch, between the centre initialisation and the first warm-up draw.  Consumed here so that a
    seeded run reproduces the reference CLI's files bit for bit (tests/test_gpu_cli.py); every rank creates its own."""
    gen = next(iter(cl.values()))._generator
    gen.u32()
    gen.u32()


def _draw_warmup(cl, batch, steps, width):
    """the warm-up labels of `steps` steps of `batch` rows, `width` of them drawn here, batch by batch across the clusterings
    like the reference loop (run_clustering.py:170-175 steps every clustering per batch) -> {view: int64 [warm-up steps, width]}"""
    need = {v: km.warmup_steps(batch, steps) for v, km in cl.items()}
    warm = {v: np.empty((need[v], width), np.int64) for v in cl}
    for t in range(max(need.values(), default=0)):
        for v, km in cl.items():
            if t < need[v]:
                warm[v][t] = km.draw_warmup(width)
    return warm


def train_clusters(args, probe, groups, shard_stems=(), cached=None):
    # a projected view (clustering.pca_dim) trains at d = p
    widths = {v: f.width_out(probe.views[v].shape[1]) for v, f in groups.fronts.items()}
    cl, loaded = load_clusterings(args, probe, widths, cached)
    if loaded and not args.clustering.resume_training:
        return cl
    pre = args.clustering.cached_epoch if loaded else 0
    rank, w = world()
    # `views` (default): several GPUs split the CLUSTERINGS, every one of which still sees every batch of every epoch with
    # the one-GPU arithmetic -- the N-GPU run produces the files of the one-GPU run.  (The reference divides the epochs by
    # the number of GPUs, run_clustering.py:146, and has every rank stream every shard with a per-rank batch of
    # batch_size / N: that run is `clustering.multi_gpu=reference`, _train_clusters_planned.)
    epochs = int(args.clustering.epochs)
    b = int(args.data.batch_size)
    if args.clustering.algorithm == 'lloyd':
        return _train_clusters_lloyd(args, cl, groups, pre, epochs, loaded, shard_stems)
    print("training sgd kmeans for views: {}".format([v[1:] for v in cl]))
    if w > 1 and multi_gpu_mode(args) != 'views':
        return _train_clusters_planned(args, cl, groups, pre, epochs, b, multi_gpu_mode(args), shard_stems)
    # WHICH rows form the batches: the reference's DataLoader for this computation.num_workers (parallel/row_plan.py), as a
    # stream of (shard, first row, rows) per epoch.  The stream is planned from the shard sizes the metadata states (the
    # reference sizes its loader from the json files too, data/clustering.py:47-52); resident data: from the rows that loaded.
    from ..parallel import make_plan
    paths, sizes, row_bytes, budget = groups.paths, groups.sizes, groups.row_bytes, groups.budget
    meta_rows = [int(sizes[p.stem]) for p in paths]
    shard_rows = meta_rows
    if not groups.streamed:
        table = groups.resident_table()
        shard_rows = [len(table.shard_rows.get(p.stem) or ()) for p in paths]
    nw_order, tail = loader_settings(args)
    plan = make_plan('views', shard_rows, 1, b, epochs, num_workers=nw_order, meta_rows=meta_rows, tail=tail)
    first_row = np.concatenate([[0], np.cumsum(shard_rows)]).astype(np.int64)
    if plan.steps == 0:
        print("no whole batch of {} rows in {} rows: nothing to train on".format(b, sum(shard_rows)))
    print("loader order: {} -> {} steps of {} rows per epoch".format(plan.loader, plan.steps, b))

    def shard_extents(pe):  # the plan's (row range) extents back in (shard, first, rows) form, cut to the epoch
        out, need = [], pe.steps * b
        for _o, f, n in pe.extents[0]:
            n = min(n, need)
            need -= n
            while n > 0:
                si = int(np.searchsorted(first_row, f, side='right')) - 1
                m = min(n, int(first_row[si + 1]) - f)
                out.append((si, f - int(first_row[si]), m))
                f, n = f + m, n - m
            if need <= 0:
                break
        return out

    for epoch in range(pre, pre + epochs):
        lr = 0.1 ** (2 + epoch // 5)
        for km in cl.values():
            km.lr = lr
        _draw_loader_seed(cl)
        # several GPUs: a rank only trains (hence only uploads) its share of the views -- view i -> rank i % world
        own = None if w == 1 else {v for i, v in enumerate(cl) if i % w == rank}
        ext = shard_extents(plan.at_epoch(epoch - pre))
        for table, part in groups.iterate_stream(paths, ext, b, row_bytes, budget, views=own):
            n = next(iter(part.values())).shape[0] if part else 0
            assert n % b == 0
            steps = n // b
            if steps == 0:
                continue
            # (every rank draws all of them from the same stream, so the generators stay in step whoever trains which clustering)
            warm = _draw_warmup(cl, b, steps, b)
            if w > 1:  # the clusterings are dealt out over the GPUs; states are exchanged once per epoch
                from ..parallel import train_epoch_view_parallel
                train_epoch_view_parallel(cl, part, b, lr, warm, broadcast=False)
            else:  # all clusterings of the batch stream side by side on the GPU (independent SGD chains)
                KMeans.train_epoch_multi(list(cl.values()), [part[v] for v in cl], b, lr=lr, warm_bests=[warm[v] for v in cl])
            for km in cl.values():  # the gathered copy of this group is released before the next one is built
                km.synchronize()
            del part
        if w > 1:  # state identical to the one-GPU run on every rank
            from ..parallel import broadcast_states
            broadcast_states(cl)
        if rank == 0:
            cache.save(args, epoch, cl, groups.fronts)
    return cl


def _local_shard_counts(groups):
    """{stem: rows} of the shards `groups` holds, as the run numbers them: the rows that loaded (resident) or that the metadata
    states (streamed)"""
    if groups.streamed:
        return {p.stem: int(groups.sizes[p.stem]) for p in groups.paths}
    table = groups.resident_table()
    return {p.stem: len(table.shard_rows.get(p.stem) or ()) for p in groups.paths}


def _train_clusters_lloyd(args, cl, groups, pre, iters, resumed, shard_stems=(), force_partitioned=False):
    """clustering.algorithm=lloyd: `iters` iterations of batch k-means per view (clustering/lloyd.py), each one pass over the row
    groups with two sweeps per view -- the assign sweep and acav_lloyd_accumulate into int64 tables on the device -- and the centre
    update on the device too (acav_lloyd_centers; on the host in an iteration that has an empty cluster to split; a spherical
    run -- clustering.spherical, or a resumed state that says so -- then renormalises the centre table, lloyd.finish_iteration).  Before the first one, one read-once pass takes every view's largest magnitude (the scale of the fixed
    point) and, for a fresh run, the initial centres: the rows generator.randperm(N)[:K], drawn view by view, read as the
    front-ends deliver them -- or, with clustering.init=kmeans++, k-means++ seeds drawn from a sample of the rows that the same
    pass gathers (clustering/kmeanspp.py).  The tables are integer sums, so resident and streamed rows give the same bytes.
    N comes from the metadata when the rows stream (like the batch plan of the SGD loop) and is checked against what the shards
    deliver.
    Several GPUs, clustering.multi_gpu=views: every rank runs every view -- the result is a pure function of the rows, the ranks
    end in the same state without an exchange -- and rank 0 writes the caches.
    Several GPUs, clustering.multi_gpu=rows (parallel/lloyd_rows.py): `groups` holds THIS rank's shards (rank::world).  The ranks
    exchange their per-shard row counts once, so that every rank numbers the rows as the one-GPU run does; every rank draws every
    permutation, fills the picked rows it owns, and the picks are exchanged bit for bit; the magnitudes are all-reduced with MAX;
    per iteration and live view the int64 tables are all-reduced with SUM, and the changed-label counts once for all views.  Every
    rank then moves its own copy of the centres from the same tables: equal states without a broadcast, the files of the one-GPU
    run.  The sequence of collectives is the same on every rank whatever its rows look like; a rank-local failure of the pre-pass
    travels as a non-finite magnitude and rises on every rank.  force_partitioned: that path with one rank (the test of the
    collectives on the device)."""
    import torch
    from . import kmeanspp, lloyd
    from ..parallel import lloyd_rows
    rank, w = world()
    part = force_partitioned or (w > 1 and multi_gpu_mode(args) != 'views')
    K = int(args.clustering.ncentroids)
    print("training lloyd kmeans for views: {}".format([v[1:] for v in cl]))
    local = _local_shard_counts(groups)
    n_local = sum(local.values())
    if part:
        index = {stem: i for i, stem in enumerate(shard_stems)}
        shard_counts = lloyd_rows.exchange_counts({index[stem]: n for stem, n in local.items()}, len(shard_stems))
        n_total = int(shard_counts.sum())
        print("lloyd: clustering.multi_gpu=rows: the rows are partitioned over {} ranks, rank {} holds {} of {} rows in {} of {} "
              "shards".format(w, rank, n_local, n_total, len(local), len(shard_stems)))
    else:
        n_total = n_local if groups.streamed else len(groups.resident_table())
    if K > n_total:
        raise ValueError("clustering.algorithm=lloyd: clustering.ncentroids={} initial centres cannot be {} distinct rows".format(K, n_total))
    # clustering.init=kmeans++ (a fresh run only; a resumed one ignores the keys as it ignores the picks): the same pass gathers,
    # instead of the K initial rows, the seeding sample -- the first M entries of the same randperm, in ascending order -- into
    # one device tensor per view; the views are then seeded in turn (clustering/kmeanspp.py), each from the uniforms its
    # generator delivers at that point, i.e. after the permutations of all views
    plus = not resumed and kmeanspp.check_init(args) == 'kmeans++'
    if plus:
        M = kmeanspp.sample_size(n_total, K, args.clustering.init_sample)
        T = kmeanspp.trials_for(K, 1 if args.clustering.init_trials is None else args.clustering.init_trials)
    picks, sample = OrderedDict(), OrderedDict()
    if not resumed:
        for v, km in cl.items():
            perm = km._generator.randperm(n_total)
            picks[v] = np.sort(perm[:M]) if plus else perm[:K]
    absmax = OrderedDict((v, 0.0) for v in cl)
    init = OrderedDict((v, np.zeros(km._shape, np.float32)) for v, km in cl.items())
    if part and not resumed:  # the picks this rank owns: (position among the picks, local row), by ascending local row
        owned = OrderedDict()
        for v in cl:
            pos, owner, loc = lloyd_rows.locate_rows(picks[v], shard_counts, w)
            mine = np.flatnonzero(owner == rank)
            mine = mine[np.argsort(loc[mine], kind='stable')]
            owned[v] = (pos[mine], loc[mine])
        got = OrderedDict((v, np.zeros((len(picks[v]), km._shape[1]), np.float32)) for v, km in cl.items())
    base, failure = 0, None
    for _gi, _table, rows in groups.iterate():
        n_g = next(iter(rows.values())).shape[0] if rows else 0
        for v in cl:
            x = rows[v]
            if part:
                try:
                    absmax[v] = max(absmax[v], lloyd.rows_absmax(x))
                except ValueError as exc:  # (a value that is not finite: every rank has to learn of it)
                    absmax[v], failure = float('inf'), failure or "view {}: {}".format('/'.join(v[1:]), exc)
                if not resumed:
                    pos, loc = owned[v]
                    lo, hi = (int(i) for i in np.searchsorted(loc, (base, base + n_g)))
                    if hi > lo:
                        got[v][pos[lo:hi]] = x[torch.from_numpy(loc[lo:hi] - base).to(x.device)].cpu().numpy()
                continue
            absmax[v] = max(absmax[v], lloyd.rows_absmax(x))
            if plus:
                lo, hi = (int(i) for i in np.searchsorted(picks[v], (base, base + n_g)))
                if v not in sample:
                    sample[v] = torch.empty((M, x.shape[1]), dtype=torch.float32, device=x.device)
                if hi > lo:
                    sample[v][lo:hi] = x[torch.from_numpy(picks[v][lo:hi] - base).to(x.device)]
            elif not resumed:
                sel = np.flatnonzero((picks[v] >= base) & (picks[v] < base + n_g))
                if len(sel):
                    init[v][sel] = x[torch.from_numpy(picks[v][sel] - base).to(x.device)].cpu().numpy()
        base += n_g
        del rows
    if part:
        # one MAX over the views' magnitudes and this rank's verdict on its own rows, then the picks view by view: the same
        # collectives on every rank, and a failure anywhere rises everywhere
        if base != n_local:
            failure = failure or "the shards of rank {} delivered {} rows, their metadata states {}".format(rank, base, n_local)
        if failure:
            print("lloyd: rank {}: {}".format(rank, failure))
        merged = lloyd_rows.allreduce_max([absmax[v] for v in cl] + [1.0 if failure else 0.0])
        for v, a in zip(cl, merged):
            absmax[v] = a
        if not resumed:
            dev = _device(args)
            for v in cl:
                rows_v = lloyd_rows.exchange_bits(got[v])
                if plus:
                    sample[v] = torch.from_numpy(rows_v).to(dev)
                else:
                    init[v] = rows_v
            del got
        if merged[-1] != 0:
            raise RuntimeError("clustering.multi_gpu=rows: the pre-pass failed on a rank ({}): fix the metadata or drop the unreadable "
                               "shards from the list".format(failure or "see that rank's log"))
    elif base != n_total:
        raise RuntimeError("the shards delivered {} rows, their metadata states {}: fix the metadata or drop the unreadable shards "
                           "from the list".format(base, n_total))
    if plus:
        for v, km in cl.items():
            x = sample.pop(v)  # (freed before the next view is seeded)
            try:
                seeds, potential = kmeanspp.seed(x, K, T, u=kmeanspp.uniforms(km._generator, 1 + (K - 1) * T))
            except ValueError as exc:
                raise ValueError("view {}: {}".format('/'.join(v[1:]), exc))
            init[v] = x[torch.from_numpy(seeds).to(x.device)].cpu().numpy()
            print("lloyd {}: k-means++ seeds from a sample of {} rows, {} trials per pick: potential {} -> {}".format(
                '/'.join(v[1:]), M, T, int(potential[0]), int(potential[-1])))
            del x
    shift = OrderedDict()
    for v, km in cl.items():
        try:
            shift[v] = lloyd.fixed_point_shift(absmax[v], n_total)
        except ValueError as exc:
            raise ValueError("view {}: {}".format('/'.join(v[1:]), exc))
        if not resumed:
            km.to_lloyd(init[v], spherical=bool(args.clustering.spherical))
        print("lloyd {}: {} rows, {} centres, largest magnitude {:.6g}, fixed point 2^{}".format(
            '/'.join(v[1:]), n_total, K, absmax[v], shift[v]))
    prev = {v: {} for v in cl}  # {view: {row group: the labels of the previous iteration}}
    done = OrderedDict((v, False) for v in cl)
    for epoch in range(pre, pre + iters):
        live = [v for v in cl if not done[v]]
        if not live:
            print("lloyd: every view has converged: cache_epoch_{} holds the final state".format(epoch - 1))
            break
        tables = {v: (None, None) for v in live}
        changed = dict.fromkeys(live, 0)
        for gi, _table, rows in groups.iterate(views=set(live)):
            for v in live:
                labels, sums, counts = lloyd.lloyd_update(cl[v], rows[v], shift[v], *tables[v])
                tables[v] = (sums, counts)
                old = prev[v].get(gi)
                changed[v] += int(labels.numel()) if old is None else int((labels != old).sum())
                prev[v][gi] = labels
            del rows
        if part:
            dev = _device(args)
            for v in live:
                if tables[v][0] is None:  # a rank whose shards hold no row still takes part in every collective
                    tables[v] = (torch.zeros(cl[v]._shape, dtype=torch.int64, device=dev), torch.zeros(K, dtype=torch.int64, device=dev))
                lloyd_rows.allreduce_tables(*tables[v])
            for v, c in zip(live, lloyd_rows.allreduce_sum([changed[v] for v in live])):
                changed[v] = c
        for v in live:
            splits = lloyd.finish_iteration(cl[v], tables[v][0], tables[v][1], shift[v], spherical=cl[v].spherical)
            print("lloyd {}: iteration {}: {} labels changed, {} empty clusters split".format('/'.join(v[1:]), epoch, changed[v], splits))
            if changed[v] == 0:
                done[v] = True
                print("lloyd {}: iteration {} changed no label: converged, no further iteration".format('/'.join(v[1:]), epoch))
        if rank == 0:
            cache.save(args, epoch, cl, groups.fronts)
    return cl


def _train_clusters_planned(args, cl, groups, pre, epochs, b, mode, shard_stems):
    """Multi-GPU training with the rows PARTITIONED over the ranks: `groups` holds THIS rank's shards (rank::world,
    mps/distributed.py:439 -- the node's aggregate HBM holds the rows, nothing streams through one GPU) and a plan
    (parallel/row_plan.py) says which rows form which step's global batch:

      striped     the ONE-GPU batch stream over partitioned rows: one slot, the shards in their global order,
                  batch_size rows per step, `epochs` epochs -- the files of the one-GPU run (and of the default `views` mode,
                  which reads every shard on the training rank instead), the rows resident on the ranks that own them.
      reference   the reference's own N-GPU run (sgd_clustering.py:94-129 under is_distributed): rank q feeds
                  int(batch_size / N) rows per step (data/clustering.py:25) of ITS stream over ALL shards in the rotated
                  order full[q::N] + full[q+1::N] + ... (mps/distributed.py:433-437), ceil(epochs / N) epochs
                  (run_clustering.py:146).  Global batch = batch_size; N * rows / batch_size steps per epoch.
      rows        large batch: every rank feeds batch_size rows of its OWN shards per step (global batch N x batch_size),
                  ceil(epochs / N) epochs -- N x N fewer SGD steps than `reference`; not the reference's run.

    KMeans.train_epoch_plan_multi: the rows of 1 024 steps at a time travel to the rank that runs a clustering's chain
    (clustering v -> rank v % N), no collective on the step path; then the trainers hand out their states.  The state
    equals ONE process fed the same global batches (tests/test_gpu_cli.py); the reference's own all-reduce of per-rank
    deltas differs from that by fp32 re-association in an order NCCL does not promise."""
    import torch.distributed as dist
    from ..parallel import make_plan, plan_warmup_labels
    rank, w = world()
    if groups.streamed:
        raise RuntimeError("clustering.multi_gpu={} keeps every rank's rows resident: {} groups do not fit the device budget "
                           "(raise data.resident_bytes, use more GPUs, or clustering.multi_gpu=views)".format(mode, len(groups.groups)))
    (_gi, table, rows), = list(groups.iterate())
    groups_sizes = getattr(groups, 'all_sizes', None)
    # rows every shard REALLY delivered (an unreadable shard was reported and skipped by the loader: 0 rows), from its owner
    mine = {stem: len(table.shard_rows.get(stem) or ()) for stem in shard_stems[rank::w]}
    everyone = [None] * w
    dist.all_gather_object(everyone, mine)
    have = {}
    for part in everyone:
        have.update(part)
    shard_rows = [int(have.get(stem, 0)) for stem in shard_stems]
    nw_order, tail = loader_settings(args)
    meta_rows = [int(groups_sizes.get(stem, 0)) for stem in shard_stems] if groups_sizes else None
    plan = make_plan(mode, shard_rows, w, b, epochs, num_workers=nw_order, meta_rows=meta_rows, tail=tail)
    seg = [sum(shard_rows[r::w]) for r in range(w)]
    # the reference clamps num_gpus to the number of shards (script.py:22,37); a rank without rows (more GPUs than shards,
    # or every shard of a rank unreadable) or an epoch without a single step would leave untrained clusterings behind
    if min(seg) == 0 or plan.steps == 0:
        raise RuntimeError("clustering.multi_gpu={}: rows per rank {} give {} steps of {} rows -- fewer shards than GPUs, or "
                           "unreadable shards; lower computation.num_gpus".format(mode, seg, plan.steps, plan.global_batch))
    print("rank {}: {} local rows; mode {}: {} steps of {} x {} rows per epoch, {} epochs; loader {}".format(
        rank, seg[rank], mode, plan.steps, plan.slots, plan.lb, plan.epochs, plan.loader))
    kms = list(cl.values())
    xs = [rows[v] for v in cl]
    plan0 = plan
    for epoch in range(pre, pre + plan0.epochs):
        plan = plan0.at_epoch(epoch - pre)  # (the in-process loader's stream continues across epochs when it wraps)
        lr = 0.1 ** (2 + epoch // 5)
        for km in kms:
            km.lr = lr
        _draw_loader_seed(cl)
        # warm-up labels of this rank's slot, then exchanged once per clustering
        local = _draw_warmup(cl, plan.global_batch, plan.steps, plan.lb)
        warm = [plan_warmup_labels(cl[v], plan, device=xs[i].device, mine=local[v], comm_slot=i) for i, v in enumerate(cl)]
        trainers = KMeans.train_epoch_plan_multi(kms, xs, plan, lr=lr, warm_bests=warm)
        for i, km in enumerate(kms):
            km.broadcast_state_from(trainers[i], comm_slot=i)
        if rank == 0:
            cache.save(args, epoch, cl, groups.fronts)
    return cl


def assign_clusters(args, groups, cl, shard_names):
    """run_clustering.py:180-272: label every row of this rank's shards, write {out}/{shard}.pkl."""
    out_dir = Path(args.data.output.path)
    prefix = '' if args.clustering.cached_epoch is None else 'epoch_{}_'.format(args.clustering.cached_epoch)
    print("extracting clustering for views: {}".format([v[1:] for v in cl]))
    # this rank's shards that still have to be written (:248-250), decided from the NAMES: a group without any of them
    # is never read, and only their rows are labelled (every rank sweeping every row would repeat the HBM-bound sweep,
    # the unpickling and the upload `world` times over)
    mine = [s for s in shard_names if not (out_dir / (s + '.pkl')).is_file()]
    saved = []
    writer = io.AssignmentWriter(groups.workers if len(mine) >= 16 else 0)
    mine_set = set(mine)
    for gi, table, rows in groups.iterate(shards=mine):
        todo = [s for s in table.shard_rows if s in mine_set]
        if not todo:
            continue
        sel = rows.pop('_rows', None)  # resident table, several ranks: the rows of this rank's shards, gathered
        labels = OrderedDict()
        for v, km in cl.items():
            best, _ = km.calc_best(rows[v], need_mean=False)
            best = best.cpu().numpy()
            if sel is not None:  # back into table row order (rows of other ranks' shards: never read)
                full = np.full(len(table), -1, np.int64)
                full[sel] = best
                best = full
            labels[v] = best
        for shard in todo:
            ids = table.shard_rows.get(shard)
            if not ids:  # unreadable (reported and skipped by the loader) or empty shard: nothing to write
                continue
            size = table.shard_size[ids[0]]
            if len(ids) < round(size * args.data.output.shard_ok_ratio):
                continue  # too incomplete to save (:261-268)
            out_path = out_dir / (prefix + shard + '.pkl')
            # (sidecar: columnar twin for our own subset-selection loader, opt-in: extra files)
            writer.submit(table, labels, ids, out_path, sidecar=io.sidecar_mode() == 'write')
            saved.append(out_path)
    writer.finish()
    order = {s: i for i, s in enumerate(shard_names)}
    return sorted(saved, key=lambda p: order.get(p.name[len(prefix):-4], 0))


def run_clustering(args):
    rank, w = world()
    check_options(args, w)
    # a cached run (assign-only, resume_training, a cache of a shard subset) whitens with the cache's std or not at all, and
    # projects with the cache's components or not at all
    cached = _cached_attrs(args)
    cache_file, cached_std = cached_whitening(args, cached)
    _, cached_pca = cached_projection(args, cached)
    check_cached_algorithm(args, cached)
    normalize, _spherical = check_normalize(args, w)
    _, cached_norm = cached_normalization(args, cached, normalize)
    if args.clustering.whiten and cache_file is not None and not cached_std:
        raise ValueError("clustering.whiten=True, but the clustering cache {} holds no whiten_std: its centres were trained on "
                         "unwhitened rows".format(cache_file))
    paths = [Path(p) for p in sorted(io.brace_expand(args.data.path))]
    sizes = io.shard_sizes_from_meta(paths, args.data.meta.path, use_cache=True)
    if args.data.meta.path is not None and rank == 0:  # the reference's meta_cache.pkl in the meta dir: read above, kept up to date
        cache_path = Path(args.data.meta.path) / 'meta_cache.pkl'
        try:
            known = dict(io.load_pickle(cache_path)) if cache_path.is_file() else {}
        except Exception:
            known = {}
        if any(k not in known for k in sizes):
            io.dump_pickle({**known, **dict(sizes)}, cache_path)
    paths = [p for p in paths if p.stem in sizes]
    if not paths:
        print(f"All shards of {args.data.path} processing already done!")
        return []
    if args.clustering.algorithm == 'lloyd' and cache_file is None and int(args.clustering.ncentroids) > sum(sizes[p.stem] for p in paths):
        raise ValueError("clustering.algorithm=lloyd: clustering.ncentroids={} initial centres cannot be {} distinct rows".format(
            args.clustering.ncentroids, sum(sizes[p.stem] for p in paths)))
    print(f"processing {len(paths)} shards")
    probe, view_dims = probe_shards(args, paths)
    if probe is None:
        print(f"None of the {len(paths)} shards of {args.data.path} could be read")
        return []
    partitioned = w > 1 and multi_gpu_mode(args) != 'views'
    if partitioned and w > len(paths):  # the reference clamps num_gpus to the number of shards (script.py:22,37)
        raise RuntimeError("clustering.multi_gpu={}: {} GPUs for {} shards -- a rank without shards holds no rows to feed the "
                           "steps; lower computation.num_gpus".format(multi_gpu_mode(args), w, len(paths)))
    # reference / rows mode: a rank reads, holds and labels its own shards only (rank::world) -- training included
    groups = open_row_groups(args, paths[rank::w] if partitioned else paths, sizes, view_dims)
    groups.all_sizes = sizes  # metadata sizes of ALL shards (the loader length of a partitioned run is computed over all of them)
    if cache_file is not None:  # the space the cached centres were trained in; nothing is recomputed
        # (a whitened Lloyd cache with rows: applying a cached std is a per-row function, and the run merges across the ranks)
        lloyd_cache = multi_gpu_mode(args) == 'rows' and all((dt.get('algorithm') or 'sgd') == 'lloyd' for dt in cached[1].values())
        for what, found in (('whitened', cached_std), ('projected', cached_pca)):
            if found and partitioned and not (what == 'whitened' and lloyd_cache):
                raise ValueError("the clustering cache {} is {}: clustering.multi_gpu={} partitions the rows, use views".format(
                    cache_file, what, multi_gpu_mode(args)))
        if cached_norm and partitioned and not lloyd_cache:
            raise ValueError("the clustering cache {} is normalised: clustering.multi_gpu={} partitions the rows of an SGD run, and "
                             "nothing tests that with the row normalisation; use views".format(cache_file, multi_gpu_mode(args)))
        fronts = OrderedDict((v, FrontEnd.from_attrs(cache.find(cached[1], v))) for v in view_dims)
        for v, f in fronts.items():
            f.check_width(v, view_dims[v], " in {}".format(cache_file))
        if cached_std:
            print("whitening with the std of the clustering cache {}".format(cache_file))
        if cached_pca:
            print("projecting with the components of the clustering cache {}".format(cache_file))
        if cached_norm:
            print("normalising the rows as the clustering cache {} says".format(cache_file))
        groups.add_front_ends(fronts)
    else:  # a fresh run: the std, then the scatter matrices of the whitened rows, then the projection, then the row norms
        if args.clustering.whiten:
            stds = compute_whitening(groups, [p.stem for p in paths], view_dims) if partitioned else compute_whitening(groups)
            groups.add_front_ends({v: FrontEnd(std=s) for v, s in stds.items()})
        if args.clustering.pca_dim is not None:
            groups.add_front_ends({v: FrontEnd(pca=f) for v, f in compute_pca(groups, int(args.clustering.pca_dim)).items()})
        if normalize:  # (a function of one row: no pre-pass, and rows that are already resident go through it once)
            groups.add_front_ends({v: FrontEnd(normalize=True) for v in view_dims})
    cl = train_clusters(args, probe, groups, [p.stem for p in paths], cached)
    _report_zero_rows(groups)
    mine = [p.stem for p in paths][rank::w]  # assign: shards strided over ranks (mps/distributed.py:439)
    return assign_clusters(args, groups, cl, mine)


def _report_zero_rows(groups):
    """one line per normalised view: the all-zero rows the normalisation met on the rows that went to the device so far (they
    have no direction and are left as they are; streamed rows are met once per pass)"""
    for v, f in groups.fronts.items():
        if f.normalize:
            print("normalize {}: {} all-zero rows among the {} rows normalised so far (left as they are)".format(
                '/'.join(v[1:]), f.zero_rows, f.rows_normalized))


def store_shards_set(args, saved_paths):
    """clustering/code/save.py:9-17"""
    if len(saved_paths) == 0:
        print("All shards already processed")
        return None
    out_path = saved_paths[0].parent / ('log_' + args.run_id + '.json')
    io.dump_json({**args.run_info, 'shards': [p.stem for p in saved_paths]}, out_path, indent=None)
    return out_path
