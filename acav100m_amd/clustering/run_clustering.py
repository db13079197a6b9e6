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
"""
import math
import pickle
from collections import OrderedDict
from pathlib import Path

import numpy as np

from .. import shards as io
from ..parallel import world
from .lloyd import check_algorithm
from .sgd_clustering import KMeans


def _device(args):
    import torch
    return f"cuda:{torch.cuda.current_device()}"


def _cache_path(args, epoch):
    return Path(args.data.output.path) / "cache_epoch_{}_{}".format(epoch, Path(args.data.path).name)


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


def load_clusterings(args, table, widths=None):
    """run_clustering.py:55-107: resume from cache_epoch_{e}_{name} (or a cache trained on a subset of
    these shards) when --clustering.cached_epoch is set."""
    epoch = args.clustering.cached_epoch
    if isinstance(epoch, int):
        path = _cache_path(args, epoch)
        if not path.is_file() and args.clustering.load_cache_from_shard_subset:
            path = _subset_cache(args, epoch)
        if path is not None and path.is_file():
            saved = _read_cache(path)
            if saved is not None:  # a reference-written file does not name the modality: match on (model_key, layer)
                by_name = {k[1:]: v for k, v in saved.items()}
                saved = {v: saved.get(v, by_name.get(v[1:])) for v in table.views}
                saved = saved if all(x is not None for x in saved.values()) else {}
            if saved is not None and set(saved.keys()) >= set(table.views.keys()):
                print("loading from clustering cache: {}".format(path))
                cl = OrderedDict((v, KMeans.load(saved[v])) for v in table.views)
                for km in cl.values():
                    km.args = args
                return _to_device(args, cl), True
            if saved is not None:
                print("clustering cache features does not match with the given models")
        print("no clustering cache found.")
    return init_clusterings(args, table, widths), False


def _subset_cache(args, epoch):
    want = set(io.brace_expand(Path(args.data.path).name))
    best = None
    for p in Path(args.data.output.path).glob("cache_epoch_{}_*".format(epoch)):
        have = set(io.brace_expand(p.name[p.name.find('shard-'):]))
        if have and not (have - want) and (best is None or len(have) > best[0]):
            best = (len(have), p)
    return None if best is None else best[1]


def _attrs_of(obj):
    """attrs dict of one cached clustering: ours (a dict), or a pickled KMeans object (the reference's default
    scheme, run_clustering.py:110-116, readable when its class is importable)"""
    if isinstance(obj, dict):
        dt = dict(obj)
    elif hasattr(obj, 'get_attrs'):
        dt = dict(obj.get_attrs())
    else:
        dt = dict(vars(obj))
    for key in ('centers', 'counts') + (('whiten_std',) if dt.get('whiten_std') is not None else ()):
        v = dt[key]
        if hasattr(v, 'detach'):
            v = v.detach().cpu().numpy()
        dt[key] = np.ascontiguousarray(v, np.float32)
    if dt.get('pca_components') is not None:
        for key, kind in zip(PCA_KEYS, (np.float32, np.float32, np.float64, np.float64)):
            v = dt[key]
            if hasattr(v, 'detach'):
                v = v.detach().cpu().numpy()
            dt[key] = np.ascontiguousarray(v, kind) if key != 'pca_total_variance' else np.float64(v)
    return dt


# the cache keys of a projected view (clustering.pca_dim): fp32 [d], fp32 [p, d], f64 [p], f64
PCA_KEYS = ('pca_mean', 'pca_components', 'pca_explained_variance', 'pca_total_variance')


def _pca_of(dt):
    """the projection a cached view's attrs hold -> dict(mean, components, explained_variance, total_variance) or None"""
    if dt is None or dt.get('pca_components') is None:
        return None
    return {key[4:]: dt[key] for key in PCA_KEYS}


def _read_cache(path):
    """-> {(kind, model_key, layer): attrs} or None.  The file is the reference's nested
    {model_key: {'layer_i' | 'model': KMeans | attrs}} written by torch.save (run_clustering.py:110-116); the flat
    pickle of round 1 is still accepted.  An unreadable file is reported and treated as absent."""
    import torch
    saved = None
    for reader in (lambda f: torch.load(f, map_location='cpu', weights_only=False), pickle.load):
        try:
            with open(path, 'rb') as f:
                saved = reader(f)
            break
        except Exception as exc:  # zip vs pickle stream, missing classes, truncated file ...
            err = exc
    if saved is None:
        print("clustering cache {} is not loadable: {}".format(path, err))
        return None
    try:
        flat = OrderedDict()
        for key, val in saved.items():
            if isinstance(key, tuple):  # round-1 layout: {(kind, model_key, layer): attrs}
                flat[key] = _attrs_of(val)
                continue
            for layer, obj in val.items():
                dt = _attrs_of(obj)
                flat[(dt.pop('_kind', None), key, layer)] = dt
        return flat
    except Exception as exc:
        print("clustering cache {} has an unknown layout: {}".format(path, exc))
        return None


def save_clusterings(args, epoch, cl, whiten_std=None, pca=None):
    """torch.save of {model_key: {layer: attrs}} -- the reference's file and layout (its save_scheme_ver2 form,
    run_clustering.py:110-116: plain attrs instead of pickled objects, so either side can read it).
    whiten_std: {view: fp32 [d]} of a whitened run (clustering.whiten) -> 'whiten_std' beside '_kind': the centres live in
    x / whiten_std space, and whoever assigns or judges rows with them divides by it first.  An unwhitened run adds no key.
    pca: {view: dict(mean, components, explained_variance, total_variance) | None} of a projected run (clustering.pca_dim) ->
    PCA_KEYS beside it: the centres live in the space of acav_rows_project's output (after the division, if there is one).  An
    unprojected view or run adds no key."""
    import torch
    path = _cache_path(args, epoch)
    print("saving clustering cache to: {}".format(path))
    path.parent.mkdir(parents=True, exist_ok=True)
    nested = OrderedDict()
    for (kind, mk, layer), km in cl.items():
        dt = km.get_attrs_plain()
        dt['_kind'] = kind
        if whiten_std and whiten_std.get((kind, mk, layer)) is not None:
            dt['whiten_std'] = np.ascontiguousarray(whiten_std[kind, mk, layer], np.float32)
        if pca and pca.get((kind, mk, layer)) is not None:
            f = pca[kind, mk, layer]
            dt['pca_mean'] = np.ascontiguousarray(f['mean'], np.float32)
            dt['pca_components'] = np.ascontiguousarray(f['components'], np.float32)
            dt['pca_explained_variance'] = np.ascontiguousarray(f['explained_variance'], np.float64)
            dt['pca_total_variance'] = np.float64(f['total_variance'])
        nested.setdefault(mk, OrderedDict())[layer] = dt
    torch.save(nested, str(path))


def check_whiten(args, world_size):
    """clustering.whiten needs every row of a view on the rank that takes its moments: refused (ValueError) when several GPUs
    partition the ROWS (clustering.multi_gpu = striped / reference / rows).  Pure: no device, no file."""
    if not args.clustering.whiten:
        return
    mode = multi_gpu_mode(args)
    if int(world_size) > 1 and mode != 'views':
        raise ValueError("clustering.whiten with clustering.multi_gpu={} on {} GPUs: the rows are partitioned over the ranks and "
                         "the column moments are not merged across them; use clustering.multi_gpu=views or one GPU".format(
                             mode, world_size))


def check_pca(args, world_size):
    """clustering.pca_dim needs every row of a view on the rank that takes its scatter matrix: refused (ValueError) when several
    GPUs partition the ROWS (clustering.multi_gpu = striped / reference / rows), and when it is not a positive integer.  Pure:
    no device, no file."""
    dim = args.clustering.pca_dim
    if dim is None:
        return
    if isinstance(dim, bool) or not isinstance(dim, int) or dim < 1:
        raise ValueError("clustering.pca_dim must be a positive integer or None, not {!r}".format(dim))
    mode = multi_gpu_mode(args)
    if int(world_size) > 1 and mode != 'views':
        raise ValueError("clustering.pca_dim with clustering.multi_gpu={} on {} GPUs: the rows are partitioned over the ranks and "
                         "the scatter matrices are not merged across them; use clustering.multi_gpu=views or one GPU".format(
                             mode, world_size))


def check_cached_algorithm(args, cached=None):
    """clustering.resume_training continues a cache with the algorithm that trained it: refused (ValueError) when the cache
    clustering.cached_epoch names was trained by the other one ('algorithm' in its states; none: sgd).  No device."""
    path, saved = cached if cached is not None else _cached_attrs(args)
    if path is None or not args.clustering.resume_training:
        return
    want = args.clustering.algorithm or 'sgd'
    for key, dt in saved.items():
        have = dt.get('algorithm') or 'sgd'
        if have != want:
            raise ValueError("clustering.resume_training with clustering.algorithm={}, but view {} of the clustering cache {} was "
                             "trained by {}: a run continues with the algorithm it started with".format(want, '/'.join(key[1:]), path, have))


def _cached_attrs(args):
    """(cache file, {(kind, model_key, layer): attrs}) of the cache that clustering.cached_epoch names -- the file
    load_clusterings will load -- or (None, {}) when there is none"""
    epoch = args.clustering.cached_epoch
    if not isinstance(epoch, int):
        return None, {}
    path = _cache_path(args, epoch)
    if not path.is_file() and args.clustering.load_cache_from_shard_subset:
        path = _subset_cache(args, epoch)
    if path is None or not path.is_file():
        return None, {}
    saved = _read_cache(path)
    if not saved:
        return None, {}
    return path, saved


def cached_whitening(args, cached=None):
    """(cache file, {(model_key, layer): whiten_std}) of the cache that clustering.cached_epoch names -- the file
    load_clusterings will load -- or (None, {}) when there is none.  The cache is authoritative: its std is used as it is, so
    new shards are assigned in the space the centres were trained in."""
    path, saved = cached if cached is not None else _cached_attrs(args)
    return path, {key[1:]: dt['whiten_std'] for key, dt in saved.items() if dt.get('whiten_std') is not None}


def cached_projection(args, cached=None):
    """(cache file, {(model_key, layer): projection}) of that cache, like cached_whitening: nothing is recomputed.  Raises the two
    ValueErrors of a cached run that names the file: clustering.pca_dim set against a cache without the keys, and a pca_dim
    that disagrees with the cached p."""
    path, saved = cached if cached is not None else _cached_attrs(args)
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


def compute_whitening(groups):
    """The stats pre-pass of clustering.whiten: one pass over the row groups, per view one acav_colstats call per group with
    the group's shards as segments, merged in shard order (whiten.ColumnMoments) -> {view: std fp32 [d]}.  Resident data: the
    pass uploads the rows training keeps using.  Streamed data: one extra read of every shard."""
    from .whiten import ColumnMoments
    if groups.streamed:
        print("whitening: the column moments take one extra read of every shard ({} groups stream)".format(len(groups.groups)))
    moments = OrderedDict()
    for _gi, table, rows in groups.iterate():
        prefix = _shard_prefix(table)
        for v, x in rows.items():
            if v not in moments:
                moments[v] = ColumnMoments(x.shape[1], x.device)
            if len(prefix) > 1 and x.shape[1] > 0:
                moments[v].update(x[:prefix[-1]], prefix)
        del rows
    stds = OrderedDict()
    for v, cm in moments.items():
        stds[v] = cm.std()
        print("whitening {}: {} rows, {} zero-variance columns of {} (divided by 1), std min {:.6g} max {:.6g}".format(
            '/'.join(v[1:]), cm.n, cm.zero_columns, cm.d, float(stds[v].min()) if cm.d else 0.0, float(stds[v].max()) if cm.d else 0.0))
    return stds


class _RowGroups:
    """The feature shards as a sequence of ROW GROUPS that fit the device budget.

    The reference never holds more than a batch (clustering/code/data/clustering.py:17-66, run_clustering.py:132-177:
    a DataLoader over the shards, re-read every epoch).  Here a group is as many consecutive shards as fit in half the
    budget (the next group is unpickled / memory-mapped by a host thread while the GPU works on the current one);
    when everything fits there is ONE group and its device tensors stay resident across epochs and the assign sweep.
    Nothing holds [N, d] for all N unless N fits."""

    def __init__(self, args, paths, sizes, row_bytes, budget, view_dims=None):
        import os
        self.args = args
        self.model_order = list(args.models or [])
        self.audio_models = tuple(args.model_types.audio or ())
        # the reference's `computation.num_workers` DataLoader workers (default 40) -> shard-reading worker processes
        # (shards.py: straight into shared memory); ACAV_LOAD_WORKERS overrides, 0 / 1 = read in this process
        nw = os.environ.get('ACAV_LOAD_WORKERS')
        nw = int(nw) if nw is not None else int(args.computation.num_workers or 0)
        self.workers = max(0, min(nw, os.cpu_count() or 1))
        self.sizes, self.view_dims = sizes, view_dims
        self.paths, self.row_bytes, self.budget = list(paths), int(row_bytes), int(budget)
        self._pool_warm = False
        total = sum(sizes[p.stem] for p in paths) * row_bytes
        if total <= budget:
            self.groups = [list(paths)]
        else:
            self.groups, cur, cur_bytes = [], [], 0
            for p in paths:
                nbytes = sizes[p.stem] * row_bytes
                if cur and cur_bytes + nbytes > budget // 2:
                    self.groups.append(cur)
                    cur, cur_bytes = [], 0
                cur.append(p)
                cur_bytes += nbytes
            if cur:
                self.groups.append(cur)
            print("streaming {} shards in {} groups (device budget {:.1f} MB, data {:.1f} MB)".format(
                len(paths), len(self.groups), budget / 1e6, total / 1e6))
        self._resident = None
        self.whiten_std = None  # clustering.whiten: {view: fp32 [d]}, set_whitening()
        self.pca = None  # clustering.pca_dim: {view: projection} of the projected views, set_projection()
        self.t_wait = self.t_upload = 0.0  # main-thread seconds waiting for the loader / copying host -> device (tools/bench_streamed.py)

    def _upload(self, v, m, dev):
        """host rows of view v -> device: the ONE way feature rows reach the device.  With a std set for the view
        (clustering.whiten) the copy is divided by it right there (whiten.whiten_): training, the assign sweep and evaluate see
        whitened rows, the host arrays of the table stay raw.  With a projection set for the view (clustering.pca_dim) the
        whitened copy is projected (pca.project) and dropped: what comes back is [rows, p]."""
        import time
        import torch
        t0 = time.perf_counter()
        t = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        std = None if self.whiten_std is None else self.whiten_std.get(v)
        if std is not None and t.shape[0] and t.shape[1]:
            from .whiten import whiten_
            whiten_(t, std)
        f = None if self.pca is None else self.pca.get(v)
        if f is not None and t.shape[1]:
            from .pca import project
            t = project(t, f['mean'], f['components'])
        self.t_upload += time.perf_counter() - t0
        return t

    def set_projection(self, fits):
        """{view: projection | None} for every later upload.  Rows that are already resident on the device -- uploaded (and
        whitened) at full width by the pre-pass -- are replaced by their projection here, exactly once and one view at a time:
        the peak is one extra view."""
        assert self.pca is None, "the projection of a run is set once"
        from .pca import project
        self.pca = {v: f for v, f in fits.items() if f is not None}
        if self._resident is not None:
            on_dev = self._resident[1]
            for v in list(on_dev):
                f = self.pca.get(v)
                if f is not None and on_dev[v].shape[1]:
                    on_dev[v] = project(on_dev[v], f['mean'], f['components'])

    def set_whitening(self, stds):
        """{view: std} for every later upload.  Rows that are already resident on the device -- uploaded raw by the stats
        pre-pass -- are divided in place here, exactly once."""
        assert self.whiten_std is None, "the whitening of a run is set once"
        from .whiten import whiten_
        self.whiten_std = dict(stds)
        if self._resident is not None:
            for v, x in self._resident[1].items():
                if self.whiten_std.get(v) is not None and x.shape[0] and x.shape[1]:
                    whiten_(x, self.whiten_std[v])

    @property
    def streamed(self):
        return len(self.groups) > 1

    def iterate_stream(self, paths, extents, lb, row_bytes, budget, views=None):
        """Training order: -> (table, {view: device tensor [rows, d]}) per ROW GROUP of an epoch's batch stream.

        extents: [(shard index into paths, first row, rows)] in delivery order (row_plan.loader_stream), whole batches of lb
        rows in total.  Resident data: ONE group -- the resident rows gathered into stream order on the device (no gather when
        the stream is the rows in order).  Streamed: the stream is cut at batch boundaries where the shards a group touches
        would exceed half the budget; a group loads exactly the shards it touches (a shard the cut falls into is read by both
        neighbours; with worker streams a group touches one shard per worker at a time), uploads them and gathers."""
        import torch
        dev = _device(self.args)

        def gather(x, idx):
            if x.shape[1] == 0:
                return torch.empty((len(idx), 0))
            if len(idx) and idx[-1] - idx[0] == len(idx) - 1 and bool((np.diff(idx) == 1).all()):
                return x[int(idx[0]):int(idx[-1]) + 1]  # consecutive rows: a view, no copy
            return x[torch.from_numpy(idx).to(x.device)]

        def index_of(table, stems, ext):
            ids = {si: np.asarray(table.shard_rows.get(stems[si]) or (), np.int64) for si in {e[0] for e in ext}}
            for si, f, n in ext:
                if f + n > len(ids[si]):
                    raise RuntimeError("shard {} delivered {} rows, the batch plan (from its metadata) expects at least {}: fix the "
                                       "metadata or drop the shard from the list".format(stems[si], len(ids[si]), f + n))
            return np.concatenate([ids[si][f:f + n] for si, f, n in ext]) if ext else np.empty(0, np.int64)

        stems = [p.stem for p in paths]
        if not self.streamed:
            for _gi, table, rows in self.iterate(views=views):
                idx = index_of(table, stems, extents)
                in_order = len(idx) > 0 and idx[0] == 0 and idx[-1] == len(idx) - 1 and bool((np.diff(idx) == 1).all())
                # another order (worker streams, a wrapped tail): gathered copies of a few GB of batches at a time -- never a
                # second copy of the resident matrices; the SGD chain simply continues from call to call (as between row groups)
                piece = len(idx) if in_order or not len(idx) else max(lb, min(budget // 8, 4 << 30) // max(1, row_bytes) // lb * lb)
                for a in range(0, len(idx), max(1, piece)):
                    sub = idx[a:a + piece]
                    yield table, OrderedDict((v, gather(x, sub)) for v, x in rows.items())
            return
        # ---- cut the stream into groups
        size = [self.sizes[p.stem] * row_bytes for p in paths]
        cuts, cur, cur_sh, cur_bytes, cur_rows = [], [], set(), 0, 0

        def close():
            nonlocal cur, cur_sh, cur_bytes, cur_rows
            keep, head, acc = cur_rows // lb * lb, [], 0
            rest = []
            for si, f, n in cur:
                if acc + n <= keep:
                    head.append((si, f, n))
                elif acc >= keep:
                    rest.append((si, f, n))
                else:
                    head.append((si, f, keep - acc))
                    rest.append((si, f + keep - acc, n - (keep - acc)))
                acc += n
            if head:
                cuts.append(head)
            cur = rest
            cur_sh = {e[0] for e in cur}
            cur_bytes, cur_rows = sum(size[si] for si in cur_sh), sum(e[2] for e in cur)

        for si, f, n in extents:
            if si not in cur_sh and cur_rows >= lb and cur_bytes + size[si] > budget // 2:
                close()
            cur.append((si, f, n))
            if si not in cur_sh:
                cur_sh.add(si)
                cur_bytes += size[si]
            cur_rows += n
        close()
        assert not cur, "the batch stream is not a whole number of batches"

        def load(ext):
            order = list(OrderedDict.fromkeys(e[0] for e in ext))
            return self._load([paths[si] for si in sorted(order)])

        def up(v, m):
            if views is not None and v not in views:
                return torch.empty((m.shape[0], 0))
            return self._upload(v, m, dev)

        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1) as pool:
            pending = pool.submit(load, cuts[0]) if cuts else None
            for k, ext in enumerate(cuts):
                import time
                t0 = time.perf_counter()
                table = pending.result()
                self.t_wait += time.perf_counter() - t0
                if k + 1 < len(cuts):
                    pending = pool.submit(load, cuts[k + 1])  # host work beside the GPU's
                idx = index_of(table, stems, ext)
                out = OrderedDict()
                for v, m in table.views.items():
                    x = up(v, m)
                    out[v] = gather(x, idx)
                    del x
                yield table, out

    def _load(self, group):
        # streamed: every shard is read once per epoch and once more for the assign sweep.  Since the library reads the pkl
        # files itself (acav_pkl_load_group: 2.1 M rows/s per pass against 2.5 M from the columnar twins and 0.8 M through
        # pickle.load, profiles/r04_streamed_native.txt) a streamed run no longer writes twins on its own: ACAV_SHARD_SIDECAR=write
        sidecar = None
        if self.streamed and not self._pool_warm:  # the worker processes (sidecar reading, assignment writing) start before
            self._pool_warm = True                  # the first host block is registered with the GPU runtime (io.warm_pool)
            io.warm_pool(self.workers)
        return io.load_feature_shards(group, model_order=self.model_order, audio_models=self.audio_models, sidecar=sidecar,
                                      workers=self.workers, expect_rows=self.sizes, expect_views=self.view_dims)

    def __iter__(self):
        return self.iterate()

    def iterate(self, views=None, shards=None):
        """-> (index, table, {view: device tensor [rows, d]}).

        views:  the views this rank needs ON THE DEVICE (None: all).  The others come back as zero-width host tensors with
                the right number of rows -- a rank that trains 1 of 10 clusterings uploads 1 of 10 matrices.
        shards: only these shard stems (None: all).  Streamed: a group without any of them is skipped WITHOUT being read,
                and only the wanted shards of a group are unpickled.  Resident: the rows of the wanted shards are gathered
                on the host and uploaded (N / world rows); `table` stays the full table, and the third item carries
                '_rows' -> the table row indices the gathered rows correspond to."""
        import torch
        dev = _device(self.args)

        def up(v, m):
            if views is not None and v not in views:
                return torch.empty((m.shape[0], 0))
            return self._upload(v, m, dev)

        if not self.streamed:
            if self._resident is None:
                self._resident = (self._load(self.groups[0]), OrderedDict())
            table, on_dev = self._resident
            if shards is not None and set(shards) < set(table.shard_rows):
                idx = np.array(sorted(i for s in shards for i in (table.shard_rows.get(s) or ())), np.int64)
                # a view that training left on the device is indexed there (no second copy of the matrix through the host)
                idx_dev = torch.from_numpy(idx).to(dev) if on_dev else None
                rows = OrderedDict((v, on_dev[v][idx_dev] if v in on_dev and (views is None or v in views) else up(v, m[idx]))
                                   for v, m in table.views.items())
                rows['_rows'] = idx
                yield 0, table, rows
                return
            rows = OrderedDict()
            for v, m in table.views.items():
                if views is not None and v not in views:
                    rows[v] = torch.empty((m.shape[0], 0))
                    continue
                if v not in on_dev:
                    on_dev[v] = up(v, m)  # stays resident across epochs and the assign sweep
                rows[v] = on_dev[v]
            yield 0, table, rows
            return
        want = None if shards is None else set(shards)
        todo = [(gi, g if want is None else [p for p in g if p.stem in want]) for gi, g in enumerate(self.groups)]
        todo = [(gi, g) for gi, g in todo if g]
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1) as pool:
            pending = pool.submit(self._load, todo[0][1]) if todo else None
            for k, (gi, _g) in enumerate(todo):
                import time
                t0 = time.perf_counter()
                table = pending.result()
                self.t_wait += time.perf_counter() - t0
                if k + 1 < len(todo):
                    pending = pool.submit(self._load, todo[k + 1][1])  # host work beside the GPU's
                yield gi, table, OrderedDict((v, up(v, m)) for v, m in table.views.items())


def loader_settings(args):
    """(computation.num_workers as the batch ORDER sees it, tail) -- config.py: data.loader_order / data.loader_tail"""
    import os
    mode = str(os.environ.get('ACAV_LOADER_ORDER') or args.data.loader_order or 'reference').lower()
    if mode not in ('reference', 'workers', 'single'):
        raise ValueError("data.loader_order / ACAV_LOADER_ORDER must be 'reference' or 'single', not {!r}".format(mode))
    tail = str(os.environ.get('ACAV_LOADER_TAIL') or args.data.loader_tail or 'wrap').lower()
    if tail not in ('wrap', 'drop'):
        raise ValueError("data.loader_tail / ACAV_LOADER_TAIL must be 'wrap' or 'drop', not {!r}".format(tail))
    return (0 if mode == 'single' else int(args.computation.num_workers or 0)), tail


def _device_budget(args):
    """bytes of feature rows the device may hold at once: data.resident_bytes / ACAV_RESIDENT_BYTES, else 60 % of the
    free HBM (288 GB on MI355X: cfg2/cfg3's 2 x 4.1 GB are resident, cfg5's 2 x 410 GB stream)"""
    import os
    import torch
    v = os.environ.get('ACAV_RESIDENT_BYTES') or args.data.resident_bytes
    if v:
        return int(float(v))
    free, _total = torch.cuda.mem_get_info()
    return int(free * 0.6)


def train_clusters(args, probe, groups, shard_stems=()):
    import torch
    # a projected view (clustering.pca_dim) trains at d = p
    widths = {v: f['components'].shape[0] for v, f in (groups.pca or {}).items()}
    cl, loaded = load_clusterings(args, probe, widths)
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
        return _train_clusters_lloyd(args, cl, groups, pre, epochs, loaded)
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
        (_gi, table, _rows), = list(groups.iterate(views=set()))  # (reads the shards; uploads nothing yet)
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
        # `for batch in dataloader` (run_clustering.py:235) creates a DataLoader iterator, which draws its
        # 64-bit base seed from the global CPU generator (torch/utils/data/dataloader.py,
        # _BaseDataLoaderIter.__init__: torch.empty((), dtype=int64).random_()) = two mt19937 words per
        # epoch, between the centre initialisation and the first warm-up draw.  Consumed here so that a
        # seeded run reproduces the reference CLI's files bit for bit (tests/test_gpu_cli.py).
        gen = next(iter(cl.values()))._generator
        gen.u32()
        gen.u32()
        # several GPUs: a rank only trains (hence only uploads) its share of the views -- view i -> rank i % world
        own = None if w == 1 else {v for i, v in enumerate(cl) if i % w == rank}
        ext = shard_extents(plan.at_epoch(epoch - pre))
        for table, part in groups.iterate_stream(paths, ext, b, row_bytes, budget, views=own):
            n = next(iter(part.values())).shape[0] if part else 0
            assert n % b == 0
            steps = n // b
            if steps == 0:
                continue
            # warm-up labels, drawn batch by batch across the clusterings like the reference loop (every rank draws
            # all of them from the same stream, so the generators stay in step whoever trains which clustering)
            need = {v: km.warmup_steps(b, steps) for v, km in cl.items()}
            warm = {v: np.empty((need[v], b), np.int64) for v in cl}
            for t in range(max(need.values(), default=0)):
                for v, km in cl.items():
                    if t < need[v]:
                        warm[v][t] = km.draw_warmup(b)
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
            save_clusterings(args, epoch, cl, groups.whiten_std, groups.pca)
    return cl


def _train_clusters_lloyd(args, cl, groups, pre, iters, resumed):
    """clustering.algorithm=lloyd: `iters` iterations of batch k-means per view (clustering/lloyd.py), each one pass over the row
    groups with two sweeps per view -- the assign sweep and acav_lloyd_accumulate into int64 tables on the device -- and the centre
    update on the host.  Before the first one, one read-once pass takes every view's largest magnitude (the scale of the fixed
    point) and, for a fresh run, the initial centres: the rows generator.randperm(N)[:K], drawn view by view, read as the
    front-ends deliver them.  The tables are integer sums, so resident and streamed rows give the same bytes.  N comes from the
    metadata when the rows stream (like the batch plan of the SGD loop) and is checked against what the shards deliver.
    Several GPUs (clustering.multi_gpu=views): every rank runs every view -- the result is a pure function of the rows, the ranks
    end in the same state without an exchange -- and rank 0 writes the caches."""
    import torch
    from . import lloyd
    rank, _w = world()
    K = int(args.clustering.ncentroids)
    print("training lloyd kmeans for views: {}".format([v[1:] for v in cl]))
    if groups.streamed:
        n_total = sum(int(groups.sizes[p.stem]) for p in groups.paths)
    else:
        (_gi, table, _rows), = list(groups.iterate(views=set()))  # (reads the shards; uploads nothing yet)
        n_total = len(table)
    if K > n_total:
        raise ValueError("clustering.algorithm=lloyd: clustering.ncentroids={} initial centres cannot be {} distinct rows".format(K, n_total))
    picks = OrderedDict()
    if not resumed:
        for v, km in cl.items():
            picks[v] = km._generator.randperm(n_total)[:K]
    absmax = OrderedDict((v, 0.0) for v in cl)
    init = OrderedDict((v, np.zeros(km._shape, np.float32)) for v, km in cl.items())
    base = 0
    for _gi, _table, rows in groups.iterate():
        n_g = next(iter(rows.values())).shape[0] if rows else 0
        for v in cl:
            x = rows[v]
            absmax[v] = max(absmax[v], lloyd.rows_absmax(x))
            if not resumed:
                sel = np.flatnonzero((picks[v] >= base) & (picks[v] < base + n_g))
                if len(sel):
                    init[v][sel] = x[torch.from_numpy(picks[v][sel] - base).to(x.device)].cpu().numpy()
        base += n_g
        del rows
    if base != n_total:
        raise RuntimeError("the shards delivered {} rows, their metadata states {}: fix the metadata or drop the unreadable shards "
                           "from the list".format(base, n_total))
    shift = OrderedDict()
    for v, km in cl.items():
        try:
            shift[v] = lloyd.fixed_point_shift(absmax[v], n_total)
        except ValueError as exc:
            raise ValueError("view {}: {}".format('/'.join(v[1:]), exc))
        if not resumed:
            km.to_lloyd(init[v])
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
        for v in live:
            splits = lloyd.finish_iteration(cl[v], tables[v][0], tables[v][1], shift[v])
            print("lloyd {}: iteration {}: {} labels changed, {} empty clusters split".format('/'.join(v[1:]), epoch, changed[v], splits))
            if changed[v] == 0:
                done[v] = True
                print("lloyd {}: iteration {} changed no label: converged, no further iteration".format('/'.join(v[1:]), epoch))
        if rank == 0:
            save_clusterings(args, epoch, cl, groups.whiten_std, groups.pca)
    return cl


def multi_gpu_mode(args):
    """clustering.multi_gpu: 'views' (default), 'striped', 'reference' or 'rows' -- see config.py"""
    mode = str(args.clustering.multi_gpu or 'views')
    if mode not in ('views', 'striped', 'reference', 'rows'):
        raise ValueError("clustering.multi_gpu must be 'views', 'striped', 'reference' or 'rows', not {!r}".format(mode))
    return mode


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
    import torch
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
        gen = kms[0]._generator  # the DataLoader iterator's seed draw, as in the one-GPU loop (every rank creates its own)
        gen.u32()
        gen.u32()
        # warm-up labels of this rank's slot, drawn batch by batch across the clusterings like the reference loop
        # (run_clustering.py:170-175 steps every clustering per batch), then exchanged once per clustering
        need = [km.warmup_steps(plan.global_batch, plan.steps) for km in kms]
        local = [np.empty((nd, plan.lb), np.int64) for nd in need]
        for t in range(max(need, default=0)):
            for i, km in enumerate(kms):
                if t < need[i]:
                    local[i][t] = km.draw_warmup(plan.lb)
        warm = [plan_warmup_labels(km, plan, device=xs[i].device, mine=local[i], comm_slot=i) for i, km in enumerate(kms)]
        trainers = KMeans.train_epoch_plan_multi(kms, xs, plan, lr=lr, warm_bests=warm)
        for i, km in enumerate(kms):
            km.broadcast_state_from(trainers[i], comm_slot=i)
        if rank == 0:
            save_clusterings(args, epoch, cl, groups.whiten_std)
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
    check_whiten(args, w)
    check_pca(args, w)
    check_algorithm(args, w)
    # a cached run (assign-only, resume_training, a cache of a shard subset) whitens with the cache's std or not at all, and
    # projects with the cache's components or not at all
    cached = _cached_attrs(args)
    cache_file, cached_std = cached_whitening(args, cached)
    _, cached_pca = cached_projection(args, cached)
    check_cached_algorithm(args, cached)
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
    # the first shard THAT LOADS tells the views and their widths (the order KMeans objects are created in, and the row
    # size): the loader reports and skips an unreadable shard, and an empty probe would create no clustering at all
    for first in paths:
        probe = io.load_feature_shards([first], model_order=list(args.models or []),
                                       audio_models=tuple(args.model_types.audio or ()))
        if probe.views:
            break
    else:
        print(f"None of the {len(paths)} shards of {args.data.path} could be read")
        return []
    row_bytes = 4 * sum(m.shape[1] for m in probe.views.values())
    view_dims = OrderedDict((v, m.shape[1]) for v, m in probe.views.items())
    partitioned = w > 1 and multi_gpu_mode(args) != 'views'
    if partitioned and w > len(paths):  # the reference clamps num_gpus to the number of shards (script.py:22,37)
        raise RuntimeError("clustering.multi_gpu={}: {} GPUs for {} shards -- a rank without shards holds no rows to feed the "
                           "steps; lower computation.num_gpus".format(multi_gpu_mode(args), w, len(paths)))
    # reference / rows mode: a rank reads, holds and labels its own shards only (rank::world) -- training included
    groups = _RowGroups(args, paths[rank::w] if partitioned else paths, sizes, row_bytes, _device_budget(args), view_dims)
    groups.all_sizes = sizes  # metadata sizes of ALL shards (the loader length of a partitioned run is computed over all of them)
    if cached_std:  # the space the cached centres were trained in; nothing is recomputed
        if partitioned:
            raise ValueError("the clustering cache {} is whitened: clustering.multi_gpu={} partitions the rows, use views".format(
                cache_file, multi_gpu_mode(args)))
        stds = OrderedDict((v, cached_std.get(v[1:])) for v in view_dims)
        for v, s in stds.items():
            if s is not None and s.shape != (view_dims[v],):
                raise ValueError("whiten_std of view {} in {} has shape {}, the rows have {} columns".format(
                    '/'.join(v[1:]), cache_file, s.shape, view_dims[v]))
        print("whitening with the std of the clustering cache {}".format(cache_file))
        groups.set_whitening(stds)
    elif args.clustering.whiten:
        groups.set_whitening(compute_whitening(groups))
    if cached_pca:  # likewise
        if partitioned:
            raise ValueError("the clustering cache {} is projected: clustering.multi_gpu={} partitions the rows, use views".format(
                cache_file, multi_gpu_mode(args)))
        fits = OrderedDict((v, cached_pca.get(v[1:])) for v in view_dims)
        for v, f in fits.items():
            if f is not None and (f['components'].ndim != 2 or f['components'].shape[1] != view_dims[v]
                                  or f['mean'].shape != (view_dims[v],)):
                raise ValueError("pca_components of view {} in {} has shape {}, the rows have {} columns".format(
                    '/'.join(v[1:]), cache_file, f['components'].shape, view_dims[v]))
        print("projecting with the components of the clustering cache {}".format(cache_file))
        groups.set_projection(fits)
    elif args.clustering.pca_dim is not None and cache_file is None:
        groups.set_projection(compute_pca(groups, int(args.clustering.pca_dim)))
    cl = train_clusters(args, probe, groups, [p.stem for p in paths])
    mine = [p.stem for p in paths][rank::w]  # assign: shards strided over ranks (mps/distributed.py:439)
    return assign_clusters(args, groups, cl, mine)


def store_shards_set(args, saved_paths):
    """clustering/code/save.py:9-17"""
    if len(saved_paths) == 0:
        print("All shards already processed")
        return None
    out_path = saved_paths[0].parent / ('log_' + args.run_id + '.json')
    io.dump_json({**args.run_info, 'shards': [p.stem for p in saved_paths]}, out_path, indent=None)
    return out_path
