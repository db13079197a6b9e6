"""The feature shards of a `cluster` or `evaluate` run as row groups that fit the device budget (_RowGroups), with what sizes and
orders them: the device, its budget, the loader settings and the probe of the first shard that loads."""
import time
from collections import OrderedDict

import numpy as np

from .. import shards as io
from .frontend import FrontEnd


def current_device(args):
    import torch
    return f"cuda:{torch.cuda.current_device()}"


def device_budget(args):
    """bytes of feature rows the device may hold at once: data.resident_bytes / ACAV_RESIDENT_BYTES, else 60 % of the
    free HBM (288 GB on MI355X: cfg2/cfg3's 2 x 4.1 GB are resident, cfg5's 2 x 410 GB stream)"""
    import os
    import torch
    v = os.environ.get('ACAV_RESIDENT_BYTES') or args.data.resident_bytes
    if v:
        return int(float(v))
    free, _total = torch.cuda.mem_get_info()
    return int(free * 0.6)


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


def probe_shards(args, paths):
    """the first shard THAT LOADS tells the views and their widths (the order KMeans objects are created in, and the row size):
    the loader reports and skips an unreadable shard, and an empty probe would create no clustering at all
    -> (its table, {view: columns}), or (None, None) when none loads"""
    for first in paths:
        probe = io.load_feature_shards([first], model_order=list(args.models or []), audio_models=tuple(args.model_types.audio or ()))
        if probe.views:
            return probe, OrderedDict((v, m.shape[1]) for v, m in probe.views.items())
    return None, None


def open_row_groups(args, paths, sizes, view_dims):
    """_RowGroups over paths for the device budget of this run; view_dims: probe_shards'"""
    return _RowGroups(args, paths, sizes, 4 * sum(view_dims.values()), device_budget(args), view_dims)


class _RowGroups:
    """The feature shards as a sequence of ROW GROUPS that fit the device budget.

    The reference never holds more than a batch (clustering/code/data/clustering.py:17-66, run_clustering.py:132-177:
    a DataLoader over the shards, re-read every epoch).  Here a group is as many consecutive shards as fit in half the
    budget (the next group is unpickled / memory-mapped by a host thread while the GPU works on the current one);
    when everything fits there is ONE group and its device tensors stay resident across epochs and the assign sweep.
    Nothing holds [N, d] for all N unless N fits."""

    def __init__(self, args, paths, sizes, row_bytes, budget, view_dims=None, device=current_device):
        import os
        self.args, self.device = args, device  # device: args -> where the rows go
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
        self.fronts = {}  # {view: FrontEnd} of the whitened / projected views (clustering.whiten, clustering.pca_dim), add_front_ends()
        self.t_wait = self.t_upload = 0.0  # main-thread seconds waiting for the loader / copying host -> device (tools/bench_streamed.py)

    def _upload(self, v, m, dev, views=None):
        """host rows of view v -> device: the ONE way feature rows reach the device.  With a front-end set for the view the copy
        goes through it right there (FrontEnd.apply): training, the assign sweep and evaluate see whitened / projected rows,
        the host arrays of the table stay raw.  A view this rank does not need on the device (views) comes back as a zero-width
        host tensor with the right number of rows."""
        import torch
        if views is not None and v not in views:
            return torch.empty((m.shape[0], 0))
        t0 = time.perf_counter()
        t = torch.from_numpy(np.ascontiguousarray(m)).to(dev)
        if v in self.fronts:
            t = self.fronts[v].apply(t)
        self.t_upload += time.perf_counter() - t0
        return t

    def add_front_ends(self, stage):
        """{view: FrontEnd} holding the next stage (the std, then the projection, then the row normalisation, or several at once)
        for every later upload.  Rows
        that are already resident on the device -- uploaded by the pre-pass that computed the stage, with the earlier stage
        applied -- go through this stage here, exactly once and one view at a time: the peak is one extra view."""
        for v, f in stage.items():
            self.fronts[v] = self.fronts.get(v, FrontEnd()).then(f)
        if self._resident is not None:
            on_dev = self._resident[1]
            for v in list(on_dev):
                if v in stage:
                    on_dev[v] = stage[v].apply(on_dev[v])
                    self.fronts[v].zero_rows += stage[v].zero_rows  # (what a row normalisation met is the view's tally)
                    self.fronts[v].rows_normalized += stage[v].rows_normalized

    @property
    def streamed(self):
        return len(self.groups) > 1

    def _prefetch(self, load, jobs):
        """-> (job, load(job)) in order, one job ahead: the next one loads on a host thread while the caller works on this one"""
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1) as pool:
            pending = pool.submit(load, jobs[0]) if jobs else None
            for k, job in enumerate(jobs):
                t0 = time.perf_counter()
                table = pending.result()
                self.t_wait += time.perf_counter() - t0
                if k + 1 < len(jobs):
                    pending = pool.submit(load, jobs[k + 1])  # host work beside the GPU's
                yield job, table

    def resident_table(self):
        """resident data: the table of all rows (reads the shards; uploads nothing yet)"""
        (_gi, table, _rows), = list(self.iterate(views=set()))
        return table

    def iterate_stream(self, paths, extents, lb, row_bytes, budget, views=None):
        """Training order: -> (table, {view: device tensor [rows, d]}) per ROW GROUP of an epoch's batch stream.

        extents: [(shard index into paths, first row, rows)] in delivery order (row_plan.loader_stream), whole batches of lb
        rows in total.  Resident data: ONE group -- the resident rows gathered into stream order on the device (no gather when
        the stream is the rows in order).  Streamed: the stream is cut at batch boundaries where the shards a group touches
        would exceed half the budget; a group loads exactly the shards it touches (a shard the cut falls into is read by both
        neighbours; with worker streams a group touches one shard per worker at a time), uploads them and gathers."""
        import torch
        dev = self.device(self.args)

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
            return self._load([paths[si] for si in sorted({e[0] for e in ext})])

        for ext, table in self._prefetch(load, cuts):
            idx = index_of(table, stems, ext)
            out = OrderedDict()
            for v, m in table.views.items():
                x = self._upload(v, m, dev, views)
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
        dev = self.device(self.args)
        if not self.streamed:
            if self._resident is None:
                self._resident = (self._load(self.groups[0]), OrderedDict())
            table, on_dev = self._resident
            if shards is not None and set(shards) < set(table.shard_rows):
                idx = np.array(sorted(i for s in shards for i in (table.shard_rows.get(s) or ())), np.int64)
                # a view that training left on the device is indexed there (no second copy of the matrix through the host)
                idx_dev = torch.from_numpy(idx).to(dev) if on_dev else None
                rows = OrderedDict((v, on_dev[v][idx_dev] if v in on_dev and (views is None or v in views)
                                    else self._upload(v, m[idx], dev, views)) for v, m in table.views.items())
                rows['_rows'] = idx
                yield 0, table, rows
                return
            rows = OrderedDict()
            for v, m in table.views.items():
                if views is not None and v not in views:
                    rows[v] = self._upload(v, m, dev, views)
                    continue
                if v not in on_dev:
                    on_dev[v] = self._upload(v, m, dev)  # stays resident across epochs and the assign sweep
                rows[v] = on_dev[v]
            yield 0, table, rows
            return
        want = None if shards is None else set(shards)
        todo = [(gi, g if want is None else [p for p in g if p.stem in want]) for gi, g in enumerate(self.groups)]
        for (gi, _g), table in self._prefetch(lambda job: self._load(job[1]), [(gi, g) for gi, g in todo if g]):
            yield gi, table, OrderedDict((v, self._upload(v, m, dev, views)) for v, m in table.views.items())
