"""Batch (Lloyd) k-means for the clustering stage: every pass assigns each row to its nearest centre and moves each centre to the
mean of its rows -- what the clusterers of the reference's correspondence_retrieval/code/clustering.py run (clustering_func_type =
'faiss', the default of its args.py:18, and 'scipy': `niters` full passes).  clustering.algorithm=lloyd selects it.

Definition of one iteration on rows x [N, d] (fp32, after the whiten / PCA front-ends) and centres c [K, d]:
  labels   the first-index argmin of the package's canonical fp32 distance: the acav_kmeans_assign sweep of a KMeans whose
           hyper-parameters are initial_rounds = 0, reinit = (.7, 1.0) -- no warm-up, and a discount that divides by exactly 1.
           The sweep's half-precision filter stays on: its acceptance bound is stated for the undiscounted distances and holds for
           a discounted one whenever 1 / r <= 1; at r = 1 the factor is the exact 1.0f.
  sums     sums[k][j] = sum over the rows labelled k of rint(double(x_ij) * 2^s) in int64, counts[k] = their number
           (acav_lloyd_accumulate), s = fixed_point_shift(absmax of all rows, N): integer sums, so the tables do not depend on the
           summation order, the device, the row groups or resident versus streamed rows
  centres  np.float32(sums.astype(float64) * 2.0**-s / counts) -- acav_lloyd_centers on device tables, the same three rounded
           operations, and numpy on the host when a cluster is empty or the tables are host arrays; then the empty clusters in
           ascending order
           (split_empty, after faiss's split_clusters): the currently largest cluster j (lowest index on ties) is split, c_i = c_j
           with the even columns of c_i times 1 + 1/1024 and of c_j times 1 - 1/1024, the odd columns the other way round, and i
           takes floor(count_j / 2) of j's count.
  spherical (clustering.spherical; faiss's Kmeans(spherical=True)): the rows are L2-normalised (clustering/normalize.py), and after
           the steps above the [K, d] centre table is normalised row by row with the same kernel (acav_rows_normalize) -- on the
           device, in the one place finish_iteration.  A cluster whose fp32 mean is exactly the zero vector (its rows cancel) counts
           as empty: its count is set to 0 before the empty-cluster rule, which then splits the largest cluster into it.  With unit
           rows and unit centres the Euclidean argmin of the assign sweep is the cosine argmax: the sweep is untouched.
The assignment and the sums are GPU sweeps (there is no CPU path); tests/_lloyd_np.py restates the iteration in numpy bit for bit
(tests/_rownorm_np.py: the spherical one).
Several GPUs with the rows partitioned (clustering.multi_gpu=rows): the tables are integers, so their all-reduced sum is the
one-GPU run's table whoever added what -- parallel/lloyd_rows.py and run_clustering._train_clusters_lloyd."""
import ctypes as C
import math

import numpy as np

from .. import _lib
from .options import multi_gpu_mode, needs_every_row
from .sgd_clustering import KMeans, _as_f32_2d, _device_index

ALGORITHMS = ('sgd', 'lloyd')
CALL_ROWS = 1 << 30        # rows of one acav_lloyd_accumulate call (its positions are 32-bit)
SPLIT_EPS = np.float32(1.0 / 1024)


def check_algorithm(args, world_size=1, merges=()):
    """clustering.algorithm is 'sgd' or 'lloyd'.  lloyd over several GPUs needs every row of a view on every rank
    (clustering.multi_gpu=views) unless the caller merges the cluster sums across the ranks: merges names the partitioned modes in
    which it does.  The clustering stage does in 'rows' (run_clustering.check_options passes merges=('rows',): the int64 tables are
    all-reduced); 'striped' and 'reference' name batch streams of the SGD chain and are merged by nobody.  A caller that states no
    merge is refused every partitioned mode, as before.  Pure: no device, no file.  -> the algorithm"""
    algo = 'sgd' if args.clustering.algorithm is None else args.clustering.algorithm  # (a hand-built args tree without the key)
    if not isinstance(algo, str) or algo not in ALGORITHMS:
        raise ValueError("clustering.algorithm must be 'sgd' or 'lloyd', not {!r}".format(algo))
    if algo == 'lloyd':
        mode = multi_gpu_mode(args)
        if int(world_size) > 1 and mode in ('striped', 'reference'):
            raise ValueError("clustering.algorithm=lloyd with clustering.multi_gpu={} on {} GPUs: the rows are partitioned over the "
                             "ranks and the cluster sums are not merged across them in a mode that names a batch stream of the SGD "
                             "chain (lloyd partitions its rows with clustering.multi_gpu=rows); use clustering.multi_gpu=views or one "
                             "GPU".format(mode, world_size))
        if mode not in merges:
            needs_every_row(args, world_size, "clustering.algorithm=lloyd", "cluster sums")
        if isinstance(args.clustering.epochs, bool) or int(args.clustering.epochs) < 1:
            raise ValueError("clustering.epochs={!r}: lloyd needs at least one iteration".format(args.clustering.epochs))
    return algo


def fixed_point_shift(absmax, n):
    """s with |x * 2^s| < 2^62 / n for every |x| <= absmax: with (m, E) = frexp(absmax), s = 62 - ceil(log2(max(n, 2))) - E"""
    absmax, n = float(absmax), int(n)
    if not math.isfinite(absmax) or absmax < 0:
        raise ValueError("absmax = {!r} is not a finite magnitude".format(absmax))
    if absmax == 0:
        raise ValueError("every feature value is 0: there is nothing to cluster")
    if n < 1:
        raise ValueError("n = {} rows".format(n))
    _m, e = math.frexp(absmax)
    return 62 - (max(n, 2) - 1).bit_length() - e


def rows_absmax(x, device="cuda"):
    """max |x_ij| of x [n, d] (numpy, or a torch tensor on the host or the device) as a python float: acav_rows_absmax.  A value
    that is not finite is a ValueError."""
    keep, xp, n, on_gpu = _as_f32_2d(x)
    d = int(keep.shape[1])
    if n == 0 or d == 0:
        return 0.0
    out = C.c_float(0)
    lib = _lib.load_library()
    _lib.check(lib.acav_rows_absmax(keep.device.index if on_gpu else _device_index(device), xp, n, d, C.byref(out), None))
    return float(out.value)


def accumulate(x, labels, s, sums, counts):
    """sums [k, d] += the fixed-point rows of x [n, d] by label, counts [k] += 1 per row (acav_lloyd_accumulate).  x and labels:
    numpy or torch, host or device; sums and counts: int64, both numpy arrays or both contiguous torch tensors on the GPU,
    updated in place."""
    k, d = int(sums.shape[0]), int(sums.shape[1])
    keep, xp, n, on_gpu = _as_f32_2d(x, d)
    on_dev = hasattr(sums, "data_ptr")
    if on_dev:
        import torch
        if not (sums.is_cuda and counts.is_cuda and sums.dtype == torch.int64 and counts.dtype == torch.int64
                and sums.is_contiguous() and counts.is_contiguous()):
            raise ValueError("sums and counts must be contiguous int64 tensors on the GPU (or numpy arrays)")
        torch.cuda.current_stream(sums.device).synchronize()
        device = sums.device.index
    else:
        if not (isinstance(sums, np.ndarray) and isinstance(counts, np.ndarray) and sums.dtype == np.int64 and counts.dtype == np.int64
                and sums.flags.c_contiguous and counts.flags.c_contiguous):
            raise ValueError("sums and counts must be C-contiguous int64 numpy arrays (or tensors on the GPU)")
        device = keep.device.index if on_gpu else _device_index("cuda")
    if tuple(counts.shape) != (k,):
        raise ValueError("counts has shape {}, sums {}".format(tuple(counts.shape), tuple(sums.shape)))
    if hasattr(labels, "data_ptr"):
        import torch
        lab = labels.detach().to(torch.long).contiguous()
        if lab.is_cuda:
            torch.cuda.current_stream(lab.device).synchronize()
    else:
        lab = np.ascontiguousarray(labels, np.int64)
    if tuple(lab.shape) != (n,):
        raise ValueError("expected {} labels, got shape {}".format(n, tuple(lab.shape)))
    lib = _lib.load_library()
    for a in range(0, n, CALL_ROWS):
        m = min(CALL_ROWS, n - a)
        _lib.check(lib.acav_lloyd_accumulate(device, C.c_void_p(xp.value + 4 * d * a), m, d, C.c_void_p(_lib.ptr(lab).value + 8 * a), k,
                                             int(s), _lib.ptr(sums), _lib.ptr(counts), None))


def accumulate_plan(hist, d, cus=256):
    """how acav_lloyd_accumulate cuts the lists of a label histogram -> (dict of the launch shape, chunks int64 [chunks, 3] =
    (label, first position, rows)); pure: no device"""
    hist = np.ascontiguousarray(hist, np.int64)
    lib = _lib.load_library()
    out = (C.c_int64 * 9)()
    _lib.check(lib.acav_lloyd_accumulate_plan(_lib.ptr(hist), len(hist), int(d), int(cus), out, None, 0))
    chunks = np.empty((int(out[1]), 3), np.int64)
    _lib.check(lib.acav_lloyd_accumulate_plan(_lib.ptr(hist), len(hist), int(d), int(cus), out, _lib.ptr(chunks), len(chunks)))
    keys = ('chunk_rows', 'chunks', 'strips', 'items', 'grid', 'bin_grid', 'bin_rows', 'lds_bins', 'scratch')
    return dict(zip(keys, (int(v) for v in out))), chunks


def split_empty(centers, counts):
    """The empty-cluster rule, in place on centers fp32 [K, d] and counts int64 [K] -> number of splits.  Empty clusters in
    ascending order; each takes the currently largest cluster j (lowest index on ties): c_i = c_j, even columns of c_i times
    1 + 1/1024 and of c_j times 1 - 1/1024, odd columns the other way round; i gets floor(count_j / 2), taken from j."""
    up, down = np.float32(1) + SPLIT_EPS, np.float32(1) - SPLIT_EPS
    splits = 0
    for i in np.flatnonzero(counts == 0):
        j = int(np.argmax(counts))
        centers[i] = centers[j]
        centers[i, 0::2] *= up
        centers[i, 1::2] *= down
        centers[j, 0::2] *= down
        centers[j, 1::2] *= up
        counts[i] = counts[j] // 2
        counts[j] -= counts[i]
        splits += 1
    return splits


def centers_from_sums(sums, counts, s, zero_mean_is_empty=False):
    """(sums int64 [K, d], counts int64 [K], s) -> (centers fp32 [K, d], sizes int64 [K], splits): the mean of every cluster
    rounded to fp32, then the empty-cluster rule.  zero_mean_is_empty (a spherical iteration): a cluster whose fp32 mean is the
    zero vector has no direction; its count is set to 0 first, so the rule treats it as empty."""
    sums, counts = np.asarray(sums, np.int64), np.array(counts, np.int64)
    if int(counts.sum()) == 0:
        raise ValueError("no row was accumulated: there is no centre to compute")
    with np.errstate(invalid='ignore', divide='ignore'):
        centers = np.float32(sums.astype(np.float64) * 2.0 ** -int(s) / counts[:, None].astype(np.float64))
    centers[counts == 0] = 0  # (0 / 0 above; split_empty overwrites every one of them)
    if zero_mean_is_empty:
        counts[~centers.any(axis=1)] = 0
    splits = split_empty(centers, counts)
    return centers, counts, splits


def centers_on_device(sums, counts, s):
    """(sums int64 [K, d], counts int64 [K]: contiguous tensors on one GPU, s) -> (centers fp32 [K, d], sizes fp32 [K], both
    tensors on that GPU, number of empty clusters): acav_lloyd_centers -- centers_from_sums before the empty-cluster rule, an
    empty cluster a row of zeros"""
    import torch
    if not (hasattr(sums, "is_cuda") and sums.is_cuda and counts.is_cuda and sums.dtype == torch.int64 and counts.dtype == torch.int64
            and sums.is_contiguous() and counts.is_contiguous() and sums.dim() == 2 and sums.device == counts.device):
        raise ValueError("sums and counts must be contiguous int64 tensors on one GPU")
    k, d = int(sums.shape[0]), int(sums.shape[1])
    if tuple(counts.shape) != (k,):
        raise ValueError("counts has shape {}, sums {}".format(tuple(counts.shape), tuple(sums.shape)))
    centers = torch.empty((k, d), dtype=torch.float32, device=sums.device)
    sizes = torch.empty(k, dtype=torch.float32, device=sums.device)
    torch.cuda.current_stream(sums.device).synchronize()  # the library runs on its own stream
    empty = C.c_int64(0)
    _lib.check(_lib.load_library().acav_lloyd_centers(sums.device.index, _lib.ptr(sums), _lib.ptr(counts), k, d, int(s), _lib.ptr(centers),
                                                      _lib.ptr(sizes), C.byref(empty), None))
    return centers, sizes, int(empty.value)


def lloyd_update(km, x, s, sums=None, counts=None):
    """The two sweeps of one iteration over the rows x [n, d] (on the GPU) of one row group: labels of km's current centres
    (calc_best, need_mean=False), their fixed-point sums and counts added into sums / counts (int64 tensors on x's device,
    created zeroed when None) -> (labels, sums, counts).  finish_iteration moves the centres once every group is in."""
    import torch
    if km.algorithm != 'lloyd':
        raise _lib.AcavError("lloyd_update needs a KMeans in its lloyd state: call KMeans.to_lloyd() first")
    k, d = km._shape
    if sums is None:
        sums = torch.zeros((k, d), dtype=torch.int64, device=x.device)
        counts = torch.zeros(k, dtype=torch.int64, device=x.device)
    labels, _ = km.calc_best(x, need_mean=False)
    accumulate(x, labels, s, sums, counts)
    return labels, sums, counts


def finish_iteration(km, sums, counts, s, spherical=False):
    """centres <- mean of their rows (+ the empty-cluster rule), counts <- the cluster sizes, count += the rows of the
    iteration -> number of splits.  Tables on the device (torch tensors) take acav_lloyd_centers: the centres go from device
    to device into km's handle and no table crosses the bus; when it reports an empty cluster, the iteration takes the host path
    below (split_empty is sequential and rare).  Host tables (numpy) take the host path.
    spherical: the centre table is then normalised row by row on the device (normalize.normalize_: acav_rows_normalize), whichever
    path made it.  A zero row it meets on the device path is a cluster whose mean is the zero vector: the table is dropped and the
    iteration takes the host path, where such a cluster's count is set to 0 in front of the empty-cluster rule."""
    if spherical:
        from .normalize import normalize_
        if km._h is None:
            raise _lib.AcavError("a spherical iteration normalises its centres on the GPU: call KMeans.to('cuda') first")
    if hasattr(sums, "data_ptr") and sums.is_cuda and km._h is not None:
        centers, sizes, empty = centers_on_device(sums, counts, s)
        if empty == 0 and spherical:
            empty = normalize_(centers)[1]
        if empty == 0:
            n = int(counts.sum())
            _lib.check(_lib._lib.acav_kmeans_set_state(km._h, _lib.ptr(centers), _lib.ptr(sizes), km.count + n, km.fallback))
            return 0
    sums_h = sums.cpu().numpy() if hasattr(sums, "cpu") else sums
    counts_h = counts.cpu().numpy() if hasattr(counts, "cpu") else counts
    n = int(counts_h.sum())
    if not spherical:
        centers, sizes, splits = centers_from_sums(sums_h, counts_h, s)
        km.load_state_arrays(centers, sizes.astype(np.float32), km.count + n, km.fallback)
        return splits
    import torch
    centers, sizes, splits = centers_from_sums(sums_h, counts_h, s, zero_mean_is_empty=True)
    table = torch.from_numpy(centers).to("cuda:{}".format(km._device))
    if normalize_(table)[1]:
        raise ValueError("a centre is the zero vector after the empty-cluster rule: every cluster's rows cancel")
    km.load_state_arrays(table.cpu().numpy(), sizes.astype(np.float32), km.count + n, km.fallback)
    return splits


class FitReport(list):
    """fit's report: the list of (changed labels, splits) per iteration; potential: the potentials int64 [k] of a k-means++
    seeding (None with init='random')"""
    potential = None


def fit(x, k, iters, generator=None, device="cuda", init='random', trials=1, sample=None, normalize=False, spherical=False):
    """Lloyd k-means of x [n, d] (numpy or a torch tensor) in one resident piece -> (KMeans in its lloyd state, labels of the last
    iteration's assignment, report: per iteration (changed labels, splits)).  Initial centres: the rows generator.randperm(n)[:k]
    (init='random'), or (init='kmeans++', clustering/kmeanspp.py) k-means++ seeds with `trials` trials per pick on the sample
    made of the first min(n, sample or 256 k) entries of the same permutation, in ascending order -- the uniforms are the
    generator's draws after the permutation, and report.potential holds the seeding's potentials, int64 [k].
    Stops early when an iteration changes no label.
    normalize: the rows are L2-normalised first (a copy: x stays what it is); spherical: implies it, and every iteration
    renormalises the centres (finish_iteration) -- the state then carries 'spherical'."""
    import torch
    from . import kmeanspp
    if init not in kmeanspp.INITS:
        raise ValueError("init must be 'random' or 'kmeans++', not {!r}".format(init))
    dev = x.device if hasattr(x, "is_cuda") and x.is_cuda else torch.device("cuda:{}".format(_device_index(device)))
    t = (x.detach() if hasattr(x, "data_ptr") else torch.from_numpy(np.ascontiguousarray(x, np.float32))).to(dev, torch.float32).contiguous()
    if normalize or spherical:
        from .normalize import normalize_
        if hasattr(x, "data_ptr") and t.data_ptr() == x.data_ptr():
            t = t.clone()
        normalize_(t)
    n, d = t.shape
    if k > n:
        raise ValueError("{} centres from {} rows: K > N".format(k, n))
    from ..rng import default_generator
    gen = generator if generator is not None else default_generator
    potential = None
    if init == 'random':
        perm = gen.randperm(n)[:k]  # the generator's next draw
    else:
        rows = np.sort(gen.randperm(n)[:kmeanspp.sample_size(n, k, sample)])
        picked, potential = kmeanspp.seed(t[torch.from_numpy(rows).to(dev)], k, trials, generator=gen)
        perm = rows[picked]
    km = KMeans(None, d, k, generator=generator)
    km.to_lloyd(t[torch.from_numpy(perm).to(dev)].cpu().numpy(), spherical=spherical)
    km.to(dev)
    s = fixed_point_shift(rows_absmax(t), n)
    report, prev = FitReport(), None
    report.potential = potential
    for _it in range(int(iters)):
        labels, sums, counts = lloyd_update(km, t, s)
        changed = n if prev is None else int((labels != prev).sum())
        report.append((changed, finish_iteration(km, sums, counts, s, spherical=spherical)))
        prev = labels
        if changed == 0:
            break
    return km, prev, report
