"""The exact silhouette of a labelled sample: sklearn.metrics.silhouette_samples / silhouette_score(sample_size=, random_state=)
for the clustering stage (`evaluate --evaluate.silhouette_sample=M`, KMeans.silhouette).  No counterpart in the reference.

inertia and nearest_inertia live in the space a view was trained in, and the centroid silhouette and Davies-Bouldin are functions
of the trained centres; this index is neither: it needs the rows and their labels alone, and it has no scale.  That makes it the
figure to compare runs that differ in clustering.whiten, clustering.pca_dim, clustering.algorithm, clustering.init or
ncentroids.

Definition on rows x [M, d] (fp32, after the view's front-end) with labels l [M] in [0, K), n_k rows labelled k:
  dist(i, j) = ||x_i - x_j|| in float64 (acav_rows_silhouette: as sqrt(max(0, ||x_i||^2 + ||x_j||^2 - 2 x_i.x_j)) on the f64
               matrix core, include/acav_hip.h states the error bound and the summation order)
  A_i = sum_{j != i, l_j = l_i} dist(i, j) / (n_{l_i} - 1)
  B_i = min over k != l_i with n_k > 0 of sum_{l_j = k} dist(i, j) / n_k
  s_i = (B_i - A_i) / max(A_i, B_i); 0 when n_{l_i} = 1, and 0 when both are 0
With fewer than two non-empty clusters, or n_k = 1 for every k, sklearn raises; here A and B are still returned (B = +inf, A = 0
where undefined) and summarise reports nan with the reason.  Every pairwise distance is a GPU sweep (there is no CPU path);
tests/_silhouette_np.py restates the definition in numpy."""
import numpy as np

from .. import _lib
from .sgd_clustering import _as_f32_2d, _device_index


def sample_indices(n, size, seed):
    """the rows sklearn's silhouette_score(..., sample_size=size, random_state=seed) draws from n, in ascending order; every row
    when size >= n"""
    n, size = int(n), int(size)
    return np.sort(np.random.RandomState(seed).permutation(n)[:min(n, size)])


def _labels(labels, n):
    if hasattr(labels, "data_ptr"):
        import torch
        lab = labels.detach().to(torch.long).contiguous()
        if lab.is_cuda:
            torch.cuda.current_stream(lab.device).synchronize()
    else:
        lab = np.ascontiguousarray(labels, np.int64)
    if tuple(lab.shape) != (n,):
        raise ValueError("expected {} labels, got shape {}".format(n, tuple(lab.shape)))
    return lab


def _scores(A, B, own_size):
    """s from (A, B) and n_{l_i} per row: (B - A) / max(A, B), 0 for the only row of its cluster and where both are 0"""
    top = np.maximum(A, B)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = np.where(np.isinf(B), 1.0, (B - A) / top)  # (B = +inf: no other cluster; summarise reports that case as nan)
    s[(own_size == 1) | (top == 0)] = 0.0
    return s


def silhouette_samples(x, labels, k=None, device="cuda", rows=None):
    """(A, B, s), float64 [M] each, of x [M, d] with labels [M] in [0, k) (k=None: max label + 1): acav_rows_silhouette.  x and
    labels: numpy or torch, host or device.  rows=(q0, q1): only those query rows, against the whole sample -- the same bytes as
    the full call's rows q0:q1."""
    keep, xp, m, on_gpu = _as_f32_2d(x)
    d = int(keep.shape[1])
    lab = _labels(labels, m)
    host_lab = lab.cpu().numpy() if hasattr(lab, "cpu") else lab
    if k is None:
        k = int(host_lab.max()) + 1 if m else 1
    q0, q1 = (0, m) if rows is None else (int(rows[0]), int(rows[1]))
    stats = np.empty((max(0, q1 - q0), 2), np.float64)
    lib = _lib.load_library()
    dev = keep.device.index if on_gpu else _device_index(device)
    if rows is None:
        _lib.check(lib.acav_rows_silhouette(dev, xp, m, d, _lib.ptr(lab), int(k), _lib.ptr(stats), None))
    else:
        _lib.check(lib.acav_rows_silhouette_range(dev, xp, m, d, _lib.ptr(lab), int(k), q0, q1, _lib.ptr(stats), None))
    A, B = stats[:, 0].copy(), stats[:, 1].copy()
    s = _scores(A, B, np.bincount(host_lab, minlength=int(k))[host_lab[q0:q1]])
    return A, B, s


def undefined_reason(labels, k):
    """why sklearn would refuse these labels (a string), or None"""
    sizes = np.bincount(np.asarray(labels, np.int64), minlength=int(k))
    if int((sizes > 0).sum()) < 2:
        return "fewer than two non-empty clusters in the sample"
    if int(sizes.max()) <= 1:
        return "every cluster has one row in the sample"
    return None


def summarise(A, B, s, labels, k):
    """the report keys of one view and epoch (pure numpy): silhouette_sampled = mean s, silhouette_sample = M,
    silhouette_negative_share = share of rows with s < 0, silhouette_by_cluster = K means (nan for a cluster absent from the
    sample), and -- only when the index is undefined -- silhouette_undefined = the reason, with nan for the figures"""
    s, lab, k = np.asarray(s, np.float64), np.asarray(labels, np.int64), int(k)
    m = int(s.shape[0])
    nan = float('nan')
    reason = undefined_reason(lab, k)
    if reason is not None:
        return {'silhouette_sampled': nan, 'silhouette_sample': m, 'silhouette_negative_share': nan,
                'silhouette_by_cluster': [nan] * k, 'silhouette_undefined': reason}
    sizes = np.bincount(lab, minlength=k)
    sums = np.bincount(lab, weights=s, minlength=k)
    by = [float(sums[c] / sizes[c]) if sizes[c] else nan for c in range(k)]
    return {'silhouette_sampled': float(s.mean()), 'silhouette_sample': m, 'silhouette_negative_share': float((s < 0).mean()),
            'silhouette_by_cluster': by}


def check_options(opts):
    """(evaluate.silhouette_sample, evaluate.silhouette_seed) of the `evaluate` options -> (M or None, seed).  Pure: no device,
    no file"""
    m, seed = opts.get('silhouette_sample'), opts.get('silhouette_seed')
    seed = 0 if seed is None else seed
    if m is None:
        return None, seed
    if isinstance(m, bool) or not isinstance(m, int) or m < 2:
        raise ValueError("evaluate.silhouette_sample must be an integer of at least 2 (rows of the sample), not {!r}".format(m))
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
        raise ValueError("evaluate.silhouette_seed must be an integer in [0, 2^32), not {!r}".format(seed))
    return m, seed
