"""A PCA front-end for the clustering stage: project every view onto its leading principal components before k-means --
sklearn.decomposition.PCA(n_components=dim).fit_transform, which the reference's correspondence_retrieval/code/clustering.py
(:62-78, pca.py: pca_features) runs on every whitened view.  No `whiten=True` scaling of the projected columns.

Definition, for rows x [N, d] fp32 and p components.  mean = the column means in float64; cov = sum (x - mean)(x - mean)^T /
(N - 1) in float64 on the stored fp32 values; numpy.linalg.eigh(cov) gives the p largest eigenvalues in descending order
(explained_variance, f64 [p]) and total_variance = trace(cov); the eigenvectors are the rows of `components`, each flipped so
that its entry of largest magnitude (the first one on a tie) is positive -- sklearn's svd_flip(u_based_decision=False); mean and
components are rounded to fp32; the projected row is y_ik = sum_j (x_ij (-) mean32_j) comp32_kj: one fp32 subtraction, the sum
in fp32 with j ascending.  N <= p is a ValueError.

The moments come from the GPU (acav_rows_scatter: float64 sum and scatter matrix of x - shift in device accumulators, a pure
function of the per-shard rows, the shard order and the shift) and are finished here: mean = shift + sum / N, S = scatter -
sum sum^T / N.  The shift -- the fp32-rounded column mean of the first rows seen -- removes the cancellation a raw sum x x^T -
N mu mu^T suffers on offset columns.  The projection is acav_rows_project.  There is no CPU path for either sweep."""
import numpy as np

from .. import _lib
from .sgd_clustering import _as_f32_2d, _device_index
from .whiten import ColumnMoments


class ScatterMoments:
    """Running (n, sum, scatter) of d columns around `shift` in float64, fed segment by segment; the two accumulators live on
    the device (a d x d float64 matrix is 42 MB at d = 2304: it crosses to the host once, in finish())."""

    def __init__(self, d, shift, device="cuda"):
        import torch
        self.d = int(d)
        self.shift = np.ascontiguousarray(shift, np.float32)
        if self.shift.shape != (self.d,):
            raise ValueError("shift has shape {}, the rows have {} columns".format(self.shift.shape, self.d))
        self.device = torch.device("cuda:{}".format(_device_index(device)))
        self.n = 0
        self.sum = torch.zeros(self.d, dtype=torch.float64, device=self.device)
        self.scatter = torch.zeros((self.d, self.d), dtype=torch.float64, device=self.device)

    def update(self, x, prefix=None):
        """one acav_rows_scatter call on x [n, d] (numpy, or a torch tensor on the host or the device); prefix: the row offsets
        of its segments ([0, ..., n], non-decreasing; None: one segment)."""
        import torch
        keep, xp, n, _ = _as_f32_2d(x, self.d)
        prefix = np.ascontiguousarray([0, n] if prefix is None else prefix, dtype=np.int64)
        nseg = len(prefix) - 1
        if prefix.ndim != 1 or nseg < 1:
            raise ValueError("prefix must hold the row offsets of at least one segment")
        torch.cuda.synchronize(self.device)  # whatever torch still has queued for x and the accumulators lands first
        lib = _lib.load_library()
        _lib.check(lib.acav_rows_scatter(self.device.index, xp, n, self.d, _lib.ptr(prefix), nseg, _lib.ptr(self.shift),
                                         _lib.ptr(self.sum), _lib.ptr(self.scatter), None))
        self.n += int(n)
        return self

    def finish(self):
        """-> (n, mean f64 [d], S f64 [d, d] = sum (x - mean)(x - mean)^T)"""
        s = self.sum.cpu().numpy()
        G = self.scatter.cpu().numpy()
        if self.n == 0:
            return 0, self.shift.astype(np.float64), G
        N = np.float64(self.n)
        return self.n, self.shift.astype(np.float64) + s / N, G - np.outer(s, s) / N


def components_from_scatter(n, mean, S, p, what="the rows"):
    """the Definition's host half (pure numpy): (n, mean f64, S f64, p) -> dict(mean fp32 [d], components fp32 [p, d],
    explained_variance f64 [p], total_variance f64)"""
    n, p = int(n), int(p)
    S = np.asarray(S, np.float64)
    d = S.shape[0]
    if not 1 <= p <= d:
        raise ValueError("{}: {} components of {} columns".format(what, p, d))
    if n <= p:
        raise ValueError("{}: {} rows cannot carry {} principal components (N <= p)".format(what, n, p))
    cov = S / np.float64(n - 1)
    w, v = np.linalg.eigh(cov)
    w, v = w[::-1][:p], v[:, ::-1][:, :p].T  # the p largest, descending; eigenvectors as rows
    top = np.argmax(np.abs(v), axis=1)       # svd_flip(u_based_decision=False): the first entry of largest magnitude
    v = v * np.sign(v[np.arange(p), top])[:, None]
    return {'mean': np.asarray(mean, np.float64).astype(np.float32), 'components': np.ascontiguousarray(v, np.float32),
            'explained_variance': np.ascontiguousarray(w, np.float64), 'total_variance': np.float64(np.trace(cov))}


def first_shift(x, device="cuda"):
    """the shift of a run that starts with rows x: their column means (one ColumnMoments.update), rounded to fp32"""
    cm = ColumnMoments(x.shape[1], device)
    cm.update(x)
    return cm.mean.astype(np.float32)


def project(x, mean, components, device="cuda"):
    """(x - mean) components^T -> a contiguous fp32 cuda tensor [n, p] (acav_rows_project); x [n, d]: numpy, or a torch tensor
    on the host or the device, left untouched."""
    import torch
    mean = np.ascontiguousarray(mean, np.float32)
    components = np.ascontiguousarray(components, np.float32)
    if components.ndim != 2 or mean.shape != (components.shape[1],):
        raise ValueError("mean {} and components {} do not belong together".format(mean.shape, components.shape))
    p, d = components.shape
    if hasattr(x, "is_cuda") and x.is_cuda:
        dev = x.device
    else:
        if not torch.cuda.is_available():
            raise _lib.AcavError("project multiplies on the GPU (there is no CPU path)")
        dev = torch.device("cuda:{}".format(_device_index(device)))
    keep, xp, n, _ = _as_f32_2d(x, d)
    y = torch.empty((n, p), dtype=torch.float32, device=dev)
    if n == 0 or p == 0:
        return y
    torch.cuda.synchronize(dev)
    lib = _lib.load_library()
    _lib.check(lib.acav_rows_project(dev.index, xp, n, d, _lib.ptr(mean), _lib.ptr(components), p, _lib.ptr(y), None))
    return y


class PCA:
    """sklearn.decomposition.PCA look-alike on the GPU: fit, transform, fit_transform; components_ fp32 [p, d], mean_ fp32 [d],
    explained_variance_ / explained_variance_ratio_ f64 [p].  numpy in gives numpy out, a torch tensor in gives a device tensor
    out.  n_components=None: every column."""

    def __init__(self, n_components=None, device="cuda"):
        self.n_components = n_components
        self.device = device

    def fit(self, x):
        import torch
        if not torch.cuda.is_available():
            raise _lib.AcavError("PCA takes its moments on the GPU (there is no CPU path)")
        if len(x.shape) != 2:
            raise ValueError("PCA needs [rows, d] features")
        n, d = int(x.shape[0]), int(x.shape[1])
        p = d if self.n_components is None else int(self.n_components)
        if not 1 <= p <= d:
            raise ValueError("n_components={} must be in [1, {}]".format(p, d))
        if n <= p:
            raise ValueError("{} rows cannot carry {} principal components (N <= p)".format(n, p))
        dev = x.device if hasattr(x, "is_cuda") and x.is_cuda else self.device
        if hasattr(x, "data_ptr") and not x.is_cuda:
            x = x.detach().to(torch.float32).contiguous().numpy()
        sm = ScatterMoments(d, first_shift(x, dev), dev)
        sm.update(x)
        fit = components_from_scatter(*sm.finish(), p)
        self.n_samples_ = n
        self.shift_ = sm.shift  # what the scatter matrix was taken around (the tests' error bound is stated in x - shift)
        self.mean_, self.components_ = fit['mean'], fit['components']
        self.explained_variance_ = fit['explained_variance']
        self.total_variance_ = fit['total_variance']
        tv = fit['total_variance']
        self.explained_variance_ratio_ = fit['explained_variance'] / tv if tv > 0 else np.zeros(p)
        return self

    def transform(self, x):
        is_torch = hasattr(x, "data_ptr")
        y = project(x, self.mean_, self.components_, x.device if is_torch and x.is_cuda else self.device)
        return y if is_torch else y.cpu().numpy()

    def fit_transform(self, x):
        return self.fit(x).transform(x)


def pca_feature(feature, dim=None, device="cuda"):
    """the reference's pca.py: pca_feature -- PCA(n_components=dim).fit_transform(feature)"""
    return PCA(dim, device).fit_transform(feature)


def pca_features(features, dim=None, device="cuda"):
    """the reference's pca.py: pca_features -- every view projected to `dim` columns (None: the smallest width over the views)"""
    if dim is None:
        dim = min(int(m.shape[1]) for m in features.values())
    return {k: pca_feature(v, dim, device) for k, v in features.items()}
