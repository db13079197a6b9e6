"""Feature whitening for the clustering stage: divide every feature column by its standard deviation over all rows --
scipy.cluster.vq.whiten, which every clusterer of the reference's correspondence_retrieval/code/clustering.py runs first
(cat_and_whiten, :54-63).  No mean-centring: scipy's whiten does none.

Definition.  std_j = the population standard deviation (ddof = 0) of column j in float64 on the stored fp32 values, rounded to
fp32; std_j == 0 -> 1.0 (scipy's rule; counted in ColumnMoments.zero_columns); whitened x_ij = x_ij / std_j, one correctly
rounded fp32 division (numpy's x / std on fp32 arrays, bit for bit).

The moments come from the GPU (acav_colstats: per SEGMENT -- one shard's rows -- and column the float64 (mean, M2), a pure
function of the segment's rows) and are merged here, in segment order, with Chan's step in numpy float64: std is a function of
the per-shard rows and the shard order alone, not of the device, the row groups or how the rows reached the device.  There is
no CPU path for the sweeps."""
import ctypes as C

import numpy as np

from .. import _lib
from .sgd_clustering import _as_f32_2d, _device_index


class ColumnMoments:
    """Running (n, mean, M2) of d columns in float64, fed segment by segment."""

    def __init__(self, d, device="cuda"):
        self.d = int(d)
        self.device = device
        self.n = 0
        self.mean = np.zeros(self.d, np.float64)
        self.M2 = np.zeros(self.d, np.float64)

    @staticmethod
    def merge(a, b):
        """Chan's step, pure: (n_a, mean_a, M2_a), (n_b, mean_b, M2_b) -> (n, mean, M2) of the rows of a followed by those of b.
        An empty side leaves the other one as it is."""
        (na, ma, qa), (nb, mb, qb) = a, b
        na, nb = int(na), int(nb)
        ma, qa, mb, qb = (np.asarray(v, np.float64) for v in (ma, qa, mb, qb))
        if nb == 0:
            return na, ma.copy(), qa.copy()
        if na == 0:
            return nb, mb.copy(), qb.copy()
        n = na + nb
        delta = mb - ma
        f1 = np.float64(nb) / np.float64(n)
        f2 = np.float64(na) * np.float64(nb) / np.float64(n)
        return n, ma + delta * f1, (qa + qb) + (delta * delta) * f2

    def update(self, x, prefix=None):
        """one acav_colstats call on x [n, d] (numpy, or a torch tensor on the host or the device); prefix: the row offsets of
        its segments ([0, ..., n], non-decreasing; None: one segment).  The segments are merged in order."""
        keep, xp, n, _ = _as_f32_2d(x, self.d)
        prefix = np.ascontiguousarray([0, n] if prefix is None else prefix, dtype=np.int64)
        nseg = len(prefix) - 1
        if prefix.ndim != 1 or nseg < 1:
            raise ValueError("prefix must hold the row offsets of at least one segment")
        moments = np.empty((nseg, 2, self.d), np.float64)
        lib = _lib.load_library()
        _lib.check(lib.acav_colstats(_device_index(self.device), xp, n, self.d, _lib.ptr(prefix), nseg, _lib.ptr(moments), None))
        for s in range(nseg):
            self.add_segment(int(prefix[s + 1] - prefix[s]), moments[s, 0], moments[s, 1])
        return moments

    def add_segment(self, n, mean, M2):
        self.n, self.mean, self.M2 = self.merge((self.n, self.mean, self.M2), (n, mean, M2))

    def _raw_std(self):
        if self.n == 0:
            return np.zeros(self.d, np.float32)
        return np.sqrt(self.M2 / np.float64(self.n)).astype(np.float32)

    @property
    def zero_columns(self):
        """columns whose std is 0 (std() gives 1.0 for them)"""
        return int((self._raw_std() == 0).sum())

    def std(self):
        s = self._raw_std()
        s[s == 0] = np.float32(1.0)
        return s


def whiten_(x, std):
    """x [n, d] (a contiguous fp32 torch tensor on the GPU) <- x / std, in place (acav_rows_scale).  Returns x."""
    if not (hasattr(x, "is_cuda") and x.is_cuda):
        raise _lib.AcavError("whiten_ scales rows in place on the GPU: pass a cuda tensor (there is no CPU path)")
    import torch
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2:
        raise ValueError("whiten_ needs a contiguous [rows, d] float32 tensor")
    std = np.ascontiguousarray(std, np.float32)
    if std.shape != (x.shape[1],):
        raise ValueError("std has shape {}, the rows have {} columns".format(std.shape, x.shape[1]))
    if x.shape[1] == 0:
        return x
    torch.cuda.current_stream(x.device).synchronize()  # whatever torch still has queued for x lands first
    lib = _lib.load_library()
    _lib.check(lib.acav_rows_scale(x.device.index, C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], _lib.ptr(std), None))
    return x


def whiten(x, device="cuda"):
    """scipy.cluster.vq.whiten for fp32 rows -> (whitened copy, std).  x: numpy [n, d] (the copy is a numpy array) or a torch
    tensor (the copy is a tensor on `device`)."""
    import torch
    is_torch = hasattr(x, "data_ptr")
    dev = x.device if is_torch and x.is_cuda else torch.device("cuda:{}".format(_device_index(device)))
    t = (x.detach() if is_torch else torch.from_numpy(np.ascontiguousarray(x, np.float32))).to(dev, torch.float32, copy=True).contiguous()
    cm = ColumnMoments(t.shape[1], dev)
    cm.update(t)
    std = cm.std()
    whiten_(t, std)
    return (t if is_torch else t.cpu().numpy()), std
