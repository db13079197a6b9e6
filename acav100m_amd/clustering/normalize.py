"""Row normalisation for the clustering stage: divide every feature row by its L2 norm, so that k-means clusters by direction
and not by magnitude -- faiss's normalize_L2, the step in front of its Kmeans(spherical=True), the clusterer the reference's
correspondence_retrieval/code/clustering.py runs by default.  clustering.normalize applies it to every view after the whitening
and the projection; clustering.spherical (clustering/lloyd.py) also renormalises the centres with it after every update.

Definition (acav_rows_normalize, include/acav_hip.h; tests/_rownorm_np.py restates it in numpy bit for bit).  Per row, ss = the
float64 sum of the exact squares in one stated order (256 chains over the columns j = q mod 256 in ascending order, folded four
at a time, then six butterfly steps), norm = sqrt(ss), x_j <- float32(float64(x_j) / norm).  A row of zeros is left as it is and
counted; a row with an inf or NaN entry is left as it is and raises ValueError.  A row's result depends on that row alone.
There is no CPU path."""
import ctypes as C

import numpy as np

from .. import _lib
from .sgd_clustering import _device_index


def normalize_(x):
    """x [n, d] (a contiguous fp32 torch tensor on the GPU) <- its rows divided by their L2 norms, in place (acav_rows_normalize)
    -> (x, zero_rows): the rows that are all zeros stay as they are and are counted.  A row that is not finite: ValueError."""
    if not (hasattr(x, "is_cuda") and x.is_cuda):
        raise _lib.AcavError("normalize_ scales rows in place on the GPU: pass a cuda tensor (there is no CPU path)")
    import torch
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2:
        raise ValueError("normalize_ needs a contiguous [rows, d] float32 tensor")
    if x.shape[0] == 0 or x.shape[1] == 0:
        return x, 0
    torch.cuda.current_stream(x.device).synchronize()  # whatever torch still has queued for x lands first
    zero, bad = C.c_int64(0), C.c_int64(0)
    lib = _lib.load_library()
    _lib.check(lib.acav_rows_normalize(x.device.index, C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], C.byref(zero), C.byref(bad), None))
    if bad.value:
        raise ValueError("{} of {} rows hold a value that is not finite (inf, NaN): they have no direction; those rows were left "
                         "as they are, the others are normalised".format(bad.value, x.shape[0]))
    return x, int(zero.value)


def normalize(x, device="cuda"):
    """-> (copy of x with unit rows, zero_rows).  x: numpy [n, d] (the copy is a numpy array) or a torch tensor (the copy is a
    tensor on `device`)."""
    import torch
    is_torch = hasattr(x, "data_ptr")
    dev = x.device if is_torch and x.is_cuda else torch.device("cuda:{}".format(_device_index(device)))
    t = (x.detach() if is_torch else torch.from_numpy(np.ascontiguousarray(x, np.float32))).to(dev, torch.float32, copy=True).contiguous()
    _, zero = normalize_(t)
    return (t if is_torch else t.cpu().numpy()), zero


def normalize_plan(n, d, cus=256):
    """the launch shape acav_rows_normalize gives n rows of width d -> dict; pure: no device"""
    out = (C.c_int64 * 6)()
    _lib.check(_lib.load_library().acav_rows_normalize_plan(int(n), int(d), int(cus), out))
    keys = ('wg_rows', 'blocks', 'lds', 'grid', 'lds_bytes', 'round_rows')
    return dict(zip(keys, (int(v) for v in out)))
