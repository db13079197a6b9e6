"""GPU: acav_colstats / acav_rows_scale (acav100m_amd/csrc/acav_colstats.hip) through clustering.whiten against the float64
restatement (tests/_whiten_np.py): std within 1 fp32 ulp, the division bit for bit, the same bits from host and device input
and from every way of cutting the rows into segments and calls."""
import ctypes as C

import numpy as np
import pytest

from tests import _whiten_np as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    lib = acav100m_amd.load_library()
    cus = C.c_int(0)
    assert lib.acav_device_info(0, None, 0, C.byref(cus), None) == 0
    return lib, cus.value


def _past_the_grid(gpu):
    lib, cus = gpu
    out = (C.c_int64 * 6)()
    assert lib.acav_colstats_plan(2 ** 30, 64, -1, cus, out) == 0
    tile_rows, grid = int(out[0]), int(out[3])
    assert grid == 8 * cus
    return tile_rows * (grid + 1) + 1


def _moments(lib, x, prefix):
    """raw acav_colstats: x numpy (host pointer) or a cuda tensor -> float64 [nseg, 2, d]"""
    from acav100m_amd import _lib
    prefix = np.ascontiguousarray(prefix, np.int64)
    d = x.shape[1]
    out = np.full((len(prefix) - 1, 2, d), np.nan)
    if hasattr(x, "data_ptr"):
        import torch
        torch.cuda.synchronize()
    _lib.check(lib.acav_colstats(0, _lib.ptr(x), x.shape[0], d, _lib.ptr(prefix), len(prefix) - 1, _lib.ptr(out), None))
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# the smallest shapes at which each path can go wrong: every std 0; two rows; n on either side of a tile with d below one strip;
# d % 4 != 0 (the guarded path); nine strips; several tiles x several strips with tails in both
SHAPES = [(1, 5), (2, 3), (63, 88), (257, 88), (1000, 7), (300, 2304), (4099, 1408)]


def _check(gpu, x_host, x_dev):
    """assertions 1-3 on one matrix, given as a host array and as a device tensor holding the same values"""
    import torch
    from acav100m_amd.clustering.whiten import ColumnMoments, whiten_
    lib, _ = gpu
    n, d = x_host.shape
    want_std, want_zero = R.std_of(x_host)
    cm = ColumnMoments(d, "cuda:0")
    m_dev = cm.update(x_dev)
    std = cm.std()
    ulps = R.ulp_diff(std, want_std)
    print("n {} d {}: std max ulp {}, zero columns {}".format(n, d, int(ulps.max()), cm.zero_columns))
    assert std.dtype == np.float32 and int(ulps.max()) <= 1
    assert std[0] == 1.0 and cm.zero_columns == want_zero >= 1 and cm.n == n
    if n == 1:
        assert (std == 1.0).all() and cm.zero_columns == d
    # the division, with the GPU's own std
    y = x_dev.clone()
    assert whiten_(y, std) is y
    assert _same_bits(y.cpu().numpy(), x_host / std)
    assert _same_bits(x_dev.cpu().numpy(), x_host)  # (the clone was scaled, not the rows)
    # host pointer == device pointer == a second call
    assert _same_bits(_moments(lib, x_host, [0, n]), m_dev)
    assert _same_bits(_moments(lib, x_dev, [0, n]), m_dev)
    return std


@pytest.mark.parametrize("n,d", SHAPES, ids=["{}x{}".format(*s) for s in SHAPES])
def test_std_and_division(gpu, n, d):
    import torch
    x = R.recipe(n, d, seed=7 * n + d)
    _check(gpu, x, torch.from_numpy(x).cuda())


def test_unaligned_rows(gpu):
    """(1000, 8) at a 4-byte offset into a larger buffer: the device pointer is not 16-byte aligned, the staged copy of the host
    pointer is -- the guarded and the 16-byte path give the same bits"""
    import torch
    x = R.recipe(1000, 8, seed=11)
    buf = torch.zeros(1000 * 8 + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    x_dev = buf[1:].view(1000, 8)
    assert x_dev.data_ptr() % 16 == 4 and x_dev.is_contiguous()
    hbuf = np.zeros(1000 * 8 + 1, np.float32)
    hbuf[1:] = x.reshape(-1)
    std = _check(gpu, hbuf[1:].reshape(1000, 8), x_dev)
    from acav100m_amd.clustering.whiten import whiten_
    whiten_(x_dev, std)  # in place on the unaligned view: the float in front of it is left alone
    assert float(buf[0]) == 0.0 and _same_bits(buf[1:].cpu().numpy().reshape(1000, 8), x / std)


def test_past_the_grid(gpu):
    """d = 64, one tile more than the grid holds workgroups, and one row: the workgroups' second round"""
    import torch
    n = _past_the_grid(gpu)
    x = R.recipe(n, 64, seed=5)
    _check(gpu, x, torch.from_numpy(x).cuda())


@pytest.mark.parametrize("n,d", [(1000, 7), (4099, 1408)], ids=["1000x7", "4099x1408"])
def test_segments_do_not_see_each_other(gpu, n, d):
    """the per-segment moments of the same rows, bit for bit: one call with the prefix [0, 100, 100, 613, n], four calls on the
    four slices, and the same segments inside a larger call with other rows before and after"""
    import torch
    from acav100m_amd.clustering.whiten import ColumnMoments
    lib, _ = gpu
    x = R.recipe(n, d, seed=n + 13 * d)
    xt = torch.from_numpy(x).cuda()
    prefix = [0, 100, 100, 613, n]
    one = _moments(lib, xt, prefix)
    assert (one[1] == 0).all()  # the empty segment
    for s, (a, b) in enumerate(zip(prefix[:-1], prefix[1:])):
        assert _same_bits(_moments(lib, xt[a:b], [0, b - a])[0], one[s]), s
        assert _same_bits(_moments(lib, x[a:b], [0, b - a])[0], one[s]), s
        if b > a:  # against the restatement's tile / Chan form.  The summation orders differ: a mean moves by a few 2^-53 of the
            # column's largest value (1e-12 of it allows thousands), and M2 -- a sum of squares around means that are each
            # off by that much, e.g. 3e-11 against deviations of 0.5 in the -3e5 column -- by well under 1e-7 of itself
            _, mean, m2 = R.segment_moments(x[a:b])
            assert (np.abs(one[s, 0] - mean) <= 1e-12 * np.abs(x[a:b]).max(0)).all()
            assert (np.abs(one[s, 1] - m2) <= 1e-7 * m2).all()
    other = R.recipe(377, d, seed=99)
    big = torch.from_numpy(np.concatenate([other[:300], x, other[300:]])).cuda()
    inside = _moments(lib, big, [0] + [300 + p for p in prefix] + [300 + n + 77])
    assert _same_bits(inside[1:5], one)
    # the merged std of any segmentation of the same shard list: one update, or one per "row group"
    a, b, c = ColumnMoments(d, "cuda:0"), ColumnMoments(d, "cuda:0"), ColumnMoments(d, "cuda:0")
    a.update(xt, prefix)
    b.update(xt[:100], [0, 100])
    b.update(xt[100:], [0, 0, 513, n - 100])
    for lo, hi in zip(prefix[:-1], prefix[1:]):
        c.update(x[lo:hi])
    assert _same_bits(a.std(), b.std()) and _same_bits(a.std(), c.std())
    assert _same_bits(a.M2, b.M2) and _same_bits(a.mean, c.mean) and a.n == b.n == c.n == n
    assert int(R.ulp_diff(a.std(), R.std_of(x)[0]).max()) <= 1


def test_bad_divisors_leave_the_rows_alone(gpu):
    import torch
    from acav100m_amd.clustering.whiten import whiten_
    x = R.recipe(300, 12, seed=2)
    xt = torch.from_numpy(x).cuda()
    for bad in (0.0, float("nan"), -2.0, float("inf")):
        std = np.ones(12, np.float32)
        std[5] = bad
        with pytest.raises(ValueError, match="std"):
            whiten_(xt, std)
        assert _same_bits(xt.cpu().numpy(), x)
    with pytest.raises(ValueError):
        whiten_(xt, np.ones(11, np.float32))


def test_whiten_is_the_scipy_look_alike(gpu):
    import torch
    from acav100m_amd.clustering import whiten
    x = R.recipe(257, 88, seed=1)
    want, want_std, _ = R.whiten(x)
    keep = x.copy()
    y, std = whiten(x)
    assert isinstance(y, np.ndarray) and _same_bits(x, keep)
    assert int(R.ulp_diff(std, want_std).max()) <= 1 and _same_bits(y, x / std)
    xt = torch.from_numpy(x).cuda()
    yt, std_t = whiten(xt)
    assert yt.is_cuda and yt.data_ptr() != xt.data_ptr() and _same_bits(std_t, std)
    assert _same_bits(yt.cpu().numpy(), y) and _same_bits(xt.cpu().numpy(), x)
    if _same_bits(std, want_std):
        assert _same_bits(y, want)
