"""GPU: acav_rows_normalize (acav100m_amd/csrc/acav_rownorm.hip) through clustering.normalize against the numpy restatement
(tests/_rownorm_np.py), bit for bit: both sides of every internal switch (16-byte against guarded accesses, the register
instantiations for 1, 2, 4, 8 and 16 blocks, registers against LDS at 4096 / 4097 columns, more rows than one round of the
grid), zero rows, rows that are not finite, the extremes of fp32, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import _rownorm_np as R

pytestmark = pytest.mark.gpu

# the issue's shapes, then the neighbours of the register instantiations' limits (512 / 513, 1024 / 1025, 2048 / 2049 columns)
SHAPES = [(1, 1), (3, 3), (5, 63), (64, 64), (65, 65), (130, 255), (257, 256), (300, 257), (1000, 1000), (70, 1408), (33, 2304),
          (9, 4096), (5, 4097), (3, 16384),
          (6, 512), (6, 513), (5, 1024), (5, 1025), (5, 2048), (5, 2049)]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _rows(n, d, seed=0):
    rs = np.random.RandomState(seed + 31 * d + n)
    scale = np.exp(rs.uniform(np.log(1e-3), np.log(1e3), (n, 1)))
    return (rs.standard_normal((n, d)) * scale).astype(np.float32)


def _raw(x_dev, n, d):
    """the C entry point itself -> (rc, zero rows, bad rows)"""
    import acav100m_amd
    lib = acav100m_amd.load_library()
    zero, bad = C.c_int64(-7), C.c_int64(-7)
    rc = lib.acav_rows_normalize(0, C.c_void_p(x_dev), n, d, C.byref(zero), C.byref(bad), None)
    return rc, zero.value, bad.value


@pytest.mark.parametrize("n,d", SHAPES)
def test_bits_of_the_restatement(torch, n, d):
    from acav100m_amd.clustering import normalize, normalize_
    x = _rows(n, d)
    want, zero = R.normalize(x)
    t = torch.from_numpy(x).cuda()
    assert t.data_ptr() % 16 == 0
    back, got_zero = normalize_(t)
    assert back is t and got_zero == zero == 0
    got = t.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (n, d, int((got != want).sum()))
    n2 = (got.astype(np.float64) ** 2).sum(1)
    assert (np.abs(n2 - 1.0) <= 6e-7).all(), (n, d, float(np.abs(n2 - 1).max()))
    # the copying form, numpy in and out: the input stays what it is
    before = x.copy()
    y, z = normalize(x)
    assert z == 0 and y.tobytes() == want.tobytes() and x.tobytes() == before.tobytes()


@pytest.mark.parametrize("n,d", [(5, 64), (130, 256), (7, 1000), (4, 2304), (3, 4100), (2, 16384)])
def test_rows_off_16_bytes_take_the_guarded_path_to_the_same_bits(torch, n, d):
    from acav100m_amd.clustering import normalize_
    x = _rows(n, d, seed=5)
    want, _ = R.normalize(x)
    big = torch.zeros(n * d + 8, dtype=torch.float32, device="cuda")
    view = big[1:1 + n * d].view(n, d)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    view.copy_(torch.from_numpy(x))
    normalize_(view)
    assert view.cpu().numpy().tobytes() == want.tobytes()
    rest = big.cpu().numpy()
    assert rest[0] == 0 and (rest[1 + n * d:] == 0).all()  # nothing outside the rows is touched


def test_one_row_more_than_a_round_of_the_grid(torch):
    from acav100m_amd.clustering.normalize import normalize_, normalize_plan
    d = 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = normalize_plan(2 ** 30, d, cus)["round_rows"] + 1
    assert normalize_plan(n, d, cus)["round_rows"] == n - 1
    x = _rows(n, d, seed=9)
    want, _ = R.normalize(x)
    t = torch.from_numpy(x).cuda()
    normalize_(t)
    assert t.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("d", [65, 1024, 2304, 4097])
def test_a_row_does_not_depend_on_its_neighbours(torch, d):
    from acav100m_amd.clustering import normalize_
    x = _rows(100, d, seed=11)
    alone = torch.from_numpy(x).cuda()
    normalize_(alone)
    other = _rows(263, d, seed=12)
    both = torch.from_numpy(np.concatenate([other[:37], x, other[37:]])).cuda()
    normalize_(both)
    assert both[37:137].cpu().numpy().tobytes() == alone.cpu().numpy().tobytes()
    assert alone.cpu().numpy().tobytes() == R.normalize(x)[0].tobytes()


@pytest.mark.parametrize("d", [3, 256, 1408, 4100])
def test_zero_rows_are_left_alone_and_counted(torch, d):
    from acav100m_amd.clustering import normalize_
    n = 41
    x = _rows(n, d, seed=13)
    x[0] = 0
    x[n // 2] = 0
    x[n // 2, ::2] = -0.0
    x[n - 1] = -0.0
    want, zero = R.normalize(x)
    assert zero == 3
    t = torch.from_numpy(x).cuda()
    _, got_zero = normalize_(t)
    got = t.cpu().numpy()
    assert got_zero == 3 and got.tobytes() == want.tobytes()
    for i in (0, n // 2, n - 1):
        assert got[i].tobytes() == x[i].tobytes()


@pytest.mark.parametrize("d", [1, 300, 4100])
def test_the_extremes_of_fp32_come_out_finite_and_unit(torch, d):
    from acav100m_amd.clustering import normalize_
    x = np.stack([np.full(d, 3e38, np.float32), np.full(d, 1e-45, np.float32), np.full(d, -3e38, np.float32)])
    assert x[1, 0] > 0  # the smallest subnormal
    want, _ = R.normalize(x)
    t = torch.from_numpy(x).cuda()
    _, zero = normalize_(t)
    got = t.cpu().numpy()
    assert zero == 0 and np.isfinite(got).all() and got.tobytes() == want.tobytes()
    assert (np.abs((got.astype(np.float64) ** 2).sum(1) - 1.0) <= 6e-7).all()


@pytest.mark.parametrize("d", [5, 1024, 4100])
def test_rows_that_are_not_finite_are_counted_left_alone_and_raise(torch, d):
    from acav100m_amd.clustering import normalize_
    x = _rows(6, d, seed=17)
    x[1, d // 2] = np.inf
    x[4, 0] = np.nan
    x[5, d - 1] = -np.inf
    good = [0, 2, 3]
    want, _ = R.normalize(x[good])
    t = torch.from_numpy(x).cuda()
    rc, zero, bad = _raw(t.data_ptr(), 6, d)
    assert (rc, zero, bad) == (0, 0, 3)
    got = t.cpu().numpy()
    assert got[good].tobytes() == want.tobytes()
    for i in (1, 4, 5):
        assert got[i].tobytes() == x[i].tobytes()
    with pytest.raises(ValueError, match="not finite"):
        normalize_(torch.from_numpy(x).cuda())


def test_refusals_leave_the_table_untouched(torch):
    from acav100m_amd import _lib
    from acav100m_amd.clustering import normalize_
    x = _rows(4, 8, seed=19)
    t = torch.from_numpy(x).cuda()
    for d in (0, 16385, -1):
        assert _raw(t.data_ptr(), 4, d) == (-1, -7, -7)
    assert _raw(t.data_ptr(), -1, 8)[0] == -1 and _raw(t.data_ptr(), 2 ** 37, 8)[0] == -1
    host = x.copy()
    assert _raw(host.ctypes.data, 4, 8) == (-1, -7, -7)  # a host pointer
    assert host.tobytes() == x.tobytes() and t.cpu().numpy().tobytes() == x.tobytes()
    assert _raw(None, 0, 8) == (0, 0, 0)
    with pytest.raises(_lib.AcavError):
        normalize_(torch.from_numpy(x))
    with pytest.raises(ValueError):
        normalize_(t.double())
    with pytest.raises(ValueError):
        normalize_(t[:, ::2])
    empty = torch.empty((0, 8), dtype=torch.float32, device="cuda")
    assert normalize_(empty)[1] == 0
