"""GPU: acav_lloyd_centers, the centre update of Lloyd k-means on the device, against the numpy restatement
(tests/_lloyd_np.centers_of before its empty-cluster rule) bit for bit -- three correctly rounded operations that numpy performs
identically, so nothing here has a tolerance -- and lloyd.finish_iteration with device tables against the same call with the
tables copied to numpy (the host path), without and with empty clusters.  Also past the kernel's capped grid (sized from the
device's compute unit count), at rows shorter than a quad, and with tables that start off a 16-byte boundary."""
import ctypes as C

import numpy as np
import pytest

from tests import _lloyd_np as L

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (64, 64), (257, 65), (33, 1027)]  # tails in k and d, a pitch off 16 bytes, more than one workgroup
# rows shorter than a quad: a quad of the flat table spans 4, 2 and 2 rows and steps to the next row's count up to three times,
# empties among them; k d leaves 3, 2 and 2 tail elements and fills more than one workgroup
SHAPES += [(1031, 1), (1031, 2), (1030, 3)]
SHIFTS = [-103, 0, 40, 209]                                  # the ends of fixed_point_shift for fp32 input, and two inside
COUNTS = [0, 1, 3, 2 ** 31, 2 ** 37]
SPECIAL = [0, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53 + 3, -(2 ** 53 + 3), 2 ** 62 - 1, -(2 ** 62 - 1), 1, -1, 3, -3]
TINY = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _before_the_split(sums, counts, s, monkeypatch):
    """centers_of with its empty-cluster rule switched off: an empty cluster keeps its row of zeros"""
    monkeypatch.setattr(L, "split_empty", lambda centers, counts: 0)
    with np.errstate(over="ignore", under="ignore"):
        return L.centers_of(sums, counts, s)[0]


def _tables(k, d, s, turn, monkeypatch):
    """sums of both signs with exact zeros and the special values, counts cycling through COUNTS; every sum whose quotient
    would be a subnormal, an infinity or a NaN in fp32 is replaced by 0 -- decided by the restatement, not by the kernel"""
    rs = np.random.RandomState(1000 * k + d + turn)
    sums = rs.randint(-2 ** 40, 2 ** 40, size=(k, d)).astype(np.int64)
    flat = sums.reshape(-1)
    at = rs.permutation(flat.size)[:max(1, flat.size // 2)]
    flat[at] = np.array(SPECIAL, np.int64)[(np.arange(len(at)) + turn) % len(SPECIAL)]
    counts = np.array(COUNTS, np.int64)[(np.arange(k) + turn) % len(COUNTS)]
    want = _before_the_split(sums, counts, s, monkeypatch)
    bad = ~np.isfinite(want) | ((want != 0) & (np.abs(want) < TINY))
    sums[bad] = 0
    want = _before_the_split(sums, counts, s, monkeypatch)
    assert np.isfinite(want).all() and ((want == 0) | (np.abs(want) >= TINY)).all()
    return sums, counts, want


@pytest.mark.parametrize("k,d", SHAPES)
def test_centres_sizes_and_empties_are_the_restatements(torch_gpu, monkeypatch, k, d):
    torch = torch_gpu
    from acav100m_amd.clustering.lloyd import centers_on_device
    kept = 0
    for turn, s in enumerate(SHIFTS):
        sums, counts, want = _tables(k, d, s, turn, monkeypatch)
        centers, sizes, empty = centers_on_device(torch.from_numpy(sums).cuda(), torch.from_numpy(counts).cuda(), s)
        got = centers.cpu().numpy()
        print((k, d), "s", s, "nonzero", int((want != 0).sum()), "of", want.size, "empty", empty,
              "mismatches", int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert got.tobytes() == want.tobytes(), (k, d, s)
        assert np.array_equal(sizes.cpu().numpy(), counts.astype(np.float32)), (k, d, s)
        assert empty == int((counts == 0).sum()), (k, d, s)
        big = np.abs(sums) > 2 ** 53
        kept += int((big & (counts[:, None] > 0)).sum())
    assert kept > 0 or k * d < 8  # the ties above 2^53 are really among the quotients that are compared


def test_a_table_past_the_capped_grid(torch_gpu, monkeypatch):
    """k_lloyd_centers caps its grid at 8 workgroups of 256 threads per compute unit, a quad of elements per thread: a table of
    more than 4 x 256 x 8 x cus elements is walked in a second round"""
    torch = torch_gpu
    from acav100m_amd.clustering.lloyd import centers_on_device
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    d = 1024
    k = 4 * 256 * 8 * cus // d + len(COUNTS)  # 2053 at 256 units: the last five rows are the second round's
    assert (k - len(COUNTS)) * d >= 4 * 256 * 8 * cus and k * d // 4 // 256 >= 8 * cus
    for turn, s in ((1, 0), (2, 40)):
        sums, counts, want = _tables(k, d, s, turn, monkeypatch)
        assert (counts[-len(COUNTS):] == 0).sum() == 1  # an empty row among the second round's
        centers, sizes, empty = centers_on_device(torch.from_numpy(sums).cuda(), torch.from_numpy(counts).cuda(), s)
        got = centers.cpu().numpy()
        print((k, d), "s", s, "empty", empty, "mismatches", int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert got.tobytes() == want.tobytes(), (k, d, s)
        assert np.array_equal(sizes.cpu().numpy(), counts.astype(np.float32)), (k, d, s)
        assert empty == int((counts == 0).sum()), (k, d, s)


@pytest.mark.parametrize("k,d", [(257, 65), (33, 1027), (1031, 1)])
def test_tables_that_start_off_16_bytes(torch_gpu, monkeypatch, k, d):
    """sums, or centers, off a 16-byte boundary: every element goes one by one (vec == 0) -- the bytes of the aligned call"""
    torch = torch_gpu
    from acav100m_amd import _lib
    from acav100m_amd.clustering.lloyd import centers_on_device
    assert d % 2 == 1
    s = 40
    sums, counts, _want = _tables(k + 1, d, s, 3, monkeypatch)
    want = _before_the_split(sums[1:], counts[1:], s, monkeypatch)
    whole_s, whole_c = torch.from_numpy(sums).cuda(), torch.from_numpy(counts).cuda()
    aligned = centers_on_device(whole_s[1:].clone(), whole_c[1:].clone(), s)
    assert aligned[0].cpu().numpy().tobytes() == want.tobytes()
    # sums off 16 bytes (8 d bytes into the table, d odd); the slice is contiguous
    off_s = whole_s[1:]
    assert off_s.data_ptr() % 16 == 8 and off_s.is_contiguous()
    got = centers_on_device(off_s, whole_c[1:], s)
    assert got[0].cpu().numpy().tobytes() == aligned[0].cpu().numpy().tobytes()
    assert torch.equal(got[1], aligned[1]) and got[2] == aligned[2] == int((counts[1:] == 0).sum())
    # centers off 16 bytes (4 d bytes into a buffer): the entry point itself, centers_on_device allocates its own buffer
    sums_a, counts_a = whole_s[1:].clone(), whole_c[1:].clone()
    buf = torch.full((k + 1, d), 7.0, dtype=torch.float32, device="cuda")
    centers, sizes = buf[1:], torch.empty(k, dtype=torch.float32, device="cuda")
    assert sums_a.data_ptr() % 16 == 0 and centers.data_ptr() % 16 != 0 and centers.is_contiguous()
    torch.cuda.synchronize()
    empty = C.c_int64(-5)
    _lib.check(_lib.load_library().acav_lloyd_centers(0, _lib.ptr(sums_a), _lib.ptr(counts_a), k, d, s, _lib.ptr(centers), _lib.ptr(sizes),
                                                      C.byref(empty), None))
    assert centers.cpu().numpy().tobytes() == aligned[0].cpu().numpy().tobytes()
    assert torch.equal(sizes, aligned[1]) and empty.value == aligned[2]
    assert bool((buf[0] == 7.0).all())  # the row in front of the table is left alone


def test_ties_above_2_53_go_to_even(torch_gpu):
    """(2^53 + 1) and (2^53 + 3) are ties of the int64 -> double conversion: to 2^53 and to 2^53 + 4"""
    torch = torch_gpu
    from acav100m_amd.clustering.lloyd import centers_on_device
    sums = np.array([[2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53 + 1), -(2 ** 53 + 3), 2 ** 62 - 1, -(2 ** 62 - 1)]], np.int64)
    for count in (1, 3, 2 ** 31, 2 ** 37):
        counts = np.array([count], np.int64)
        want = np.float32(sums.astype(np.float64) * 2.0 ** -0 / counts[:, None].astype(np.float64))
        centers, sizes, empty = centers_on_device(torch.from_numpy(sums).cuda(), torch.from_numpy(counts).cuda(), 0)
        assert centers.cpu().numpy().tobytes() == want.tobytes() and empty == 0 and float(sizes[0]) == float(count)


def _state(km):
    centers, counts, count, fallback = km.state_arrays()
    return centers.tobytes(), counts.tobytes(), count, fallback


@pytest.mark.parametrize("empties", [0, 2])
def test_finish_iteration_on_device_tables_is_the_host_path(torch_gpu, empties):
    torch = torch_gpu
    from acav100m_amd.clustering import KMeans
    from acav100m_amd.clustering.lloyd import finish_iteration
    k, d, n = 37, 65, 4000
    rs = np.random.RandomState(3 + empties)
    x = rs.randn(n, d).astype(np.float32)
    used = np.array([c for c in range(k) if not (empties and c in (5, k - 1))])  # with empties: clusters 5 and k - 1 get no row
    labels = used[rs.randint(0, len(used), n)]
    s = L.shift_of(np.abs(x).max(), n)
    sums, counts = L.sums_counts(x, labels, k, s)
    assert int((counts == 0).sum()) == empties
    start = rs.randn(k, d).astype(np.float32)
    got, ref = (KMeans(None, d, k).to_lloyd(start).to("cuda:0") for _ in range(2))
    for km in (got, ref):
        km.count = 123
    splits_dev = finish_iteration(got, torch.from_numpy(sums).cuda(), torch.from_numpy(counts).cuda(), s)
    splits_host = finish_iteration(ref, sums.copy(), counts.copy(), s)
    want_centers, want_sizes, want_splits = L.centers_of(sums, counts, s)
    assert splits_dev == splits_host == want_splits == empties
    assert _state(got) == _state(ref)
    assert _state(got) == (want_centers.tobytes(), want_sizes.astype(np.float32).tobytes(), 123 + n, 0)


def test_argument_errors_leave_the_outputs_untouched(torch_gpu):
    torch = torch_gpu
    from acav100m_amd import _lib
    lib = _lib.load_library()
    k, d = 4, 6
    sums = torch.ones((k, d), dtype=torch.int64, device="cuda")
    counts = torch.ones(k, dtype=torch.int64, device="cuda")
    centers = torch.full((k, d), 7.0, device="cuda")
    sizes = torch.full((k,), 7.0, device="cuda")
    host = np.ones((k, d), np.int64)
    host_f = np.ones((k, d), np.float32)
    p = _lib.ptr
    torch.cuda.synchronize()
    cases = {
        "NULL sums": (None, p(counts), k, d, 0, p(centers), p(sizes)),
        "NULL counts": (p(sums), None, k, d, 0, p(centers), p(sizes)),
        "NULL centers": (p(sums), p(counts), k, d, 0, None, p(sizes)),
        "NULL sizes": (p(sums), p(counts), k, d, 0, p(centers), None),
        "host sums": (p(host), p(counts), k, d, 0, p(centers), p(sizes)),
        "host centers": (p(sums), p(counts), k, d, 0, p(host_f), p(sizes)),
        "k = 0": (p(sums), p(counts), 0, d, 0, p(centers), p(sizes)),
        "d = 0": (p(sums), p(counts), k, 0, 0, p(centers), p(sizes)),
        "d = 16385": (p(sums), p(counts), k, 16385, 0, p(centers), p(sizes)),
        "k d > 2^30": (p(sums), p(counts), 65537, 16384, 0, p(centers), p(sizes)),
        "s = 1001": (p(sums), p(counts), k, d, 1001, p(centers), p(sizes)),
        "s = -1001": (p(sums), p(counts), k, d, -1001, p(centers), p(sizes)),
    }
    for name, (a, b, kk, dd, s, c, z) in cases.items():
        empty = C.c_int64(-5)
        assert lib.acav_lloyd_centers(0, a, b, kk, dd, s, c, z, C.byref(empty), None) == -1, name  # ACAV_EINVAL
        assert empty.value == -5, name
        assert bool((centers == 7.0).all()) and bool((sizes == 7.0).all()) and (host_f == 1).all(), name
    empty = C.c_int64(-5)
    assert lib.acav_lloyd_centers(0, p(sums), p(counts), k, d, 0, p(centers), None, None, None) == -1  # NULL empty_host
    _lib.check(lib.acav_lloyd_centers(0, p(sums), p(counts), k, d, 0, p(centers), p(sizes), C.byref(empty), None))
    assert empty.value == 0 and bool((centers == 1.0).all()) and bool((sizes == 1.0).all())
