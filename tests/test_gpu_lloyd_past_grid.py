"""GPU: acav_rows_absmax and acav_lloyd_accumulate at sizes past one round of their capped grids and in their second arms, bit
for bit against numpy (np.abs(x).max()) and the restatement (tests/_lloyd_np.sums_counts).  Every kernel of acav_lloyd.hip caps
its grid at a few workgroups per compute unit and strides over the rest; the caps are restated here from the unit's constants
(LL_PER_CU = 8, LL_BIN_ROWS = 4096, LL_LDS_BINS = 8192, 256 threads) and every test sizes its input from the device's compute
unit count and asserts the inequality that makes the second round happen.  Integers throughout: nothing has a tolerance."""
import numpy as np
import pytest

from tests import _lloyd_np as L

pytestmark = pytest.mark.gpu

PER_CU = 8        # workgroups per compute unit of the absmax and sum grids
BIN_ROWS = 4096   # rows a binning workgroup takes at least
LDS_BINS = 8192   # k up to which a binning workgroup keeps its histogram in LDS


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cus(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- rows_absmax

ABSMAX_D = 7


@pytest.fixture(scope="module")
def table(torch, cus):
    """a table of a bit more than 4.5 x 256 x 8 x cus float4s at d = 7, on the host and on the device: every thread of the
    capped grid takes the unrolled loop once, half of them the one-load loop once, and total % 4 == 3 elements are left"""
    stride = 256 * PER_CU * cus              # threads of the capped grid = float4s of one round
    n = -(-(18 * stride + 64) // ABSMAX_D)   # 4.5 rounds of float4s = 18 rounds of floats, and a little
    while (n * ABSMAX_D) % 4 != 3:
        n += 1
    x = np.random.RandomState(7).standard_normal((n, ABSMAX_D)).astype(np.float32)
    total = n * ABSMAX_D
    quads = total // 4
    assert quads // 256 >= PER_CU * cus      # the grid is the capped one
    assert 4 * stride + stride // 2 < quads < 5 * stride  # one unrolled round for all; the one-load loop for the first threads
    assert total % 4 == 3
    return dict(x=x, xt=torch.from_numpy(x).cuda(), stride=stride, quads=quads, total=total, n=n)


def _restore(table, at, old):
    """the shared table is left as it was"""
    table["x"].reshape(-1)[at] = old
    table["xt"].view(-1)[at] = float(old)


def _places(table):
    """flat elements read by the unrolled loop at u = 0 .. 3 (by different threads of different workgroups), by the one-load
    loop, and the last total % 4 elements"""
    stride, quads, total = table["stride"], table["quads"], table["total"]
    places = {"u%d" % u: 4 * (u * stride + (37 + 1000 * u) % stride) + u for u in range(4)}
    places["u3 last thread"] = 4 * (3 * stride + stride - 1) + 3
    places["one-load first"] = 4 * (4 * stride)
    places["one-load last"] = 4 * (quads - 1) + 2
    places["tail first"] = 4 * quads
    places["tail last"] = total - 1
    return places


def test_absmax_past_the_grid_is_numpys(torch, cus, table):
    from acav100m_amd.clustering import rows_absmax
    x, xt = table["x"], table["xt"]
    assert xt.data_ptr() % 16 == 0  # the float4 arm
    assert rows_absmax(xt) == float(np.abs(x).max())
    assert rows_absmax(x) == float(np.abs(x).max())  # host rows
    flat, flat_t = x.reshape(-1), xt.view(-1)
    for name, at in _places(table).items():
        old = flat[at]
        try:
            flat[at] = flat_t[at] = -3e30  # the maximum, negative
            want = float(np.abs(x).max())
            assert want == float(np.float32(3e30))
            assert rows_absmax(xt) == want, name
        finally:
            _restore(table, at, old)
    assert rows_absmax(xt) == float(np.abs(x).max())


def test_absmax_of_rows_off_16_bytes_past_the_grid_is_numpys(torch, cus, table):
    from acav100m_amd.clustering import rows_absmax
    x, xt = table["x"], table["xt"]
    stride, total = table["stride"], table["total"]
    off = xt[1:]
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()  # the one-element-at-a-time arm
    assert total - ABSMAX_D > 256 * PER_CU * cus               # past its cap: the kernel strides
    assert rows_absmax(off) == float(np.abs(x[1:]).max())
    flat, flat_t = x.reshape(-1), xt.view(-1)
    # an element of the first round, of a middle round and the very last one (positions of the sliced table, + d in the whole)
    for name, at in (("first round", ABSMAX_D + 5), ("round 7", ABSMAX_D + 7 * stride + 12345), ("last", total - 1)):
        old = flat[at]
        try:
            flat[at] = flat_t[at] = -3e30
            assert rows_absmax(off) == float(np.abs(x[1:]).max()) == float(np.float32(3e30)), name
        finally:
            _restore(table, at, old)
    # the first row is not part of the slice: a maximum there is not seen
    old = flat[3]
    try:
        flat[3] = flat_t[3] = 3e30
        assert rows_absmax(off) == float(np.abs(x[1:]).max()) < 3e30
    finally:
        _restore(table, 3, old)


@pytest.mark.parametrize("bad,u", [(np.nan, 2), (np.inf, 1), (-np.inf, 3)])
def test_absmax_refuses_a_non_finite_value_in_the_unrolled_region(torch, cus, table, bad, u):
    from acav100m_amd.clustering import rows_absmax
    at = _places(table)["u%d" % u]
    assert at // 4 < 4 * table["stride"]
    old = table["x"].reshape(-1)[at]
    try:
        table["xt"].view(-1)[at] = float(bad)
        with pytest.raises(ValueError, match="not finite"):
            rows_absmax(table["xt"])
    finally:
        _restore(table, at, old)
    assert rows_absmax(table["xt"]) == float(np.abs(table["x"]).max())


# ---- accumulate

def _rows(seed, n, d):
    rs = np.random.RandomState(seed)
    return (rs.randn(n, d) * np.exp(rs.uniform(-3, 3, d))).astype(np.float32)


def _accumulate(torch, x, lab, k, s, pieces, tables="device", rows="device"):
    """the tables after accumulate over the row ranges pieces[i] .. pieces[i + 1], as numpy"""
    from acav100m_amd.clustering import accumulate
    d = x.shape[1]
    if tables == "device":
        S, Cn = torch.zeros((k, d), dtype=torch.int64, device="cuda"), torch.zeros(k, dtype=torch.int64, device="cuda")
    else:
        S, Cn = np.zeros((k, d), np.int64), np.zeros(k, np.int64)
    if rows == "device":
        x, lab = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
    for a, b in zip(pieces[:-1], pieces[1:]):
        accumulate(x[a:b], lab[a:b], s, S, Cn)
    return (S.cpu().numpy(), Cn.cpu().numpy()) if tables == "device" else (S, Cn)


def _same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_accumulate_with_a_second_round_of_sum_items(torch, cus):
    """k_lloyd_sum: a workgroup takes four (chunk, strip) items at a time and the grid is capped at 8 per compute unit; with more
    than 4 x grid items some waves take a second one"""
    from acav100m_amd.clustering.lloyd import accumulate_plan
    d = 130                                    # three strips, the last two columns wide
    n = k = 4 * PER_CU * cus // 3 + 270        # one-row lists: n chunks x 3 strips > 4 x 8 x cus items (3000 at 256 units)
    x = _rows(1, n, d)
    lab = np.random.RandomState(2).permutation(n).astype(np.int64)
    plan, _chunks = accumulate_plan(np.bincount(lab, minlength=k), d, cus)
    assert plan["strips"] == 3 and plan["items"] == 3 * n and plan["grid"] == PER_CU * cus
    assert plan["items"] > 4 * plan["grid"]
    s = L.shift_of(np.abs(x).max(), n)
    want = L.sums_counts(x, lab, k, s)
    _same(_accumulate(torch, x, lab, k, s, [0, n]), want)
    _same(_accumulate(torch, x, lab, k, s, [0, n], tables="host", rows="host"), want)


def test_accumulate_with_the_binning_grid_clamped(torch, cus):
    """k_lloyd_bin: the grid is capped at 4 workgroups per compute unit, beyond which a workgroup bins more than 4096 rows"""
    from acav100m_amd.clustering.lloyd import accumulate_plan
    n, d, k = BIN_ROWS * 4 * cus + 1, 1, 7
    rs = np.random.RandomState(3)
    x = _rows(4, n, d)
    lab = rs.randint(0, k - 1, n).astype(np.int64)
    lab[lab == 4] = k - 1  # cluster 4 is empty, the last one is not
    plan, _chunks = accumulate_plan(np.bincount(lab, minlength=k), d, cus)
    assert plan["bin_grid"] == 4 * cus and plan["bin_rows"] > BIN_ROWS and plan["lds_bins"] == 1
    s = L.shift_of(np.abs(x).max(), n)
    want = L.sums_counts(x, lab, k, s)
    assert want[1][4] == 0 and (np.delete(want[1], 4) > 0).all()
    _same(_accumulate(torch, x, lab, k, s, [0, n]), want)
    _same(_accumulate(torch, x, lab, k, s, [0, n // 3 + 5, n]), want)  # two uneven calls into the same tables
    _same(_accumulate(torch, x, lab, k, s, [0, n], tables="host", rows="host"), want)


@pytest.mark.parametrize("k", [LDS_BINS + 1, 20000])
def test_accumulate_with_more_clusters_than_lds_bins(torch, cus, k):
    """k > 8192: both binning kernels (histogram and inverted index) take one global atomic per row"""
    from acav100m_amd.clustering import accumulate
    from acav100m_amd.clustering.lloyd import accumulate_plan
    n, d = 40000, 3
    rs = np.random.RandomState(k)
    singles = k // 3
    lab = rs.randint(k // 2, k, n).astype(np.int64)       # the clusters singles + 1 .. k / 2 - 1 stay empty
    at = rs.permutation(n)
    lab[at[:singles]] = 1 + np.arange(singles)            # one row each, scattered over the rows
    lab[at[singles:singles + 700]] = 0                    # more than one chunk of 512 rows
    lab[at[singles + 700]] = k - 1
    x = _rows(k + 1, n, d)
    hist = np.bincount(lab, minlength=k)
    assert hist[0] == 700 and (hist[1:singles + 1] == 1).all() and (hist[singles + 1:k // 2] == 0).all() and hist[k - 1] >= 1
    plan, _chunks = accumulate_plan(hist, d, cus)
    assert plan["lds_bins"] == 0
    s = L.shift_of(np.abs(x).max(), n)
    want = L.sums_counts(x, lab, k, s)
    one = _accumulate(torch, x, lab, k, s, [0, n])
    _same(one, want)
    again = _accumulate(torch, x, lab, k, s, [0, n])  # a second identical call: the same bytes
    assert again[0].tobytes() == one[0].tobytes() and again[1].tobytes() == one[1].tobytes()
    _same(_accumulate(torch, x, lab, k, s, [0, n // 2 + 3, n], tables="host", rows="host"), want)
    xt = torch.from_numpy(x).cuda()
    S = torch.from_numpy(want[0]).cuda()
    Cn = torch.from_numpy(want[1]).cuda()
    for bad in (k, -1):
        wrong = lab.copy()
        wrong[n - 7] = bad
        with pytest.raises(ValueError, match="label"):
            accumulate(xt, wrong, s, S, Cn)
        assert np.array_equal(S.cpu().numpy(), want[0]) and np.array_equal(Cn.cpu().numpy(), want[1])  # nothing was added


@pytest.mark.parametrize("call_rows", [1000, 999])
@pytest.mark.parametrize("side", ["device", "host"])
def test_accumulate_splits_its_rows_into_calls(torch, monkeypatch, side, call_rows):
    """lloyd.accumulate cuts its rows into calls of CALL_ROWS rows by pointer arithmetic on the rows (4 d bytes per row) and the
    labels (8 bytes per row).  With d = 7 a piece of 999 rows starts off a 16-byte boundary (one of 1000 rows cannot: 4000 d
    is a multiple of 16), and so does every piece of rows that themselves start off one."""
    from acav100m_amd.clustering import lloyd
    n, d, k = 2500, 7, 11
    x = _rows(5, n + 1, d)
    lab = np.random.RandomState(6).randint(0, k, n + 1).astype(np.int64)
    s = L.shift_of(np.abs(x).max(), n + 1)
    monkeypatch.setattr(lloyd, "CALL_ROWS", call_rows)
    assert -(-n // lloyd.CALL_ROWS) == 3 and d % 4 != 0 and ((4 * d * call_rows) % 16 != 0) == (call_rows == 999)
    _same(_accumulate(torch, x[:n], lab[:n], k, s, [0, n], tables=side, rows=side), L.sums_counts(x[:n], lab[:n], k, s))
    # the rows 1 .. n of a table of n + 1: a base off 16 bytes (28 bytes into the table)
    _same(_accumulate(torch, x, lab, k, s, [1, n + 1], tables=side, rows=side), L.sums_counts(x[1:], lab[1:], k, s))
