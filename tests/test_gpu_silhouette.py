"""GPU: acav_rows_silhouette (acav100m_amd/csrc/acav_silhouette.hip) through clustering.silhouette against the float64 restatement
in difference form (tests/_silhouette_np.py) within the bounds derived there from include/acav_hip.h -- at the smallest shapes at
which each mechanism can fail -- and the same bytes from a second call, from any contiguous part of the query rows, from both
tile sizes and from host and device pointers."""
import ctypes as C

import numpy as np
import pytest

from tests import _silhouette_np as R

pytestmark = pytest.mark.gpu

LEN = 9  # ACAV_SILHOUETTE_PLAN_LEN


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


def _plan(gpu, m, d, k):
    lib, cus = gpu
    out = (C.c_int64 * LEN)()
    assert lib.acav_rows_silhouette_plan(m, d, k, cus, out) == 0
    return tuple(out)


@pytest.fixture(scope="module")
def cases(gpu):
    """the seeded inputs with the plan's column block, their restatements (computed once, left unchanged) and the kernel's figures"""
    from acav100m_amd.clustering import silhouette_samples
    block = _plan(gpu, 256, 32, 4)[1]
    out = {}
    for name, (x, lab, k) in R.cases(block).items():
        out[name] = (x, lab, k, R.Reference(x, lab, k), silhouette_samples(x, lab, k))
    return out


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_against_the_restatement(cases, name):
    x, lab, k, ref, (A, B, s) = cases[name]
    assert A.dtype == B.dtype == s.dtype == np.float64 and A.shape == B.shape == s.shape == (len(x),)
    ref.check(A, B, s, what=name)
    assert (s[ref.single] == 0).all() and (A[ref.single] == 0).all()


def test_shapes_are_the_ones_the_mechanisms_need(gpu, cases):
    tile, block, chunk = _plan(gpu, 600, 128, 2)[:3]
    assert (tile, block, chunk) == (64, 64, 32)
    x, lab, k = cases["tails_65x88_k33"][:3]
    assert len(x) == tile + 1 == block + 1 and x.shape[1] % chunk != 0
    assert cases["tails_65x87_k33"][0].shape[1] % 4 != 0
    x, lab, k = cases["two_599_1"][:3]
    assert np.bincount(lab).tolist() == [599, 1] and 599 > 2 * block and len(x) > 2 * tile
    x, lab, k = cases["absent_values"][:3]
    sizes = np.bincount(lab, minlength=k)
    assert (sizes == 0).sum() == 5 and (sizes == 1).sum() == 1
    ends = np.cumsum(np.bincount(cases["block_ends"][1]))
    assert ends.tolist() == [block, 2 * block + 1, 3 * block, 4 * block]
    assert cases["wide_1024"][0].shape == (257, 1024) and cases["wide_2304"][0].shape == (257, 2304)


def test_duplicate_rows_are_within_sqrt_delta_of_zero(gpu):
    """equal rows in different clusters and in the same cluster: the kernel's distance of such a pair is not 0 but at most
    sqrt(Delta_ij) -- seen through the row whose only neighbour in a cluster is its duplicate"""
    from acav100m_amd.clustering import silhouette_samples
    rs = np.random.RandomState(12)
    x = (3.0 + rs.randn(6, 64)).astype(np.float32)
    x[1] = x[0]  # the same cluster: A_0 = A_1 = dist(0, 1)
    x[3] = x[2]  # different clusters: B_2 = dist(2, 3) (cluster 2 is row 3 alone)
    lab = np.array([0, 0, 1, 2, 1, 3], np.int64)
    A, B, s = silhouette_samples(x, lab, 4)
    ref = R.Reference(x, lab, 4)
    ref.check(A, B, s, what="duplicates")
    nrm = (x.astype(np.float64) ** 2).sum(1)
    root = lambda i, j: np.sqrt(2 * R.gamma(64 + 2) * (nrm[i] + nrm[j])) * (1 + 2.0 ** -52)  # noqa: E731
    print("dist(0,1) = {!r} <= {!r}; dist(2,3) = {!r} <= {!r}".format(A[0], root(0, 1), B[2], root(2, 3)))
    assert ref.A[0] == 0 and 0 <= A[0] <= root(0, 1) and A[1] == A[0]
    assert ref.B[2] == 0 and 0 <= B[2] <= root(2, 3)
    x, lab, pairs = R.duplicates(8)
    A, B, s = silhouette_samples(x, lab, 3)
    R.Reference(x, lab, 3).check(A, B, s, what="duplicates 96 x 64")


def test_fewer_than_two_clusters_still_returns_a_and_b(gpu):
    from acav100m_amd.clustering import silhouette_samples, summarise
    x, _ = R.mixture([70], 24, 13)
    lab = np.full(70, 2, np.int64)
    A, B, s = silhouette_samples(x, lab, 5)
    ref = R.Reference(x, lab, 5)
    ref.check(A, B, what="one cluster")
    assert np.isinf(B).all() and (B > 0).all()
    rep = summarise(A, B, s, lab, 5)
    assert np.isnan(rep["silhouette_sampled"]) and "fewer than two" in rep["silhouette_undefined"]
    lab = np.arange(70, dtype=np.int64)  # every row alone: A = 0, s = 0, B the nearest other row
    A, B, s = silhouette_samples(x, lab, 70)
    R.Reference(x, lab, 70).check(A, B, s, what="all singletons")
    assert (A == 0).all() and (s == 0).all()
    assert "one row" in summarise(A, B, s, lab, 70)["silhouette_undefined"]


def test_the_same_call_gives_the_same_bytes(cases):
    from acav100m_amd.clustering import silhouette_samples
    for name in ("two_599_1", "tails_65x87_k33", "wide_1024"):
        x, lab, k, _ref, first = cases[name]
        again = silhouette_samples(x, lab, k)
        assert all(_same_bits(a, b) for a, b in zip(first, again)), name


def test_any_part_of_the_query_rows_gives_the_same_bytes(cases):
    """the query rows q0 <= i < q1 against the whole sample: other tiles, other workgroups, the same (A, B)"""
    from acav100m_amd.clustering import silhouette_samples
    for name, parts in (("two_599_1", [(0, 600), (0, 1), (599, 600), (17, 82), (64, 128), (301, 600)]),
                        ("tails_65x87_k33", [(0, 64), (64, 65), (3, 40)]), ("block_ends", [(0, 129), (129, 256), (100, 101)])):
        x, lab, k, _ref, (A, B, s) = cases[name]
        for q0, q1 in parts:
            a, b, t = silhouette_samples(x, lab, k, rows=(q0, q1))
            assert _same_bits(a, A[q0:q1]) and _same_bits(b, B[q0:q1]) and _same_bits(t, s[q0:q1]), (name, q0, q1)


def test_both_tile_sizes_give_the_same_bytes(gpu):
    """the smallest sample at which the plan for this device takes the 128-row query tile, against the restatement for a few query
    rows, and against the 64-row tile (a part of the query rows) to the bit"""
    from acav100m_amd.clustering import silhouette_samples
    lib, cus = gpu
    m, d, k = 128 * (cus - 1) + 1, 6, 24
    assert _plan(gpu, m, d, k)[0] == 128 and _plan(gpu, m - 1, d, k)[0] == 64
    x, lab = R.random_labels(m, d, k, 14)
    A, B, s = silhouette_samples(x, lab, k)
    rows = np.r_[0:40, m // 2:m // 2 + 40, m - 40:m]
    ref = R.Reference(x, lab, k, rows=rows)
    ref.check(A[rows], B[rows], s[rows], what="128-row tiles")
    q0, q1 = m // 2 - 100, m // 2 + 300
    a, b, t = silhouette_samples(x, lab, k, rows=(q0, q1))  # 400 query rows: the 64-row tile
    assert _same_bits(a, A[q0:q1]) and _same_bits(b, B[q0:q1])


def test_permuting_the_other_label_values_changes_no_a(cases):
    """the label values only order the runs: A is the same chain, B a minimum over the same sums"""
    from acav100m_amd.clustering import silhouette_samples
    x, lab, k, ref, (A, B, s) = cases["block_ends"]
    perm = np.array([2, 0, 3, 1])
    a, b, t = silhouette_samples(x, perm[lab], k)
    assert _same_bits(a, A) and _same_bits(b, B)


@pytest.mark.parametrize("bad", [-1, "K"])
def test_a_label_outside_the_range_is_refused(gpu, cases, bad):
    import torch
    lib, _ = gpu
    x, lab, k = cases["tails_65x88_k33"][:3]
    lab = lab.copy()
    lab[40] = k if bad == "K" else bad
    stats = np.full((len(x), 2), -3.0)
    rc = lib.acav_rows_silhouette(0, x.ctypes.data_as(C.c_void_p), len(x), x.shape[1], lab.ctypes.data_as(C.c_void_p), k,
                                  stats.ctypes.data_as(C.c_void_p), None)
    assert rc == -1 and b"1 of 65 labels are outside [0, 33)" in lib.acav_last_error()
    assert (stats == -3.0).all()
    on_dev = torch.full((len(x), 2), -3.0, dtype=torch.float64, device="cuda:0")
    rc = lib.acav_rows_silhouette(0, x.ctypes.data_as(C.c_void_p), len(x), x.shape[1], lab.ctypes.data_as(C.c_void_p), k,
                                  C.c_void_p(on_dev.data_ptr()), None)
    assert rc == -1 and bool((on_dev == -3.0).all())
    from acav100m_amd.clustering import silhouette_samples
    with pytest.raises(ValueError, match="outside"):
        silhouette_samples(x, lab, k)


def test_host_and_device_pointers_give_the_same_bytes(gpu, cases):
    import torch
    from acav100m_amd.clustering import silhouette_samples
    lib, _ = gpu
    for name in ("tails_65x87_k33", "two_599_1"):
        x, lab, k, _ref, (A, B, s) = cases[name]
        xt, lt = torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda()
        for xs, ls in ((xt, lt), (xt, lab), (x, lt), (torch.from_numpy(x), torch.from_numpy(lab))):
            a, b, t = silhouette_samples(xs, ls, k)
            assert _same_bits(a, A) and _same_bits(b, B) and _same_bits(t, s), name
        stats = torch.zeros((len(x), 2), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        assert lib.acav_rows_silhouette(0, C.c_void_p(xt.data_ptr()), len(x), x.shape[1], C.c_void_p(lt.data_ptr()), k,
                                        C.c_void_p(stats.data_ptr()), None) == 0
        got = stats.cpu().numpy()
        assert _same_bits(got[:, 0].copy(), A) and _same_bits(got[:, 1].copy(), B), name
        off = torch.zeros(len(x) * x.shape[1] + 1, dtype=torch.float32, device="cuda:0")[1:].view(len(x), x.shape[1])
        off.copy_(xt)  # rows off 16 bytes: the guarded loads feed the same values into the same chains
        a, b, t = silhouette_samples(off, lt, k)
        assert _same_bits(a, A) and _same_bits(b, B), name


def test_kmeans_silhouette_labels_the_rows_itself(gpu):
    import acav100m_amd
    from acav100m_amd.clustering import KMeans, silhouette_samples
    x, _ = R.mixture([90, 80, 70], 40, 15)
    acav100m_amd.manual_seed(3)
    km = KMeans(None, 40, 3)
    km.to_lloyd(x[:3]).to("cuda:0")
    labels, _ = km.calc_best(x, need_mean=False)
    got = km.silhouette(x)
    want = silhouette_samples(x, labels, 3)
    assert all(_same_bits(a, b) for a, b in zip(got, want))
    R.Reference(x, labels.numpy(), 3).check(*got, what="KMeans.silhouette")
