"""GPU: KMeans.quality / acav_kmeans_quality (acav100m_amd/csrc/acav_kmeans_quality.hip) against the float64 restatement of
tests/_kmeans_quality_np.py within its derived bounds, its determinism and split invariance, its refusals, and that it leaves
the handle alone.  The labels are calc_best's (pinned to the oracle in tests/test_gpu_kmeans.py); the states have under-used
clusters, so the discount moves rows away from their nearest centre.  The `large` tests run the same checks at the smallest
sizes at which every workgroup of k_quality takes several row tiles (R.large_shapes, from the device's CU count)."""
import ctypes as C

import numpy as np
import pytest

from tests import _kmeans_quality_np as R

pytestmark = pytest.mark.gpu

CASES = [("discount",) + s for s in R.SHAPES] + [("warm", 1000, 128, 64), ("scaled", 65, 88, 33), ("special", 1000, 128, 64)]
_IDS = ["{}-{}x{}x{}".format(*c) for c in CASES]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


_cache = {}


def _case(kind, n, d, K):
    """(km, x on the device, labels of calc_best, cluster_stats, row_stats, Reference) -- built once and shared, never changed"""
    key = (kind, n, d, K)
    if key not in _cache:
        import torch
        from acav100m_amd.clustering import KMeans
        x, c, counts, count = R.make_case(n, d, K, kind=kind)
        km = KMeans(None, d, K).to("cuda:0")
        km.load_state_arrays(c, counts, count, 0)
        xt = torch.from_numpy(x).cuda()
        labels, _ = km.calc_best(xt, need_mean=False)
        cs, rows = km.quality(xt, labels, rows=True)
        _cache[key] = (km, xt, labels, cs, rows, R.Reference(x, c, labels.cpu().numpy()))
    return _cache[key]


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan(n, K, cus):
    """acav_kmeans_quality_plan -> (ntiles, grid, lds_bytes, per_cu)"""
    from acav100m_amd import _lib
    out = (C.c_int64 * 4)()
    _lib.check(_lib.load_library().acav_kmeans_quality_plan(n, K, cus, out))
    return tuple(out)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_rows_and_clusters_within_the_derived_bounds(env, case):
    _check_rows_and_clusters(case)


LARGE_IDS = ["small_k", "two_centre_passes", "largest_k"]  # the rows of R.large_shapes


@pytest.mark.parametrize("which", range(3), ids=LARGE_IDS)
def test_large_rows_and_clusters_within_the_derived_bounds(env, which):
    """every workgroup takes at least two tiles (sums carried over, labs and rv reused, the last tile of one row is not its
    workgroup's first); then the checks of test_rows_and_clusters_within_the_derived_bounds, the same bounds"""
    cus = _cus()
    n, d, K = R.large_shapes(cus)[which]
    ntiles, grid, _, per_cu = _plan(n, K, cus)
    assert ntiles >= 2 * grid and grid == cus * per_cu and n % 64 == 1, (n, K, cus, ntiles, grid)
    assert per_cu == (1 if K == 2048 else 4)
    _check_rows_and_clusters(("discount", n, d, K))


@pytest.mark.parametrize("which", range(3), ids=LARGE_IDS)
def test_large_whole_call_equals_one_tile_per_workgroup_pieces(env, which):
    """the whole call (several tiles per workgroup) against the same rows in pieces of at most grid * 64 rows, each of which
    runs one tile per workgroup -- the path the small cases pin: the same row_stats bytes, equal counts, float sums within the
    reference's bounds; and the whole call twice gives the same bytes"""
    cus = _cus()
    n, d, K = R.large_shapes(cus)[which]
    ntiles, grid, _, _ = _plan(n, K, cus)
    assert ntiles >= 2 * grid
    km, xt, labels, cs, rows, ref = _case("discount", n, d, K)
    g = grid * 64
    cuts = [0, g - 27, 2 * g - 27, n]  # a first piece that ends inside a tile, a full grid of tiles, the rest (92 rows)
    total = np.zeros_like(cs)
    pieces = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        piece_tiles, piece_grid, _, _ = _plan(b - a, K, cus)
        assert 0 < b - a <= g and piece_tiles == piece_grid
        c_part, r_part = km.quality(xt[a:b], labels[a:b], rows=True)
        total += c_part
        pieces.append(r_part)
    assert np.concatenate(pieces).tobytes() == rows.tobytes()
    for col in (R.COUNT, R.DISPLACED):
        assert np.array_equal(total[:, col], cs[:, col])
    for col in (R.SUM_A2, R.SUM_SQRT_A2, R.SUM_S, R.SUM_MIN):
        assert (np.abs(total[:, col] - ref.cluster[:, col]) <= ref.cluster_tol[:, col]).all(), col
    cs2, rows2 = km.quality(xt, labels, rows=True)
    assert cs2.tobytes() == cs.tobytes() and rows2.tobytes() == rows.tobytes()
    assert km.quality(xt, labels).tobytes() == cs.tobytes()  # without row_stats


def _check_rows_and_clusters(case):
    kind, n, d, K = case
    km, xt, labels, cs, rows, ref = _case(*case)
    assert cs.shape == (K, R.COLS) and rows.shape == (n, 2) and cs.dtype == rows.dtype == np.float64
    if K > 1:  # the discount has displaced rows, and the bound decides almost every row
        assert ref.displaced.sum() > 0
    assert ref.undecided.mean() <= 0.01
    a2, b2 = rows[:, 0], rows[:, 1]
    err_a = np.abs(a2 - ref.a2)
    with np.errstate(invalid='ignore'):
        err_b = np.where(np.isinf(ref.b2) & np.isinf(b2), 0.0, np.abs(b2 - ref.b2))
    print("{}: max |a2 - ref| / bound = {:.3g}, max |b2 - ref| / bound = {:.3g}, undecided rows {}, displaced {}".format(
        case, (err_a / np.maximum(ref.ta, 1e-300)).max(), (err_b / np.maximum(ref.tb, 1e-300)).max(), int(ref.undecided.sum()),
        int(ref.displaced.sum())))
    assert (a2 >= 0).all() and (b2 >= 0).all()
    assert (err_a <= ref.ta).all()
    assert (err_b <= ref.tb).all()
    sure = ~ref.undecided
    assert np.array_equal((b2 < a2)[sure], ref.displaced[sure])
    assert np.array_equal(cs[:, R.COUNT], ref.cluster[:, R.COUNT])
    assert np.array_equal(cs[:, R.COUNT], np.bincount(labels.cpu().numpy(), minlength=K))
    err = np.abs(cs - ref.cluster)
    for col in (R.SUM_A2, R.SUM_SQRT_A2, R.SUM_S, R.DISPLACED, R.SUM_MIN):
        print("  column {}: max error {:.3g}, max error / bound {:.3g}".format(
            col, err[:, col].max(), (err[:, col] / np.maximum(ref.cluster_tol[:, col], 1e-300)).max()))
        assert (err[:, col] <= ref.cluster_tol[:, col]).all(), col
    assert np.array_equal(cs[:, R.DISPLACED], np.rint(cs[:, R.DISPLACED]))
    if kind == "special":
        lab = labels.cpu().numpy()
        assert (lab[1:6] == 1).all() and np.array_equal(b2[1:6], a2[1:6])  # twin centres: the same arithmetic, the same bits
        assert cs[3, R.COUNT] == 0 and cs[5, R.COUNT] == 0 and not cs[3].any() and not cs[5].any()
        assert lab[0] == 7 and a2[0] <= ref.ta[0]
    if K == 1:
        assert np.isinf(b2).all() and cs[0, R.SUM_S] == 0 and cs[0, R.DISPLACED] == 0
        assert np.array_equal(cs[0, R.SUM_MIN], cs[0, R.SUM_A2])


@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[5]], ids=[_IDS[2], _IDS[4], _IDS[5]])
def test_same_call_same_bits(env, case):
    km, xt, labels, cs, rows, _ = _case(*case)
    cs2, rows2 = km.quality(xt, labels, rows=True)
    assert cs.tobytes() == cs2.tobytes() and rows.tobytes() == rows2.tobytes()
    assert km.quality(xt, labels).tobytes() == cs.tobytes()  # without row_stats, and host labels / host rows alike
    cs3, rows3 = km.quality(xt.cpu().numpy(), labels.cpu().numpy(), rows=True)
    assert cs3.tobytes() == cs.tobytes() and rows3.tobytes() == rows.tobytes()


@pytest.mark.parametrize("case", [CASES[3], CASES[4]], ids=[_IDS[3], _IDS[4]])
def test_row_stats_do_not_depend_on_the_split(env, case):
    kind, n, d, K = case
    km, xt, labels, cs, rows, ref = _case(*case)
    cuts = [0, 1, 64, 128, n]  # pieces of 1, 63, 64 rows and the rest
    total = np.zeros_like(cs)
    pieces = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        c_part, r_part = km.quality(xt[a:b], labels[a:b], rows=True)
        total += c_part
        pieces.append(r_part)
    assert np.concatenate(pieces).tobytes() == rows.tobytes()
    for col in (R.COUNT, R.DISPLACED):
        assert np.array_equal(total[:, col], cs[:, col])
    for col in (R.SUM_A2, R.SUM_SQRT_A2, R.SUM_S, R.SUM_MIN):
        assert (np.abs(total[:, col] - ref.cluster[:, col]) <= ref.cluster_tol[:, col]).all(), col


def test_labels_default_to_calc_best(env):
    km, xt, labels, cs, rows, _ = _case(*CASES[2])
    assert km.quality(xt).tobytes() == cs.tobytes()


def test_refusals(env):
    import torch
    from acav100m_amd import _lib
    from acav100m_amd.clustering import KMeans
    km, xt, labels, cs, rows, _ = _case(*CASES[2])
    K = cs.shape[0]
    # a label equal to K: refused by the checking kernel, nothing is indexed with it; the outputs stay as they were
    bad = labels.clone()
    bad[17] = K
    out = np.full((K, R.COLS), -1.0)
    rc = _lib._lib.acav_kmeans_quality(km._h, C.c_void_p(xt.data_ptr()), xt.shape[0], C.c_void_p(bad.data_ptr()),
                                       out.ctypes.data_as(C.c_void_p), None)
    assert rc == -1 and b"1 of 65 labels are outside [0, 33)" in _lib._lib.acav_last_error()
    with pytest.raises(ValueError, match="outside"):
        km.quality(xt, bad)
    bad[17] = -1
    with pytest.raises(ValueError, match="outside"):
        km.quality(xt, bad)
    with pytest.raises(ValueError, match="labels"):
        km.quality(xt, labels[:-1])
    # a handle in its warm-up: ACAV_ESTATE before any launch
    warm = KMeans(None, xt.shape[1], K).to("cuda:0")
    assert warm.count < warm.initial_rounds * K
    rc = _lib._lib.acav_kmeans_quality(warm._h, C.c_void_p(xt.data_ptr()), xt.shape[0], C.c_void_p(labels.data_ptr()),
                                       out.ctypes.data_as(C.c_void_p), None)
    assert rc == -4 and b"count=0 < initial_rounds*k=330" in _lib._lib.acav_last_error()
    with pytest.raises(_lib.AcavError, match="warm-up"):
        warm.quality(xt, labels)
    # no rows: zeros
    assert not km.quality(torch.empty((0, xt.shape[1]), device="cuda"), torch.empty(0, dtype=torch.long, device="cuda")).any()
    # and the handle still answers as before
    assert km.quality(xt, labels).tobytes() == cs.tobytes()


def test_the_handle_is_left_alone(env):
    from acav100m_amd import _lib
    km, xt, labels, cs, rows, _ = _case(*CASES[3])

    def snapshot():
        a, s = C.c_int64(0), C.c_int64(0)
        _lib.check(_lib._lib.acav_kmeans_stats(km._h, C.byref(a), C.byref(s)))
        centers, counts, count, fb = km.state_arrays()
        return (a.value, s.value), km.filter_stats(), km.train_stats(), centers.tobytes(), counts.tobytes(), count, fb
    before = snapshot()
    km.quality(xt, labels, rows=True)
    assert snapshot() == before
    again, _ = km.calc_best(xt, need_mean=False)
    assert np.array_equal(again.cpu().numpy(), labels.cpu().numpy())
