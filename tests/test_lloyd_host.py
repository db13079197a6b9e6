"""CPU: the host side of clustering.algorithm=lloyd -- the key and its refusals, the Lloyd state and its pickle, the host half of
an iteration against the restatement, and the argument checks and chunking of acav_lloyd_accumulate, none of which needs a
device."""
import ctypes as C
import pickle

import numpy as np
import pytest

from tests import _lloyd_np as L


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _args(**over):
    from acav100m_amd.config import CLUSTERING_DEFAULTS, merge
    return merge(CLUSTERING_DEFAULTS, over)


def test_key_parses_and_defaults_to_sgd():
    from acav100m_amd.clustering.lloyd import check_algorithm
    from acav100m_amd.config import CLUSTERING_DEFAULTS, parse_cli
    assert CLUSTERING_DEFAULTS["clustering"]["algorithm"] == "sgd"
    command, kwargs = parse_cli(["cluster", "--clustering.algorithm=lloyd", "--clustering.epochs=4", "--feature_path=x"])
    assert command == "cluster" and kwargs["clustering.algorithm"] == "lloyd"
    assert check_algorithm(_args(**kwargs), 1) == "lloyd" and check_algorithm(_args(), 8) == "sgd"


@pytest.mark.parametrize("bad", ["faiss", "scipy", "Lloyd", "", 1, True])
def test_unknown_algorithms_are_refused(bad, tmp_path):
    from acav100m_amd.clustering import run_clustering as rc
    from acav100m_amd.clustering.lloyd import check_algorithm
    with pytest.raises(ValueError, match="clustering.algorithm"):
        check_algorithm(_args(**{"clustering.algorithm": bad}), 1)
    # the stage refuses it before a shard is read: the shard paths do not exist, reading one would fail differently
    args = _args(**{"clustering.algorithm": bad, "data.output.path": str(tmp_path / "out"),
                    "data.path": str(tmp_path / "nowhere" / "shard-{000000..000003}.pkl")})
    with pytest.raises(ValueError, match="clustering.algorithm"):
        rc.run_clustering(args)


def test_row_partitioned_modes_are_refused_in_whitening_s_words():
    from acav100m_amd.clustering.lloyd import check_algorithm
    from acav100m_amd.clustering.run_clustering import check_whiten
    for mode in ("striped", "reference", "rows"):
        args = _args(**{"clustering.algorithm": "lloyd", "clustering.multi_gpu": mode})
        with pytest.raises(ValueError, match=mode) as mine:
            check_algorithm(args, 2)
        with pytest.raises(ValueError) as theirs:
            check_whiten(_args(**{"clustering.whiten": True, "clustering.multi_gpu": mode}), 2)
        # the same restriction in the same words: "<key> with clustering.multi_gpu=<mode> on 2 GPUs: the rows are partitioned
        # over the ranks and <what> are not merged across them; use clustering.multi_gpu=views or one GPU"
        a, b = str(mine.value), str(theirs.value)
        assert a.split(" with ")[1].split(" and ")[0] == b.split(" with ")[1].split(" and ")[0]
        assert a.split("; ")[1] == b.split("; ")[1]
        check_algorithm(args, 1)
        check_algorithm(_args(**{"clustering.multi_gpu": mode}), 8)  # sgd: nothing is refused
    check_algorithm(_args(**{"clustering.algorithm": "lloyd"}), 8)  # views (default)
    with pytest.raises(ValueError, match="epochs"):
        check_algorithm(_args(**{"clustering.algorithm": "lloyd", "clustering.epochs": 0}), 1)


def _lloyd_state(k=4, d=3):
    from acav100m_amd.clustering import KMeans
    km = KMeans(None, d, k)
    return km.to_lloyd(np.arange(k * d, dtype=np.float32).reshape(k, d))


def test_lloyd_state_pickles_and_an_sgd_state_has_no_new_key():
    from acav100m_amd.clustering import KMeans
    sgd = KMeans(None, 3, 4)
    assert set(sgd.get_attrs()) == {"args", "count", "lr", "initial_rounds", "reinit", "fallback", "sequential", "centers", "counts"}
    assert sgd.algorithm is None and sgd.initial_rounds == 10 and tuple(sgd.reinit) == (.7, 5.0)
    km = _lloyd_state()
    attrs = km.get_attrs()
    assert set(attrs) == set(sgd.get_attrs()) | {"algorithm"}
    assert attrs["algorithm"] == "lloyd" and attrs["initial_rounds"] == 0 and tuple(attrs["reinit"]) == (.7, 1.0)
    assert attrs["count"] == 0 and (attrs["counts"] == 0).all()
    for back in (pickle.loads(pickle.dumps(km)), KMeans.load(km.get_attrs_plain())):
        assert back.algorithm == "lloyd" and back.initial_rounds == 0 and tuple(back.reinit) == (.7, 1.0)
        assert np.array_equal(back.get_attrs()["centers"], attrs["centers"])
    again = pickle.loads(pickle.dumps(sgd))
    assert again.algorithm is None and "algorithm" not in again.get_attrs()


def test_cache_round_trip_keeps_the_algorithm_and_adds_nothing_without(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import KMeans
    from acav100m_amd.clustering import run_clustering as rc
    v = ("audio", "layer_vggish", "layer_0")
    plain = _args(**{"data.output.path": str(tmp_path / "plain"), "data.path": "shard-{000000..000003}.pkl"})
    lloyd = _args(**{"data.output.path": str(tmp_path / "lloyd"), "data.path": "shard-{000000..000003}.pkl"})
    rc.save_clusterings(plain, 1, {v: KMeans(None, 3, 4)})
    rc.save_clusterings(lloyd, 1, {v: _lloyd_state()})
    a, b = rc._read_cache(rc._cache_path(plain, 1))[v], rc._read_cache(rc._cache_path(lloyd, 1))[v]
    assert "algorithm" not in a and set(b) == set(a) | {"algorithm"}
    assert b["algorithm"] == "lloyd" and b["initial_rounds"] == 0 and tuple(b["reinit"]) == (.7, 1.0)
    back = KMeans.load(b)
    assert back.algorithm == "lloyd" and back.initial_rounds == 0


def test_resume_training_from_the_other_algorithm_is_refused_before_any_shard_is_read(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import KMeans
    from acav100m_amd.clustering import run_clustering as rc
    v = ("audio", "layer_vggish", "layer_0")
    for trained, asked, state in (("sgd", "lloyd", lambda: KMeans(None, 3, 4)), ("lloyd", "sgd", _lloyd_state)):
        out = tmp_path / trained
        args = _args(**{"data.output.path": str(out), "data.path": str(tmp_path / "nowhere" / "shard-{000000..000003}.pkl"),
                        "clustering.cached_epoch": 1, "clustering.resume_training": True, "clustering.algorithm": asked})
        rc.save_clusterings(args, 1, {v: state()})
        with pytest.raises(ValueError, match="trained by " + trained):
            rc.run_clustering(args)
        # the same algorithm, or no resume_training: not this refusal
        args.clustering.algorithm = trained
        rc.check_cached_algorithm(args)
        args.clustering.algorithm, args.clustering.resume_training = asked, False
        rc.check_cached_algorithm(args)


def test_sgd_entry_points_refuse_a_lloyd_state():
    from acav100m_amd import _lib
    from acav100m_amd.clustering import KMeans
    km = _lloyd_state()
    km._h = C.c_void_p(1)  # (a handle that is never used: every call below is refused before the library is entered)
    try:
        x = np.zeros((8, 3), np.float32)
        for call in (lambda: km.add(x), lambda: km.apply_update(x, np.zeros(8, np.int64), 0.01), lambda: km.train_epoch(x, 4),
                     lambda: KMeans.train_epoch_multi([km], [x], 4), lambda: km.train_epoch_distributed(x, 4),
                     lambda: KMeans.train_epoch_distributed_multi([km], [x], 4), lambda: KMeans.train_epoch_plan_multi([km], [x], None),
                     lambda: km.train_epoch_comm(None, x, 4, 0.01)):
            with pytest.raises(_lib.AcavError, match="Lloyd"):
                call()
    finally:
        km._h = None
    with pytest.raises(_lib.AcavError, match="to_lloyd"):
        from acav100m_amd.clustering import lloyd_update
        lloyd_update(KMeans(None, 3, 4), x, 10)


def test_host_half_of_an_iteration_is_the_restatement():
    from acav100m_amd.clustering import centers_from_sums, fixed_point_shift, split_empty
    rs = np.random.RandomState(5)
    x = (rs.randn(500, 7) * 100).astype(np.float32)
    labels = rs.randint(0, 9, 500)
    labels[labels == 3] = 4
    labels[labels == 6] = 4  # two empty clusters, one large one
    for n in (1, 2, 3, 500, 2 ** 20, 2 ** 20 + 1, 2 ** 27):
        for absmax in (1e-30, 0.5, 1.0, 388.5, 1e30):
            assert fixed_point_shift(absmax, n) == L.shift_of(absmax, n), (absmax, n)
    s = L.shift_of(np.abs(x).max(), 500)
    sums, counts = L.sums_counts(x, labels, 9, s)
    want = L.centers_of(sums, counts, s)
    got = centers_from_sums(sums, counts, s)
    assert got[2] == want[2] == 2
    assert got[0].dtype == np.float32 and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    assert counts[3] == 0 and counts[6] == 0  # the inputs are left alone
    c, n = want[0].copy(), np.array([5, 0, 5, 0], np.int64)
    c2, n2 = c[:4].copy(), n.copy()
    assert split_empty(c2, n2) == L.split_empty(c[:4], n) == 2 and c2.tobytes() == c[:4].tobytes() and np.array_equal(n, n2)
    for bad in (0.0, float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            fixed_point_shift(bad, 10)


HISTS = [([2500, 300, 0, 150, 50], 88), ([1] * 300, 1408), ([513, 512, 511, 1, 0, 1024, 1025], 64), ([0] * 324 + [1] * 700, 64),
         ([10 ** 6 // 2] + [500] * 1000, 1024)]


@pytest.mark.parametrize("hist,d", HISTS)
def test_plan_cuts_every_list_into_chunks_of_at_most_512(hist, d):
    from acav100m_amd.clustering.lloyd import accumulate_plan
    hist = np.asarray(hist, np.int64)
    plan, chunks = accumulate_plan(hist, d, cus=256)
    assert plan["chunk_rows"] == 512 and plan["chunks"] == len(chunks) == int((-(-hist // 512)).sum())
    assert plan["strips"] == -(-d // 64) and plan["items"] == plan["chunks"] * plan["strips"]
    assert 1 <= plan["grid"] <= 8 * 256 and plan["grid"] <= max(1, -(-plan["items"] // 4))
    assert plan["bin_grid"] * plan["bin_rows"] >= hist.sum() and plan["lds_bins"] == 1
    assert (chunks[:, 2] >= 1).all() and (chunks[:, 2] <= 512).all()
    # every position of the label-ordered index lies in exactly one chunk, and that chunk carries the position's label
    starts = np.concatenate([[0], np.cumsum(hist)])
    seen = np.zeros(int(hist.sum()), np.int64)
    for label, start, rows in chunks:
        seen[start:start + rows] += 1
        assert starts[label] <= start and start + rows <= starts[label + 1]
    assert (seen == 1).all()
    assert (np.diff(chunks[:, 0]) >= 0).all()  # label order
    # the largest list is many waves' work, never one's
    assert (chunks[:, 0] == int(np.argmax(hist))).sum() == -(-int(hist.max()) // 512)


@pytest.mark.parametrize("cus", [256, 80])
def test_plan_past_its_caps(cus):
    """the arms and the clamps of the launch plan: no LDS histogram past 8192 clusters, the sum grid at 8 workgroups per compute
    unit once there are more than 4 x 8 x cus items, the binning grid at 4 per unit with ceil(n / grid) rows each past
    4096 x 4 x cus rows"""
    from acav100m_amd.clustering.lloyd import accumulate_plan
    for k, lds in ((8192, 1), (8193, 0), (20000, 0)):
        hist = np.zeros(k, np.int64)
        hist[[0, k // 2, k - 1]] = 700, 1, 1
        plan, chunks = accumulate_plan(hist, 3, cus=cus)
        assert plan["lds_bins"] == lds and plan["chunks"] == len(chunks) == 4 and plan["bin_grid"] == 1 and plan["bin_rows"] == 702
        assert chunks.tolist() == [[0, 0, 512], [0, 512, 188], [k // 2, 700, 1], [k - 1, 701, 1]]
    # one-row lists at d = 130: three strips per chunk
    for n in (4 * 8 * cus // 3, 4 * 8 * cus // 3 + 1, 4 * 8 * cus // 3 + 270):
        plan, _chunks = accumulate_plan(np.ones(n, np.int64), 130, cus=cus)
        assert plan["items"] == 3 * n and plan["grid"] == min(-(-3 * n // 4), 8 * cus)
        if plan["items"] > 4 * 8 * cus:
            assert plan["grid"] == 8 * cus
    assert plan["items"] > 4 * 8 * cus
    for n in (4096 * 4 * cus - 1, 4096 * 4 * cus, 4096 * 4 * cus + 1, 3 * 4096 * 4 * cus + 5):
        hist = np.array([n - n // 2, 0, n // 2], np.int64)
        plan, _chunks = accumulate_plan(hist, 1, cus=cus)
        assert plan["bin_grid"] == min(-(-n // 4096), 4 * cus) and plan["bin_rows"] == -(-n // plan["bin_grid"])
        assert (plan["bin_rows"] > 4096) == (n > 4096 * 4 * cus)
        assert plan["bin_grid"] * plan["bin_rows"] >= n > (plan["bin_grid"] - 1) * plan["bin_rows"]  # no workgroup without rows
    assert plan["bin_grid"] == 4 * cus and plan["bin_rows"] == 3 * 4096 + 1


def test_accumulate_refuses_bad_arguments_without_a_device(lib):
    x = np.zeros((10, 4), np.float32)
    lab = np.zeros(10, np.int64)
    sums, counts = np.full((3, 4), 7, np.int64), np.full(3, 7, np.int64)
    xp, lp, sp, cp = (a.ctypes.data_as(C.c_void_p) for a in (x, lab, sums, counts))
    for args in ((0, None, 10, 4, lp, 3, 0, sp, cp), (0, xp, 10, 4, None, 3, 0, sp, cp), (0, xp, 10, 4, lp, 3, 0, None, cp),
                 (0, xp, 10, 4, lp, 3, 0, sp, None), (0, xp, -1, 4, lp, 3, 0, sp, cp), (0, xp, 2 ** 31, 4, lp, 3, 0, sp, cp),
                 (0, xp, 10, 0, lp, 3, 0, sp, cp), (0, xp, 10, 16385, lp, 3, 0, sp, cp), (0, xp, 10, 4, lp, 0, 0, sp, cp),
                 (0, xp, 10, 4, lp, 2 ** 29, 0, sp, cp), (0, xp, 10, 4, lp, 3, 1001, sp, cp), (0, xp, 10, 4, lp, 3, -1001, sp, cp)):
        assert lib.acav_lloyd_accumulate(*args, None) == -1, args
    assert lib.acav_lloyd_accumulate(0, None, 0, 4, None, 3, 0, sp, cp, None) == 0  # no rows: a no-op, no device needed
    assert (sums == 7).all() and (counts == 7).all()
    out = C.c_float(7)
    for args in ((0, None, 10, 4), (0, xp, -1, 4), (0, xp, 2 ** 37, 4), (0, xp, 10, 0), (0, xp, 10, 16385)):
        assert lib.acav_rows_absmax(*args, C.byref(out), None) == -1, args
    assert lib.acav_rows_absmax(0, xp, 10, 4, None, None) == -1
    assert lib.acav_rows_absmax(0, None, 0, 4, C.byref(out), None) == 0 and out.value == 0.0
    plan = (C.c_int64 * 9)()
    hist = np.array([5, 5], np.int64)
    hp = hist.ctypes.data_as(C.c_void_p)
    for args in ((None, 2, 4, 256, plan, None, 0), (hp, 0, 4, 256, plan, None, 0), (hp, 2, 0, 256, plan, None, 0),
                 (hp, 2, 4, 0, plan, None, 0), (hp, 2, 4, 256, None, None, 0), (hp, 2, 4, 256, plan, sp, 1)):
        assert lib.acav_lloyd_accumulate_plan(*args) == -1, args
    for bad in ([-1, 5], [2 ** 31, 0], [2 ** 30, 2 ** 30]):
        h = np.array(bad, np.int64)
        assert lib.acav_lloyd_accumulate_plan(h.ctypes.data_as(C.c_void_p), 2, 4, 256, plan, None, 0) == -1, bad
