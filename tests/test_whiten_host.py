"""CPU: the host side of clustering.whiten -- the refusal of row-partitioned multi-GPU modes, the flag, the cache key, and the
argument checks and launch plan of acav_colstats / acav_rows_scale, none of which needs a device."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _args(**over):
    from acav100m_amd.config import CLUSTERING_DEFAULTS, merge
    return merge(CLUSTERING_DEFAULTS, over)


def test_check_whiten_refuses_row_partitioned_modes():
    from acav100m_amd.clustering.run_clustering import check_whiten
    for mode in ("striped", "reference", "rows"):
        args = _args(**{"clustering.whiten": True, "clustering.multi_gpu": mode})
        with pytest.raises(ValueError, match=mode):
            check_whiten(args, 2)
        check_whiten(args, 1)  # one GPU: every mode is the one-GPU run
        check_whiten(_args(**{"clustering.multi_gpu": mode}), 8)  # without the switch nothing is refused
    check_whiten(_args(**{"clustering.whiten": True}), 8)  # views (default)
    check_whiten(_args(**{"clustering.whiten": True, "clustering.multi_gpu": "views"}), 2)


def test_flag_parses_and_defaults_to_off():
    from acav100m_amd.config import CLUSTERING_DEFAULTS, parse_cli
    assert CLUSTERING_DEFAULTS["clustering"]["whiten"] is False
    command, kwargs = parse_cli(["cluster", "--clustering.whiten=True", "--feature_path=x"])
    assert command == "cluster" and kwargs["clustering.whiten"] is True
    assert _args(**kwargs).clustering.whiten is True and _args().clustering.whiten is False


class _FakeKMeans:
    def __init__(self, d):
        self.d = d

    def get_attrs_plain(self):
        return {'count': 320, 'lr': 0.01, 'initial_rounds': 10, 'reinit': (.7, 5.0), 'fallback': 0, 'sequential': False,
                'centers': np.arange(4 * self.d, dtype=np.float32).reshape(4, self.d), 'counts': np.ones(4, np.float32)}


def test_cache_round_trip_keeps_whiten_std_and_adds_nothing_without(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import run_clustering as rc
    views = [("audio", "layer_vggish", "layer_0"), ("video", "layer_slow_fast", "layer_0")]
    cl = {v: _FakeKMeans(3 + i) for i, v in enumerate(views)}
    stds = {views[0]: np.array([1.0, 0.5, 2.0 ** -20], np.float32), views[1]: np.array([3.0, 1.0, 1e3, 1e-3], np.float32)}
    plain = _args(**{"data.output.path": str(tmp_path / "plain"), "data.path": "shard-{000000..000003}.pkl"})
    white = _args(**{"data.output.path": str(tmp_path / "white"), "data.path": "shard-{000000..000003}.pkl"})
    rc.save_clusterings(plain, 1, cl)
    rc.save_clusterings(white, 1, cl, stds)
    a, b = rc._read_cache(rc._cache_path(plain, 1)), rc._read_cache(rc._cache_path(white, 1))
    assert list(a) == views and list(b) == views
    for v in views:
        assert set(a[v]) == set(_FakeKMeans(1).get_attrs_plain())  # today's keys ('_kind' moves into the view key)
        assert set(b[v]) == set(a[v]) | {"whiten_std"}
        assert b[v]["whiten_std"].dtype == np.float32 and b[v]["whiten_std"].tobytes() == stds[v].tobytes()
        assert np.array_equal(a[v]["centers"], b[v]["centers"])
    # what a cached run reads: the file it will load, and the divisors by (model_key, layer)
    white.clustering.cached_epoch = 1
    path, found = rc.cached_whitening(white)
    assert path == rc._cache_path(white, 1) and set(found) == {v[1:] for v in views}
    plain.clustering.cached_epoch = 1
    path, found = rc.cached_whitening(plain)
    assert path == rc._cache_path(plain, 1) and found == {}
    plain.clustering.cached_epoch = None
    assert rc.cached_whitening(plain) == (None, {})


def test_whiten_against_an_unwhitened_cache_is_refused_before_any_shard_is_read(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import run_clustering as rc
    args = _args(**{"data.output.path": str(tmp_path / "out"), "data.path": str(tmp_path / "nowhere" / "shard-{000000..000003}.pkl"),
                    "clustering.whiten": True, "clustering.cached_epoch": 1})
    rc.save_clusterings(args, 1, {("audio", "layer_vggish", "layer_0"): _FakeKMeans(3)})
    with pytest.raises(ValueError, match="cache_epoch_1_"):
        rc.run_clustering(args)  # the shard paths do not exist: reading one would fail differently


def test_evaluate_refuses_epochs_that_disagree_on_whiten_std(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import run_clustering as rc
    from acav100m_amd.clustering.evaluate import load_states
    v = ("audio", "layer_vggish", "layer_0")
    args = _args(**{"data.output.path": str(tmp_path / "out"), "data.path": "shard-{000000..000003}.pkl", "models": ["layer_vggish"]})
    s = np.array([1.0, 0.5, 2.0], np.float32)
    rc.save_clusterings(args, 0, {v: _FakeKMeans(3)}, {v: s})
    rc.save_clusterings(args, 1, {v: _FakeKMeans(3)}, {v: s.copy()})
    rc.save_clusterings(args, 2, {v: _FakeKMeans(3)}, {v: np.nextafter(s, np.float32(4))})
    rc.save_clusterings(args, 3, {v: _FakeKMeans(3)})
    assert list(load_states(args, [0, 1])) == [0, 1]
    assert list(load_states(args, [3])) == [3]
    for epochs in ([0, 2], [1, 3], [3, 0]):
        with pytest.raises(ValueError, match="whiten_std"):
            load_states(args, epochs)


BAD_PREFIX = [([0, 5, 3, 10], 10), ([0, 5, 9], 10), ([1, 5, 10], 10), ([0, 11, 10], 10)]


def test_colstats_refuses_bad_arguments_without_a_device(lib):
    x = np.zeros((10, 4), np.float32)
    out = np.full((3, 2, 4), 7.0)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for prefix, n in BAD_PREFIX:
        p = np.asarray(prefix, np.int64)
        assert lib.acav_colstats(0, xp, n, 4, p.ctypes.data_as(C.c_void_p), len(p) - 1, op, None) == -1, prefix
    good = np.array([0, 10], np.int64).ctypes.data_as(C.c_void_p)
    for d in (0, 16385, -1):
        assert lib.acav_colstats(0, xp, 10, d, good, 1, op, None) == -1, d
    assert lib.acav_colstats(0, None, 10, 4, good, 1, op, None) == -1
    assert lib.acav_colstats(0, xp, 10, 4, None, 1, op, None) == -1
    assert lib.acav_colstats(0, xp, 10, 4, good, 1, None, None) == -1
    assert lib.acav_colstats(0, xp, 10, 4, good, 0, op, None) == -1
    assert lib.acav_colstats(0, xp, -1, 4, good, 1, op, None) == -1
    assert (out == 7.0).all()  # a refused call writes nothing
    # no rows: zeros, and no device is needed for that
    empty = np.array([0, 0, 0], np.int64)
    assert lib.acav_colstats(0, None, 0, 4, empty.ctypes.data_as(C.c_void_p), 2, op, None) == 0
    assert (out[:2] == 0).all() and (out[2] == 7.0).all()


def test_rows_scale_refuses_bad_divisors_without_a_device(lib):
    x = np.ones((2, 3), np.float32)
    xp = x.ctypes.data_as(C.c_void_p)
    for bad in (0.0, -1.0, np.nan, np.inf):
        s = np.array([1.0, bad, 2.0], np.float32)
        assert lib.acav_rows_scale(0, xp, 2, 3, s.ctypes.data_as(C.c_void_p), None) == -1, bad
    s = np.ones(3, np.float32).ctypes.data_as(C.c_void_p)
    assert lib.acav_rows_scale(0, xp, 2, 0, s, None) == -1
    assert lib.acav_rows_scale(0, xp, 2, 16385, s, None) == -1
    assert lib.acav_rows_scale(0, xp, 2, 3, None, None) == -1
    assert lib.acav_rows_scale(0, None, 2, 3, s, None) == -1
    assert (x == 1).all()


def test_colstats_plan(lib):
    out = (C.c_int64 * 6)(*([-7] * 6))
    # (n, d, tiles, cus) -> (tile rows, tiles, strips, grid, LDS bytes, scratch bytes = 16 d tiles + 16 tiles)
    for args, want in [((0, 64, -1, 256), (256, 0, 1, 0, 16384, 0)),
                       ((1, 64, -1, 256), (256, 1, 1, 1, 16384, 16 * 64 + 16)),
                       ((256, 256, -1, 256), (256, 1, 1, 1, 16384, 16 * 256 + 16)),
                       ((257, 257, -1, 256), (256, 2, 2, 4, 16384, 2 * (16 * 257 + 16))),
                       ((257, 257, 200, 256), (256, 200, 2, 400, 16384, 200 * (16 * 257 + 16))),
                       ((10 ** 6, 1024, -1, 256), (256, 3907, 4, 2048, 16384, 3907 * (16 * 1024 + 16))),
                       ((10 ** 6, 1024, 4000, 256), (256, 4000, 4, 2048, 16384, 4000 * (16 * 1024 + 16))),
                       ((256 * 2049 + 1, 64, -1, 256), (256, 2050, 1, 2048, 16384, 2050 * (16 * 64 + 16))),
                       ((4099, 1408, -1, 8), (256, 17, 6, 64, 16384, 17 * (16 * 1408 + 16)))]:
        assert lib.acav_colstats_plan(*args, out) == 0, args
        assert tuple(out) == want, args
    for args in ((-1, 64, -1, 256), (2 ** 37, 64, -1, 256), (100, 0, -1, 256), (100, 16385, -1, 256), (100, 64, -1, 0),
                 (1000, 64, 3, 256), (10, 64, 11, 256)):
        assert lib.acav_colstats_plan(*args, out) == -1, args
    assert lib.acav_colstats_plan(100, 64, -1, 256, None) == -1


def test_colstats_plan_is_monotone_in_n(lib):
    out = (C.c_int64 * 6)()
    for d, cus in ((64, 256), (1024, 256), (2304, 8)):
        last = (0, 0, 0)
        for n in [0, 1, 255, 256, 257, 1000, 65536, 65537, 10 ** 6, 2 ** 30, 2 ** 37 - 1]:
            assert lib.acav_colstats_plan(n, d, -1, cus, out) == 0
            cur = (out[1], out[3], out[5])
            assert all(c >= p for c, p in zip(cur, last)), (n, d, cus)
            assert out[3] <= 8 * cus and out[1] == -(-n // 256)
            last = cur
