"""CPU: the host side of clustering.pca_dim -- the refusal of row-partitioned multi-GPU modes, the key, the cache keys, the two
refusals of a cached run, and the argument checks and launch plan of acav_rows_scatter / acav_rows_project, none of which
needs a device."""
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


def test_check_pca_refuses_row_partitioned_modes():
    from acav100m_amd.clustering.run_clustering import check_pca
    for mode in ("striped", "reference", "rows"):
        args = _args(**{"clustering.pca_dim": 32, "clustering.multi_gpu": mode})
        with pytest.raises(ValueError, match=mode):
            check_pca(args, 2)
        check_pca(args, 1)  # one GPU: every mode is the one-GPU run
        check_pca(_args(**{"clustering.multi_gpu": mode}), 8)  # without the key nothing is refused
    check_pca(_args(**{"clustering.pca_dim": 32}), 8)  # views (default)
    check_pca(_args(**{"clustering.pca_dim": 32, "clustering.multi_gpu": "views"}), 2)
    for bad in (0, -3, 2.5, True, "many"):
        with pytest.raises(ValueError, match="pca_dim"):
            check_pca(_args(**{"clustering.pca_dim": bad}), 1)


def test_key_parses_and_defaults_to_none():
    from acav100m_amd.config import CLUSTERING_DEFAULTS, parse_cli
    assert CLUSTERING_DEFAULTS["clustering"]["pca_dim"] is None
    command, kwargs = parse_cli(["cluster", "--clustering.pca_dim=256", "--feature_path=x"])
    assert command == "cluster" and kwargs["clustering.pca_dim"] == 256
    assert _args(**kwargs).clustering.pca_dim == 256 and _args().clustering.pca_dim is None


def test_names_are_exported():
    import acav100m_amd.clustering as c
    for name in ("PCA", "ScatterMoments", "project", "pca_feature", "pca_features", "whiten"):
        assert hasattr(c, name), name


class _FakeKMeans:
    def __init__(self, d):
        self.d = d

    def get_attrs_plain(self):
        return {'count': 320, 'lr': 0.01, 'initial_rounds': 10, 'reinit': (.7, 5.0), 'fallback': 0, 'sequential': False,
                'centers': np.arange(4 * self.d, dtype=np.float32).reshape(4, self.d), 'counts': np.ones(4, np.float32)}


def _fit(d, p, seed):
    rs = np.random.RandomState(seed)
    return {'mean': rs.randn(d).astype(np.float32), 'components': rs.randn(p, d).astype(np.float32),
            'explained_variance': np.sort(rs.rand(p))[::-1].copy(), 'total_variance': np.float64(p + rs.rand())}


VIEWS = [("audio", "layer_vggish", "layer_0"), ("video", "layer_slow_fast", "layer_0"), ("video", "layer_slow_fast", "layer_1")]


def test_cache_round_trip_keeps_the_projection_and_adds_nothing_without(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import run_clustering as rc
    cl = {v: _FakeKMeans(2) for v in VIEWS}
    fits = {VIEWS[0]: _fit(5, 2, 0), VIEWS[1]: _fit(7, 2, 1), VIEWS[2]: None}  # the third view is not wider than pca_dim
    stds = {VIEWS[0]: np.array([1.0, 0.5, 2.0, 1.0, 3.0], np.float32)}
    plain = _args(**{"data.output.path": str(tmp_path / "plain"), "data.path": "shard-{000000..000003}.pkl"})
    proj = _args(**{"data.output.path": str(tmp_path / "proj"), "data.path": "shard-{000000..000003}.pkl"})
    rc.save_clusterings(plain, 1, cl)
    rc.save_clusterings(proj, 1, cl, stds, fits)
    a, b = rc._read_cache(rc._cache_path(plain, 1)), rc._read_cache(rc._cache_path(proj, 1))
    assert list(a) == VIEWS and list(b) == VIEWS
    new = {"pca_mean", "pca_components", "pca_explained_variance", "pca_total_variance"}
    assert set(rc.PCA_KEYS) == new
    for v in VIEWS:
        assert set(a[v]) == set(_FakeKMeans(1).get_attrs_plain())  # today's keys ('_kind' moves into the view key)
        extra = (new if fits[v] is not None else set()) | ({"whiten_std"} if v in stds else set())
        assert set(b[v]) == set(a[v]) | extra
        if fits[v] is None:
            assert rc._pca_of(b[v]) is None
            continue
        got = rc._pca_of(b[v])
        assert got["mean"].dtype == np.float32 and got["mean"].tobytes() == fits[v]["mean"].tobytes()
        assert got["components"].dtype == np.float32 and got["components"].shape == fits[v]["components"].shape
        assert got["components"].tobytes() == fits[v]["components"].tobytes()
        assert got["explained_variance"].dtype == np.float64 and got["explained_variance"].tobytes() == fits[v]["explained_variance"].tobytes()
        assert isinstance(got["total_variance"], np.float64) and got["total_variance"] == fits[v]["total_variance"]
    # what a cached run reads: the file it will load, and the projections by (model_key, layer) -- no key, no flag needed
    proj.clustering.cached_epoch = 1
    path, found = rc.cached_projection(proj)
    assert path == rc._cache_path(proj, 1) and set(found) == {v[1:] for v in VIEWS[:2]}
    proj.clustering.pca_dim = 2  # agreeing with the cache is fine
    assert set(rc.cached_projection(proj)[1]) == set(found)
    plain.clustering.cached_epoch = 1
    path, found = rc.cached_projection(plain)
    assert path == rc._cache_path(plain, 1) and found == {}
    plain.clustering.cached_epoch = None
    assert rc.cached_projection(plain) == (None, {})
    plain.clustering.pca_dim = 2  # a fresh run: nothing to disagree with
    assert rc.cached_projection(plain) == (None, {})


def test_cached_runs_refuse_a_pca_dim_the_cache_does_not_have_before_any_shard_is_read(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import run_clustering as rc
    common = {"data.path": str(tmp_path / "nowhere" / "shard-{000000..000003}.pkl"), "clustering.cached_epoch": 1}
    # (1) pca_dim against a cache without the keys
    args = _args(**{"data.output.path": str(tmp_path / "plain"), "clustering.pca_dim": 2}, **common)
    rc.save_clusterings(args, 1, {VIEWS[0]: _FakeKMeans(5)})
    with pytest.raises(ValueError, match="cache_epoch_1_.*pca_components|pca_components.*cache_epoch_1_"):
        rc.run_clustering(args)  # the shard paths do not exist: reading one would fail differently
    # (2) a pca_dim that disagrees with the cached p
    args = _args(**{"data.output.path": str(tmp_path / "proj"), "clustering.pca_dim": 3}, **common)
    rc.save_clusterings(args, 1, {VIEWS[0]: _FakeKMeans(2)}, None, {VIEWS[0]: _fit(5, 2, 0)})
    with pytest.raises(ValueError, match="cache_epoch_1_") as err:
        rc.run_clustering(args)
    assert "pca_dim=3" in str(err.value) and "2 columns" in str(err.value)


def test_evaluate_refuses_epochs_that_disagree_on_the_projection(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import run_clustering as rc
    from acav100m_amd.clustering.evaluate import load_states
    v = VIEWS[0]
    args = _args(**{"data.output.path": str(tmp_path / "out"), "data.path": "shard-{000000..000003}.pkl", "models": ["layer_vggish"]})
    f = _fit(5, 2, 0)
    g = dict(f, components=np.nextafter(f["components"], np.float32(4)))
    rc.save_clusterings(args, 0, {v: _FakeKMeans(2)}, None, {v: f})
    rc.save_clusterings(args, 1, {v: _FakeKMeans(2)}, None, {v: dict(f)})
    rc.save_clusterings(args, 2, {v: _FakeKMeans(2)}, None, {v: g})
    rc.save_clusterings(args, 3, {v: _FakeKMeans(2)})
    assert list(load_states(args, [0, 1])) == [0, 1]
    assert list(load_states(args, [3])) == [3]
    for epochs in ([0, 2], [1, 3], [3, 0]):
        with pytest.raises(ValueError, match="pca projection"):
            load_states(args, epochs)


def test_components_from_scatter_is_the_restatement():
    from acav100m_amd.clustering.pca import components_from_scatter
    from tests import _pca_np as R
    x = R.recipe(300, 20, 1)
    want = R.fit(x, 6)
    got = components_from_scatter(300, want["mean64"], want["S"], 6)
    assert got["mean"].tobytes() == want["mean"].tobytes() and got["components"].tobytes() == want["components"].tobytes()
    assert got["explained_variance"].tobytes() == want["explained_variance"].tobytes()
    assert got["total_variance"] == want["total_variance"] and isinstance(got["total_variance"], np.float64)
    with pytest.raises(ValueError, match="view a/b.*N <= p"):
        components_from_scatter(6, want["mean64"], want["S"], 6, what="view a/b")


BAD_PREFIX = [([0, 5, 3, 10], 10), ([0, 5, 9], 10), ([1, 5, 10], 10), ([0, 11, 10], 10)]


def test_rows_scatter_refuses_bad_arguments_without_a_device(lib):
    x = np.zeros((10, 4), np.float32)
    shift = np.zeros(4, np.float32)
    s, g = np.full(4, 7.0), np.full((4, 4), 7.0)
    xp, hp, sp, gp = (a.ctypes.data_as(C.c_void_p) for a in (x, shift, s, g))
    for prefix, n in BAD_PREFIX:
        p = np.asarray(prefix, np.int64)
        assert lib.acav_rows_scatter(0, xp, n, 4, p.ctypes.data_as(C.c_void_p), len(p) - 1, hp, sp, gp, None) == -1, prefix
    good = np.array([0, 10], np.int64).ctypes.data_as(C.c_void_p)
    for d in (0, 16385, -1):
        assert lib.acav_rows_scatter(0, xp, 10, d, good, 1, hp, sp, gp, None) == -1, d
    for args in ((None, 10, 4, good, 1, hp, sp, gp), (xp, 10, 4, None, 1, hp, sp, gp), (xp, 10, 4, good, 1, None, sp, gp),
                 (xp, 10, 4, good, 1, hp, None, gp), (xp, 10, 4, good, 1, hp, sp, None), (xp, 10, 4, good, 0, hp, sp, gp),
                 (xp, -1, 4, good, 1, hp, sp, gp)):
        assert lib.acav_rows_scatter(0, *args, None) == -1, args
    for bad in (np.nan, np.inf):
        h = np.array([0, bad, 0, 0], np.float32)
        assert lib.acav_rows_scatter(0, xp, 10, 4, good, 1, h.ctypes.data_as(C.c_void_p), sp, gp, None) == -1
    # no rows: a no-op, and no device is needed for that
    empty = np.array([0, 0, 0], np.int64)
    assert lib.acav_rows_scatter(0, None, 0, 4, empty.ctypes.data_as(C.c_void_p), 2, hp, sp, gp, None) == 0
    assert (s == 7.0).all() and (g == 7.0).all()  # nothing was written


def test_rows_project_refuses_bad_arguments_without_a_device(lib):
    x = np.ones((2, 3), np.float32)
    mean, comps, y = np.zeros(3, np.float32), np.ones((2, 3), np.float32), np.full((2, 2), 7.0, np.float32)
    xp, mp, cp, yp = (a.ctypes.data_as(C.c_void_p) for a in (x, mean, comps, y))
    for args in ((xp, 2, 0, mp, cp, 2, yp), (xp, 2, 16385, mp, cp, 2, yp), (xp, 2, 3, mp, cp, 0, yp), (xp, 2, 3, mp, cp, 16385, yp),
                 (xp, -1, 3, mp, cp, 2, yp), (None, 2, 3, mp, cp, 2, yp), (xp, 2, 3, None, cp, 2, yp), (xp, 2, 3, mp, None, 2, yp),
                 (xp, 2, 3, mp, cp, 2, None)):
        assert lib.acav_rows_project(0, *args, None) == -1, args
    assert lib.acav_rows_project(0, None, 0, 3, mp, cp, 2, None, None) == 0  # no rows: a no-op
    assert (y == 7.0).all() and (x == 1).all()


def _plan(lib, n, d, cus):
    out = (C.c_int64 * 7)(*([-7] * 7))
    assert lib.acav_rows_scatter_plan(n, d, cus, out) == 0, (n, d, cus)
    return tuple(out)


def test_rows_scatter_plan(lib):
    # (n, d, cus) -> (slice rows, block, block pairs, slices of a round, workgroups of the largest launch, LDS, scratch)
    per = lambda pairs, nb: 8 * (pairs * 4096 + nb * 64)  # noqa: E731  (bytes a slice's partials take)
    desc = 16 * 65536
    for args, want in [((0, 64, 256), (1024, 64, 1, 512, 0, 40960, per(1, 1) * 514 + desc)),
                       ((1, 64, 256), (1024, 64, 1, 512, 1, 40960, per(1, 1) * 514 + desc)),
                       ((1025, 65, 256), (1024, 64, 3, 171, 6, 40960, per(3, 2) * 173 + desc)),
                       ((10 ** 6, 64, 256), (1024, 64, 1, 512, 512, 40960, per(1, 1) * 514 + desc)),
                       ((10 ** 6, 1024, 256), (1024, 64, 136, 4, 544, 40960, per(136, 16) * 6 + desc)),
                       ((10 ** 6, 2304, 256), (1024, 64, 666, 4, 2664, 40960, per(666, 36) * 6 + desc)),
                       ((10 ** 6, 64, 8), (1024, 64, 1, 16, 16, 40960, per(1, 1) * 18 + desc)),
                       ((10 ** 6, 64, 4096), (1024, 64, 1, 1024, 977, 40960, per(1, 1) * 1026 + desc)),
                       ((5000, 16384, 256), (1024, 64, 32896, 1, 32896, 40960, per(32896, 256) * 3 + desc))]:
        assert _plan(lib, *args) == want, args
    out = (C.c_int64 * 7)()
    for args in ((-1, 64, 256), (2 ** 37, 64, 256), (100, 0, 256), (100, 16385, 256), (100, 64, 0)):
        assert lib.acav_rows_scatter_plan(*args, out) == -1, args
    assert lib.acav_rows_scatter_plan(100, 64, 256, None) == -1


def test_rows_scatter_plan_scratch_does_not_grow_with_n(lib):
    for d, cus in ((64, 256), (1024, 256), (2304, 8), (16384, 304)):
        base = _plan(lib, 1, d, cus)
        last = 0
        for n in [1, 1023, 1024, 1025, 65536, 10 ** 6, 2 ** 30, 2 ** 37 - 1]:
            cur = _plan(lib, n, d, cus)
            assert cur[:4] == base[:4] and cur[5:] == base[5:], (n, d, cus)  # only the launch size depends on n
            assert cur[4] >= last and cur[4] == min(-(-n // 1024), cur[3]) * cur[2]
            last = cur[4]
        assert 8 * (base[2] * 4096 + -(-d // 64) * 64) * base[3] <= max(512 << 20, 8 * (base[2] * 4096 + -(-d // 64) * 64))
