"""CPU: the host side of clustering.normalize / clustering.spherical -- the option checks, the third stage of FrontEnd and its
cache key, the refusals of a cached run, and the argument checks and launch plan of acav_rows_normalize, none of which needs a
device."""
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


# ------------------------------------------------------------------------------------------------------------------ options
def test_flags_parse_and_default_to_off():
    from acav100m_amd.config import CLUSTERING_DEFAULTS, parse_cli
    assert CLUSTERING_DEFAULTS["clustering"]["normalize"] is False and CLUSTERING_DEFAULTS["clustering"]["spherical"] is False
    _, kwargs = parse_cli(["cluster", "--clustering.normalize=True", "--clustering.spherical=True", "--feature_path=x"])
    assert kwargs["clustering.normalize"] is True and kwargs["clustering.spherical"] is True
    assert _args(**kwargs).clustering.spherical is True and _args().clustering.normalize is False


def test_spherical_needs_lloyd_and_implies_normalize():
    from acav100m_amd.clustering.options import check_normalize
    assert check_normalize(_args(), 1) == (False, False)
    assert check_normalize(_args(**{"clustering.normalize": True}), 1) == (True, False)
    assert check_normalize(_args(**{"clustering.normalize": True, "clustering.algorithm": "lloyd"}), 1) == (True, False)
    assert check_normalize(_args(**{"clustering.spherical": True, "clustering.algorithm": "lloyd"}), 1) == (True, True)
    with pytest.raises(ValueError, match="SGD chain has no such step"):
        check_normalize(_args(**{"clustering.spherical": True}), 1)
    with pytest.raises(ValueError, match="algorithm=sgd"):
        check_normalize(_args(**{"clustering.spherical": True, "clustering.algorithm": "sgd", "clustering.normalize": True}), 1)


@pytest.mark.parametrize("key", ["normalize", "spherical"])
def test_values_that_are_not_bools_are_refused(key):
    from acav100m_amd.clustering.run_clustering import check_options
    for bad in (1, 0, "True", "yes", 1.0, [True]):
        with pytest.raises(ValueError, match="clustering." + key):
            check_options(_args(**{"clustering." + key: bad, "clustering.algorithm": "lloyd"}), 1)


def test_several_gpus():
    from acav100m_amd.clustering.run_clustering import check_options
    for mode in ("striped", "reference", "rows"):  # the partitioned modes of the SGD chain
        args = _args(**{"clustering.normalize": True, "clustering.multi_gpu": mode})
        with pytest.raises(ValueError, match="nothing would have to be merged.*no test covers"):
            check_options(args, 2)
        check_options(args, 1)  # one GPU: every mode is the one-GPU run
        check_options(_args(**{"clustering.multi_gpu": mode}), 8)  # without the switch nothing is refused
    check_options(_args(**{"clustering.normalize": True}), 8)  # views (default)
    check_options(_args(**{"clustering.normalize": True, "clustering.multi_gpu": "views"}), 2)
    for extra in ({"clustering.normalize": True}, {"clustering.spherical": True}, {"clustering.spherical": True, "clustering.whiten": True}):
        check_options(_args(**{"clustering.algorithm": "lloyd", "clustering.multi_gpu": "rows", **extra}), 2)
        check_options(_args(**{"clustering.algorithm": "lloyd", "clustering.multi_gpu": "views", **extra}), 2)
    for mode in ("striped", "reference"):  # (lloyd itself refuses these)
        with pytest.raises(ValueError):
            check_options(_args(**{"clustering.algorithm": "lloyd", "clustering.spherical": True, "clustering.multi_gpu": mode}), 2)


# ----------------------------------------------------------------------------------------------------------------- FrontEnd
def _pca(d=4, p=2):
    return {'mean': np.zeros(d, np.float32), 'components': np.eye(p, d, dtype=np.float32), 'explained_variance': np.ones(p),
            'total_variance': 3.0}


def test_front_end_attrs_round_trip_and_the_key_is_absent_when_off():
    from acav100m_amd.clustering.frontend import FrontEnd
    std = np.array([1, 2, 3, 4], np.float32)
    assert FrontEnd().to_attrs() == {} and FrontEnd().normalize is False
    assert FrontEnd(normalize=True).to_attrs() == {'normalize': True}
    assert 'normalize' not in FrontEnd(std=std).to_attrs() and 'normalize' not in FrontEnd(std=std, pca=_pca()).to_attrs()
    full = FrontEnd(std=std, pca=_pca(), normalize=True)
    attrs = full.to_attrs()
    assert list(attrs)[0] == 'whiten_std' and list(attrs)[-1] == 'normalize' and attrs['normalize'] is True
    back = FrontEnd.from_attrs(attrs)
    assert back.normalize is True and full.differs(back) is None
    assert FrontEnd.from_attrs(None).normalize is False and FrontEnd.from_attrs({'centers': 0}).normalize is False
    assert FrontEnd.from_attrs({'normalize': True}).normalize is True
    # the widths are those of the stages before it
    assert full.width_out(4) == 2 and FrontEnd(normalize=True).width_out(7) == 7
    FrontEnd(normalize=True).check_width(("audio", "m", "layer_0"), 123)


def test_then_puts_the_normalisation_last():
    from acav100m_amd.clustering.frontend import FrontEnd
    std = np.ones(4, np.float32)
    f = FrontEnd(std=std).then(FrontEnd(pca=_pca())).then(FrontEnd(normalize=True))
    assert f.std is not None and f.pca is not None and f.normalize is True
    assert FrontEnd().then(FrontEnd(normalize=True)).normalize is True
    assert FrontEnd(std=std).then(FrontEnd(normalize=True)).to_attrs().keys() == {'whiten_std', 'normalize'}
    for later in (FrontEnd(std=std), FrontEnd(pca=_pca()), FrontEnd(normalize=True)):
        with pytest.raises(AssertionError, match="normalisation last"):
            FrontEnd(normalize=True).then(later)


def test_differs_names_the_row_normalisation():
    from acav100m_amd.clustering.frontend import FrontEnd
    std = np.ones(4, np.float32)
    assert FrontEnd(normalize=True).differs(FrontEnd()) == 'the row normalisation'
    assert FrontEnd(std=std).differs(FrontEnd(std=std, normalize=True)) == 'the row normalisation'
    assert FrontEnd(std=std, normalize=True).differs(FrontEnd(std=std, normalize=True)) is None
    assert FrontEnd(std=std, normalize=True).differs(FrontEnd(std=2 * std, normalize=True)) == 'whiten_std'


class _FakeKMeans:
    def __init__(self, d, **extra):
        self.d, self.extra = d, extra

    def get_attrs_plain(self):
        return {'count': 320, 'lr': 0.01, 'initial_rounds': 10, 'reinit': (.7, 5.0), 'fallback': 0, 'sequential': False,
                'centers': np.arange(4 * self.d, dtype=np.float32).reshape(4, self.d), 'counts': np.ones(4, np.float32), **self.extra}


V = ("audio", "layer_vggish", "layer_0")


def test_cache_round_trip_keeps_the_key_and_adds_nothing_without(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import cache, run_clustering as rc
    from acav100m_amd.clustering.frontend import FrontEnd
    plain = _args(**{"data.output.path": str(tmp_path / "plain"), "data.path": "shard-{000000..000003}.pkl", "clustering.cached_epoch": 1})
    unit = _args(**{"data.output.path": str(tmp_path / "unit"), "data.path": "shard-{000000..000003}.pkl", "clustering.cached_epoch": 1})
    cache.save(plain, 1, {V: _FakeKMeans(3)})
    cache.save(unit, 1, {V: _FakeKMeans(3)}, {V: FrontEnd(normalize=True)})
    a, b = cache.read(cache.path(plain, 1)), cache.read(cache.path(unit, 1))
    assert set(a[V]) == set(_FakeKMeans(1).get_attrs_plain()) and set(b[V]) == set(a[V]) | {"normalize"} and b[V]["normalize"] is True
    assert FrontEnd.from_attrs(cache.find(b, V)).normalize and not FrontEnd.from_attrs(cache.find(a, V)).normalize
    assert rc.cached_normalization(unit) == (cache.path(unit, 1), {V[1:]})
    assert rc.cached_normalization(unit, normalize=True)[1] == {V[1:]}
    assert rc.cached_normalization(plain) == (cache.path(plain, 1), set())
    with pytest.raises(ValueError, match="cache_epoch_1_"):
        rc.cached_normalization(plain, normalize=True)
    plain.clustering.cached_epoch = None
    assert rc.cached_normalization(plain, normalize=True) == (None, set())  # a fresh run: nothing to contradict


def test_normalize_against_a_plain_cache_is_refused_before_any_shard_is_read(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import cache, run_clustering as rc
    for switch in ({"clustering.normalize": True}, {"clustering.spherical": True, "clustering.algorithm": "lloyd"}):
        args = _args(**{"data.output.path": str(tmp_path / "out"), "data.path": str(tmp_path / "nowhere" / "shard-{000000..000003}.pkl"),
                        "clustering.cached_epoch": 1, **switch})
        cache.save(args, 1, {V: _FakeKMeans(3, **({"algorithm": "lloyd"} if "clustering.algorithm" in switch else {}))})
        with pytest.raises(ValueError, match="holds no 'normalize' key"):
            rc.run_clustering(args)  # the shard paths do not exist: reading one would fail differently


def test_resume_refuses_spherical_against_a_state_that_is_not(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import cache, run_clustering as rc
    from acav100m_amd.clustering.frontend import FrontEnd
    args = _args(**{"data.output.path": str(tmp_path / "out"), "data.path": "shard-{000000..000003}.pkl", "clustering.cached_epoch": 1,
                    "clustering.resume_training": True, "clustering.algorithm": "lloyd", "clustering.spherical": True})
    cache.save(args, 1, {V: _FakeKMeans(3, algorithm="lloyd")}, {V: FrontEnd(normalize=True)})
    with pytest.raises(ValueError, match="not a spherical state"):
        rc.check_cached_algorithm(args)
    cache.save(args, 1, {V: _FakeKMeans(3, algorithm="lloyd", spherical=True)}, {V: FrontEnd(normalize=True)})
    rc.check_cached_algorithm(args)
    args.clustering.spherical = False  # the cache is followed
    rc.check_cached_algorithm(args)


def test_state_carries_spherical_only_when_set():
    from acav100m_amd.clustering import KMeans
    km = KMeans(None, 3, 4)
    assert 'spherical' not in km.get_attrs()
    km.to_lloyd(np.zeros((4, 3), np.float32))
    assert km.get_attrs()['algorithm'] == 'lloyd' and 'spherical' not in km.get_attrs()
    km.to_lloyd(spherical=True)
    dt = km.get_attrs()
    assert dt['algorithm'] == 'lloyd' and dt['spherical'] is True
    assert KMeans.load(dt).spherical is True and KMeans.load({k: v for k, v in dt.items() if k != 'spherical'}).spherical is False


def test_evaluate_refuses_epochs_that_disagree_on_the_normalisation(tmp_path):
    pytest.importorskip("torch")
    from acav100m_amd.clustering import cache
    from acav100m_amd.clustering.evaluate import load_states
    from acav100m_amd.clustering.frontend import FrontEnd
    args = _args(**{"data.output.path": str(tmp_path / "out"), "data.path": "shard-{000000..000003}.pkl", "models": ["layer_vggish"]})
    cache.save(args, 0, {V: _FakeKMeans(3)}, {V: FrontEnd(normalize=True)})
    cache.save(args, 1, {V: _FakeKMeans(3)}, {V: FrontEnd(normalize=True)})
    cache.save(args, 2, {V: _FakeKMeans(3)})
    assert list(load_states(args, [0, 1])) == [0, 1]
    with pytest.raises(ValueError, match="the row normalisation"):
        load_states(args, [0, 2])


# ------------------------------------------------------------------------------------------------------ the C ABI, no device
def test_rows_normalize_refuses_bad_arguments_without_a_device(lib):
    x = np.ones((2, 3), np.float32)
    xp = x.ctypes.data_as(C.c_void_p)
    zero, bad = C.c_int64(-7), C.c_int64(-7)
    z, b = C.byref(zero), C.byref(bad)
    for d in (0, -1, 16385):
        assert lib.acav_rows_normalize(0, xp, 2, d, z, b, None) == -1, d
    for n in (-1, 2 ** 37):
        assert lib.acav_rows_normalize(0, xp, n, 3, z, b, None) == -1, n
    assert lib.acav_rows_normalize(0, None, 2, 3, z, b, None) == -1
    assert lib.acav_rows_normalize(0, xp, 2, 3, None, b, None) == -1
    assert lib.acav_rows_normalize(0, xp, 2, 3, z, None, None) == -1
    assert (x == 1).all() and zero.value == -7 and bad.value == -7  # a refused call writes nothing
    assert lib.acav_rows_normalize(0, None, 0, 3, z, b, None) == 0  # no rows: a no-op that needs no device
    assert zero.value == 0 and bad.value == 0


def _plan(lib, n, d, cus):
    out = (C.c_int64 * 6)(*([-7] * 6))
    assert lib.acav_rows_normalize_plan(n, d, cus, out) == 0, (n, d, cus)
    return tuple(out)


def test_rows_normalize_plan(lib):
    # (n, d, cus) -> (rows of a workgroup, blocks, LDS path, grid, LDS bytes, rows of a round)
    for args, want in [((0, 64, 256), (4, 1, 0, 1, 0, 4)),
                       ((1, 1, 256), (4, 1, 0, 1, 0, 4)),
                       ((1000, 64, 256), (4, 1, 0, 250, 0, 1000)),
                       ((1001, 257, 256), (4, 2, 0, 251, 0, 1004)),
                       ((10 ** 6, 1024, 256), (4, 4, 0, 2048, 0, 8192)),
                       ((262144, 2304, 256), (4, 9, 0, 2048, 0, 8192)),
                       ((100, 4096, 8), (4, 16, 0, 25, 0, 100)),
                       ((100, 4097, 8), (1, 17, 1, 64, 17 * 1024, 64)),
                       ((10 ** 4, 8192, 256), (1, 32, 1, 256 * 5, 32 * 1024, 256 * 5)),
                       ((10 ** 4, 16384, 256), (1, 64, 1, 512, 65536, 512))]:
        assert _plan(lib, *args) == want, args
    assert _plan(lib, 10 ** 6, 1024, 256) == _plan(lib, 10 ** 6, 1024, 256)  # pure
    out = (C.c_int64 * 6)()
    for args in ((-1, 64, 256), (2 ** 37, 64, 256), (100, 0, 256), (100, 16385, 256), (100, 64, 0)):
        assert lib.acav_rows_normalize_plan(*args, out) == -1, args
    assert lib.acav_rows_normalize_plan(100, 64, 256, None) == -1


def test_rows_normalize_plan_covers_n(lib):
    for d, cus in ((1, 256), (64, 256), (1024, 256), (2304, 8), (4096, 256), (4097, 256), (16384, 3)):
        last = 0
        for n in [0, 1, 3, 4, 5, 1000, 8191, 8192, 8193, 10 ** 6, 2 ** 30, 2 ** 37 - 1]:
            wg_rows, blocks, lds, grid, lds_bytes, round_rows = _plan(lib, n, d, cus)
            assert blocks == -(-d // 256) and lds == (blocks > 16) and wg_rows == (1 if lds else 4)
            assert lds_bytes == (blocks * 1024 if lds else 0) and lds_bytes <= 65536
            assert 1 <= grid <= 8 * cus and round_rows == grid * wg_rows
            assert grid * lds_bytes <= cus * 160 * 1024  # what is resident at once fits the LDS of the compute units
            # every row is some workgroup's: row i belongs to workgroup (i // wg_rows) % grid, rounds of round_rows rows
            if lds:
                assert grid == max(n, 1) or grid < n
            else:
                assert grid == max(1, min(-(-n // 4), 8 * cus))
            assert grid >= last  # monotone in n
            last = grid
