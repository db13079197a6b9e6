"""CPU: the launch shape of acav_rows_silhouette (acav_rows_silhouette_plan, the function the entry point launches from) for a
few (m, d, k, cus), its refusals, and `evaluate`'s refusal of a sample that is no integer of at least 2 -- before any cache or
shard is read and before the device is touched."""
import ctypes as C

import pytest

LEN = 9  # ACAV_SILHOUETTE_PLAN_LEN


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _plan(lib, m, d, k, cus):
    out = (C.c_int64 * LEN)(*([-7] * LEN))
    assert lib.acav_rows_silhouette_plan(m, d, k, cus, out) == 0, (m, d, k, cus)
    return tuple(out)


def test_plan_table(lib):
    small = 64 * 65 * 8 + 2 * 64 * 4     # the 64-row distance tile (it lies over the stages) + the block's run ids and sizes
    large = 128 * 65 * 8 + 2 * 64 * 4
    per_row = 3 * 4 + 2 * 4 + 8 + 2 * 8  # positions, runs, sizes | query positions, output rows | norm | (A, B)
    # (query rows of a tile, columns of a block, columns of a stage, tiles = workgroups, blocks, stages, accumulators, LDS, scratch)
    for args, want in [((65, 88, 33, 256), (64, 64, 32, 2, 2, 3, 4, small, 65 * per_row)),
                       ((600, 128, 2, 256), (64, 64, 32, 10, 10, 4, 4, small, 600 * per_row)),
                       ((32640, 128, 256, 256), (64, 64, 32, 510, 510, 4, 4, small, 32640 * per_row)),   # 255 tiles of 128 < 256 CUs
                       ((32641, 128, 256, 256), (128, 64, 32, 256, 511, 4, 8, large, 32641 * per_row)),  # 256 of them: the larger tile
                       ((32768, 1024, 1024, 256), (128, 64, 32, 256, 512, 32, 8, large, 32768 * per_row)),
                       ((8192, 2304, 2, 8), (128, 64, 32, 64, 128, 72, 8, large, 8192 * per_row)),
                       ((8192, 2304, 2, 304), (64, 64, 32, 128, 128, 72, 4, small, 8192 * per_row)),
                       ((2, 1, 1, 1), (128, 64, 32, 1, 1, 1, 8, large, 2 * per_row))]:
        assert _plan(lib, *args) == want, args
    assert 2 * large <= 160 * 1024  # two workgroups share a compute unit's LDS


def test_plan_does_not_depend_on_k(lib):
    for m, d, cus in ((65, 88, 256), (40000, 128, 256)):
        assert len({_plan(lib, m, d, k, cus) for k in (1, 2, 1024, 2 ** 31 - 1)}) == 1  # no per-cluster table: k is not limited


def test_plan_refusals(lib):
    out = (C.c_int64 * LEN)()
    for args in ((1, 64, 4, 256), (0, 64, 4, 256), (-5, 64, 4, 256), (2 ** 31, 64, 4, 256), (100, 0, 4, 256), (100, 16385, 4, 256),
                 (100, 64, 0, 256), (100, 64, -1, 256), (100, 64, 4, 0)):
        assert lib.acav_rows_silhouette_plan(*args, out) == -1, args
    assert lib.acav_rows_silhouette_plan(100, 64, 4, 256, None) == -1


def test_entry_refuses_sizes_before_the_device(lib):
    """m < 2, d < 1, k < 1 and NULL pointers are ACAV_EINVAL with row_stats untouched: checked before any device call"""
    import numpy as np
    x, lab = np.zeros((4, 3), np.float32), np.zeros(4, np.int64)
    stats = np.full((4, 2), -3.0)
    px, pl, ps = (a.ctypes.data_as(C.c_void_p) for a in (x, lab, stats))
    for args in ((px, 1, 3, pl, 2, ps), (px, 4, 0, pl, 2, ps), (px, 4, 3, pl, 0, ps), (None, 4, 3, pl, 2, ps), (px, 4, 3, None, 2, ps),
                 (px, 4, 3, pl, 2, None), (px, 2 ** 31, 3, pl, 2, ps)):
        assert lib.acav_rows_silhouette(0, *args, None) == -1, args[1:]
    for q0, q1 in ((2, 2), (3, 1), (-1, 2), (0, 5)):
        assert lib.acav_rows_silhouette_range(0, px, 4, 3, pl, 2, q0, q1, ps, None) == -1, (q0, q1)
    assert (stats == -3.0).all()


@pytest.fixture
def no_reads(monkeypatch):
    """every way to the caches, the shards and the device raises"""
    from acav100m_amd import shards as io
    from acav100m_amd.clustering import cache, sgd_clustering

    def reached(*a, **kw):
        raise AssertionError("evaluate went on past the refusal")
    for name in ("load_feature_shards", "load_pickle", "shard_sizes_from_meta"):
        monkeypatch.setattr(io, name, reached)
    monkeypatch.setattr(cache, "read", reached)
    monkeypatch.setattr(sgd_clustering.KMeans, "to", reached)


@pytest.mark.parametrize("value", [1, 0, -4, 2.5, "many", True])
def test_evaluate_refuses_a_bad_sample_size(tmp_path, no_reads, value):
    from acav100m_amd.clustering.cli import Cli
    with pytest.raises(ValueError, match=r"evaluate\.silhouette_sample must be an integer of at least 2"):
        Cli().evaluate(feature_path=str(tmp_path / "features" / "shard-{000000..000001}.pkl"), meta_path=str(tmp_path / "videos"),
                       out_path=str(tmp_path / "clusters"), **{"clustering.cached_epoch": 0, "evaluate.silhouette_sample": value})


def test_evaluate_refuses_a_bad_seed(tmp_path, no_reads):
    from acav100m_amd.clustering.cli import Cli
    with pytest.raises(ValueError, match=r"evaluate\.silhouette_seed must be an integer in \[0, 2\^32\)"):
        Cli().evaluate(feature_path=str(tmp_path / "features" / "shard-{000000..000001}.pkl"), meta_path=str(tmp_path / "videos"),
                       out_path=str(tmp_path / "clusters"),
                       **{"clustering.cached_epoch": 0, "evaluate.silhouette_sample": 64, "evaluate.silhouette_seed": -1})


def test_options_default_to_off():
    from acav100m_amd.clustering.silhouette import check_options
    assert check_options({}) == (None, 0)
    assert check_options({"silhouette_sample": 4096}) == (4096, 0)
    assert check_options({"silhouette_sample": 2, "silhouette_seed": 7}) == (2, 7)
