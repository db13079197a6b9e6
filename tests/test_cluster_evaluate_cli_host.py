"""CPU: the refusals of `clustering.cli evaluate` come before any shard is read and before the device is touched, and the
command line accepts a list of epochs."""
import numpy as np
import pytest


@pytest.fixture
def no_shard_reads(monkeypatch):
    """every way into the shard files raises"""
    from acav100m_amd import shards as io

    def reached(*a, **kw):
        raise AssertionError("a shard was read before the refusal")
    for name in ("load_feature_shards", "load_pickle", "shard_sizes_from_meta"):
        monkeypatch.setattr(io, name, reached)
    from acav100m_amd.clustering import sgd_clustering

    def on_device(self, device):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(sgd_clustering.KMeans, "to", on_device)


def _write_cache(out, epoch, name, views, count, k=4, d=3):
    import torch
    nested = {}
    for mk, layer in views:
        nested.setdefault(mk, {})[layer] = {
            'args': None, 'count': count, 'lr': 1e-2, 'initial_rounds': 10, 'reinit': (.7, 5.0), 'fallback': 0,
            'sequential': False, 'centers': np.zeros((k, d), np.float32), 'counts': np.ones(k, np.float32), '_kind': 'audio'}
    out.mkdir(parents=True, exist_ok=True)
    torch.save(nested, str(out / "cache_epoch_{}_{}".format(epoch, name)))


def _evaluate(tmp_path, **extra):
    from acav100m_amd.clustering.cli import Cli
    kw = {"feature_path": str(tmp_path / "features" / "shard-{000000..000001}.pkl"), "meta_path": str(tmp_path / "videos"),
          "out_path": str(tmp_path / "clusters"), "computation.num_gpus": 1, "models": ["layer_vggish", "layer_slow_fast"]}
    kw.update(extra)
    return Cli().evaluate(**kw)


NAME = "shard-{000000..000001}.pkl"
BOTH = [("layer_vggish", "layer_0"), ("layer_slow_fast", "layer_0")]


def test_refuses_without_cached_epoch(tmp_path, no_shard_reads):
    with pytest.raises(ValueError, match=r"evaluate needs --clustering\.cached_epoch"):
        _evaluate(tmp_path)
    with pytest.raises(ValueError, match="an epoch or a list of epochs"):
        _evaluate(tmp_path, **{"clustering.cached_epoch": "last"})


def test_refuses_a_missing_cache(tmp_path, no_shard_reads):
    _write_cache(tmp_path / "clusters", 0, NAME, BOTH, count=1000)
    with pytest.raises(FileNotFoundError, match="no clustering cache of epoch 1"):
        _evaluate(tmp_path, **{"clustering.cached_epoch": [0, 1]})


def test_refuses_a_cache_that_lacks_a_view(tmp_path, no_shard_reads):
    _write_cache(tmp_path / "clusters", 0, NAME, BOTH[:1], count=1000)
    with pytest.raises(ValueError, match="lacks a view of model 'layer_slow_fast'"):
        _evaluate(tmp_path, **{"clustering.cached_epoch": 0})


def test_refuses_a_state_in_warm_up(tmp_path, no_shard_reads):
    _write_cache(tmp_path / "clusters", 0, NAME, BOTH, count=39)  # K = 4: the warm-up lasts until count = 40
    with pytest.raises(ValueError, match=r"warm-up, count = 39 < 10\*K = 40"):
        _evaluate(tmp_path, **{"clustering.cached_epoch": 0})


def test_writes_nothing_when_it_refuses(tmp_path, no_shard_reads):
    _write_cache(tmp_path / "clusters", 0, NAME, BOTH, count=39)
    before = sorted(p.name for p in (tmp_path / "clusters").iterdir())
    with pytest.raises(ValueError):
        _evaluate(tmp_path, **{"clustering.cached_epoch": 0, "evaluate.out_path": str(tmp_path / "clusters" / "quality.json"),
                               "evaluate.rows_path": str(tmp_path / "rows")})
    assert sorted(p.name for p in (tmp_path / "clusters").iterdir()) == before and not (tmp_path / "rows").exists()


def test_command_line_accepts_a_list_of_epochs():
    from acav100m_amd.config import parse_cli
    command, kwargs = parse_cli(["evaluate", "--feature_path=f/shard-{000000..000003}.pkl", "--out_path=clusters",
                                 "--clustering.cached_epoch=[0,1]", "--evaluate.out_path=quality.json"])
    assert command == "evaluate" and kwargs["clustering.cached_epoch"] == [0, 1] and kwargs["evaluate.out_path"] == "quality.json"
    assert parse_cli(["evaluate", "--clustering.cached_epoch=3"])[1]["clustering.cached_epoch"] == 3
    from acav100m_amd.clustering.evaluate import _epochs
    assert _epochs([0, 1]) == [0, 1] and _epochs(3) == [3]
    from acav100m_amd.clustering.cli import Cli
    assert callable(Cli().evaluate)
