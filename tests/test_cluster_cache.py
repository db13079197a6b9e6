"""CPU: the clustering cache module (acav100m_amd/clustering/cache.py) as its callers see it -- a reference-written file, which
names no modality, is resolved to the same attrs by every reader; a subset cache is located once, the same way for `cluster` and
`evaluate`; and a cached `cluster` run reads its file once.  No device: the KMeans class and the row groups are stand-ins."""
import re
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

VIEWS = [("audio", "layer_vggish", "layer_0"), ("video", "layer_slow_fast", "layer_0")]
DIMS = OrderedDict(zip(VIEWS, (5, 7)))
P = 2  # columns after the projection
FRONT_KEYS = ('whiten_std', 'pca_mean', 'pca_components', 'pca_explained_variance', 'pca_total_variance')


def _args(**over):
    from acav100m_amd.config import CLUSTERING_DEFAULTS, merge
    return merge(CLUSTERING_DEFAULTS, over)


class _FakeKMeans:
    """what KMeans.load is handed, kept"""
    loaded = []

    def __init__(self, d):
        self.d = d

    def get_attrs_plain(self):
        return {'count': 320, 'lr': 0.01, 'initial_rounds': 10, 'reinit': (.7, 5.0), 'fallback': 0, 'sequential': False,
                'centers': np.arange(4 * self.d, dtype=np.float32).reshape(4, self.d), 'counts': np.ones(4, np.float32)}

    @classmethod
    def load(cls, attrs):
        cls.loaded.append(attrs)
        return cls(attrs['centers'].shape[1])


def _front(d, seed):
    rs = np.random.RandomState(seed)
    return {'whiten_std': (1 + rs.rand(d)).astype(np.float32), 'pca_mean': rs.randn(d).astype(np.float32),
            'pca_components': rs.randn(P, d).astype(np.float32), 'pca_explained_variance': np.sort(rs.rand(P))[::-1].copy(),
            'pca_total_variance': np.float64(P + rs.rand())}


def _write_reference_cache(args, epoch):
    """{model_key: {layer: attrs}} without '_kind', the front-end keys as tensors: the file the reference's classes would write"""
    from acav100m_amd.clustering import cache
    nested = OrderedDict()
    for i, (_kind, mk, layer) in enumerate(VIEWS):
        dt = _FakeKMeans(P).get_attrs_plain()
        dt.update({k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in _front(DIMS[VIEWS[i]], i).items()})
        nested.setdefault(mk, OrderedDict())[layer] = dt
    file = cache.path(args, epoch)
    file.parent.mkdir(parents=True, exist_ok=True)
    torch.save(nested, str(file))
    return file


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert type(a[k]) is type(b[k]) and a[k] == b[k], k


def _count_reads(monkeypatch):
    from acav100m_amd.clustering import cache
    reads, orig = [], cache.read
    monkeypatch.setattr(cache, "read", lambda file: reads.append(file) or orig(file))
    return reads


def _stand_ins(monkeypatch, rc):
    """run_clustering() up to the assign sweep without a shard or a device -> what the sweep would have been handed"""
    seen = []

    class Groups:
        fronts = {}

        def add_front_ends(self, stage):
            self.fronts = dict(stage)
    probe = SimpleNamespace(views=OrderedDict((v, np.zeros((4, d), np.float32)) for v, d in DIMS.items()))
    monkeypatch.setattr(rc.io, "shard_sizes_from_meta", lambda paths, *a, **kw: {p.stem: 4 for p in paths})
    monkeypatch.setattr(rc, "probe_shards", lambda args, paths: (probe, DIMS))
    monkeypatch.setattr(rc, "open_row_groups", lambda *a: Groups())
    monkeypatch.setattr(rc, "KMeans", _FakeKMeans)
    monkeypatch.setattr(rc, "_to_device", lambda args, cl: cl)
    monkeypatch.setattr(rc, "assign_clusters", lambda args, groups, cl, mine: seen.append((groups, cl)) or [])
    monkeypatch.setattr(_FakeKMeans, "loaded", [])
    return seen


def test_a_reference_written_cache_resolves_to_the_same_attrs_everywhere_and_is_read_once(tmp_path, monkeypatch):
    from acav100m_amd.clustering import cache, run_clustering as rc
    from acav100m_amd.clustering.evaluate import load_states
    args = _args(**{"data.output.path": str(tmp_path / "out"), "data.path": str(tmp_path / "features" / "shard-{000000..000001}.pkl"),
                    "clustering.cached_epoch": 1, "clustering.pca_dim": P})
    file = _write_reference_cache(args, 1)
    saved = cache.read(file)
    assert list(saved) == [(None,) + v[1:] for v in VIEWS]  # no modality in the file
    want = [cache.find(saved, v) for v in VIEWS]
    for i, v in enumerate(VIEWS):  # the dtypes of the cache, whatever the file held
        assert want[i] is saved[(None,) + v[1:]]
        _same({k: want[i][k] for k in FRONT_KEYS}, _front(DIMS[v], i))
    assert cache.find(saved, ("audio", "layer_vggish", "layer_1")) is None

    # the cluster run: one read, and its loader is handed the attrs above, in view order
    reads = _count_reads(monkeypatch)
    seen = _stand_ins(monkeypatch, rc)
    assert rc.run_clustering(args) == []
    assert reads == [file]
    assert len(_FakeKMeans.loaded) == len(VIEWS)
    for got, w in zip(_FakeKMeans.loaded, want):
        _same(got, w)
    (groups, cl), = seen
    assert list(cl) == VIEWS and list(groups.fronts) == VIEWS
    for v, w in zip(VIEWS, want):  # and the rows would go through the cache's front-end
        _same(groups.fronts[v].to_attrs(), {k: w[k] for k in FRONT_KEYS})

    # the two summaries of a cached run and evaluate's reader
    path, stds = rc.cached_whitening(args)
    assert path == file and list(stds) == [v[1:] for v in VIEWS]
    path, fits = rc.cached_projection(args)
    assert path == file and list(fits) == [v[1:] for v in VIEWS]
    states = load_states(args, [1])
    for v, w in zip(VIEWS, want):
        assert stds[v[1:]].tobytes() == w['whiten_std'].tobytes()
        _same({'pca_' + k: x for k, x in fits[v[1:]].items()}, {k: w[k] for k in rc.PCA_KEYS})
        _same(cache.find(states[1], v), w)


def test_cluster_and_evaluate_locate_the_same_subset_cache(tmp_path, monkeypatch):
    from acav100m_amd.clustering import cache, run_clustering as rc
    from acav100m_amd.clustering.evaluate import load_states
    common = {"data.output.path": str(tmp_path / "out"), "clustering.cached_epoch": 1, "models": ["layer_vggish"]}
    args = _args(**{"data.path": "shard-{000000..000003}.pkl"}, **common)
    for name in ("shard-{000000..000001}.pkl", "shard-{000000..000002}.pkl", "shard-{000002..000005}.pkl"):  # 2 of them, 3, not a subset
        cache.save(_args(**{"data.path": name}, **common), 1, {VIEWS[0]: _FakeKMeans(3)})
    assert args.clustering.load_cache_from_shard_subset is True  # the default
    exact, want = cache.path(args, 1), tmp_path / "out" / "cache_epoch_1_shard-{000000..000002}.pkl"
    assert not exact.exists() and cache.locate(args, 1) == want  # the largest subset
    reads = _count_reads(monkeypatch)
    assert rc._cached_attrs(args)[0] == want and rc.cached_whitening(args) == (want, {})
    assert list(load_states(args, [1])) == [1]
    assert reads == [want] * 3
    # without the switch there is only the exact file, for both
    args.clustering.load_cache_from_shard_subset = False
    assert cache.locate(args, 1) == exact and rc._cached_attrs(args) == (None, None)
    with pytest.raises(FileNotFoundError, match=re.escape("{} does not exist".format(exact))):
        load_states(args, [1])
    # and the exact file wins over any subset
    args.clustering.load_cache_from_shard_subset = True
    cache.save(args, 1, {VIEWS[0]: _FakeKMeans(3)})
    assert cache.locate(args, 1) == exact
