"""GPU: `clustering.cli cluster --clustering.algorithm=lloyd --clustering.init=kmeans++` on tiny synthetic shards (two views, 256
rows, K = 8): the caches and the assignment shards are the numpy restatements' (tests/_kmeanspp_np.py seeds fed into the
tests/_lloyd_np.py iteration), streamed row groups and the sample size change no byte where they should not, the seeds are taken
in the whitened space, and init=random is the run without the key."""
import os
import sys

import numpy as np
import pytest

from tests import _kmeanspp_np as P
from tests import _lloyd_np as L
from tests import _whiten_np as R
from tests.test_gpu_whiten_cli import SHARDS, _cache, _features, _labels

pytestmark = pytest.mark.gpu

K, ITERS, N = 8, 4, 256
PLUS = {"clustering.algorithm": "lloyd", "clustering.init": "kmeans++", "clustering.init_trials": "auto",
        "clustering.epochs": ITERS, "clustering.ncentroids": K}


def _restate(order, dims, rows_of, sample=None, trials='auto'):
    """the run's generator: one rand(K, d) per view (the KMeans objects, in view order), one randperm(N) per view, then -- after
    the pass over the rows -- the uniforms of each view in turn -> {view: the Lloyd loop from the restated seeds}"""
    from oracle import oracle as O
    rng = O.Rng(0)
    for v in order:
        rng.rand(K, dims[v])
    M = min(N, sample if sample is not None else 256 * K)
    T = P.trials_for(K, trials)
    picks = {v: np.sort(rng.randperm(N)[:M]) for v in order}
    steps, potentials = {}, {}
    for v in order:
        x = rows_of(v)
        seeds, potentials[v] = P.seed(x[picks[v]], K, T, P.uniforms(rng.u32, 1 + (K - 1) * T))
        steps[v] = L.loop(x, x[picks[v][seeds]], ITERS)
    return steps, potentials


@pytest.fixture(scope="module")
def runs(tmp_path_factory, golden_dir):
    """the shards, the k-means++ run every test looks at and its restatement -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    root = str(tmp_path_factory.mktemp("acav_kmeanspp_cli"))
    glob = synth.write_feature_shards(root, n_shards=4, rows=N // 4, seed=3, comps=8, audio_dims=[24], video_dims=[40])
    dims = {("layer_vggish", "layer_0"): 24, ("layer_slow_fast", "layer_0"): 40}
    raw = _features(os.path.join(root, "features"), dims)
    common = dict(feature_path=glob, meta_path=os.path.join(root, "videos"), **{"computation.num_workers": 0})

    def cluster(out, **more):
        acav100m_amd.manual_seed(0)
        saved = Cli().cluster(out_path=os.path.join(root, out), **common, **more)
        assert len(saved) == 4
        return os.path.join(root, out)

    plus = cluster("plus", **PLUS)
    order = [(mk, layer) for mk, per in _cache(plus, 0).items() for layer in per]
    assert sorted(order) == sorted(dims)
    return dict(root=root, dims=dims, raw=raw, cluster=cluster, plus=plus, order=order)


def _check(out, runs, steps, rows_of):
    labels, names = _labels(out, runs["dims"])
    assert len(names) == N
    epochs = max(len(st) for st in steps.values())  # the loop ends once every view has converged
    assert len(_caches(out)) == epochs
    for v, st in steps.items():
        for e in range(epochs):
            dt = _cache(out, e)[v[0]][v[1]]
            s = st[min(e, len(st) - 1)]  # a view that converged keeps its state
            assert np.asarray(dt["centers"], np.float32).tobytes() == s["centers"].tobytes(), (v, e)
            assert np.array_equal(np.asarray(dt["counts"]), s["sizes"].astype(np.float32)), (v, e)
            assert dt["algorithm"] == "lloyd"
        assert np.array_equal(labels[v], L.nearest(rows_of(v), st[-1]["centers"])), v


def _caches(out):
    return sorted(f for f in os.listdir(out) if f.startswith("cache_epoch_"))


def _same_files(a, b):
    names = _caches(a) + SHARDS
    assert 1 <= len(_caches(a)) <= ITERS and _caches(b) == _caches(a)
    for name in names:
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name


def test_caches_and_shards_are_the_restatements(runs):
    steps, potentials = _restate(runs["order"], runs["dims"], lambda v: runs["raw"][v])
    for v in runs["order"]:
        print(v, "potential", int(potentials[v][0]), "->", int(potentials[v][-1]), "changed", [s["changed"] for s in steps[v]])
    _check(runs["plus"], runs, steps, lambda v: runs["raw"][v])


def test_streamed_row_groups_change_no_byte(runs):
    shard_bytes = (N // 4) * 4 * sum(runs["dims"].values())
    out = runs["cluster"]("plus_groups", **PLUS, **{"data.resident_bytes": int(1.5 * shard_bytes)})
    _same_files(runs["plus"], out)


def test_a_sample_of_all_rows_is_the_default_here_and_a_smaller_one_is_restated(runs):
    out = runs["cluster"]("plus_all", **PLUS, **{"clustering.init_sample": N})  # 256 K > N: the default sample is every row
    _same_files(runs["plus"], out)
    small = runs["cluster"]("plus_small", **PLUS, **{"clustering.init_sample": 100})
    steps, _pot = _restate(runs["order"], runs["dims"], lambda v: runs["raw"][v], sample=100)
    _check(small, runs, steps, lambda v: runs["raw"][v])


def test_seeds_are_taken_in_the_whitened_space(runs):
    out = runs["cluster"]("plus_white", **PLUS, **{"clustering.whiten": True})
    nested = _cache(out, 0)
    white = {}
    for v, x in runs["raw"].items():
        std = np.asarray(nested[v[0]][v[1]]["whiten_std"], np.float32)
        want, zero = R.std_of(x)
        assert int(R.ulp_diff(std, want).max()) <= 1 and zero == 0
        white[v] = (x / std).astype(np.float32)
    steps, _pot = _restate(runs["order"], runs["dims"], lambda v: white[v])
    _check(out, runs, steps, lambda v: white[v])


def test_init_random_is_the_run_without_the_key_and_kmeanspp_is_not(runs):
    lloyd = {"clustering.algorithm": "lloyd", "clustering.epochs": ITERS, "clustering.ncentroids": K}
    a = runs["cluster"]("lloyd_plain", **lloyd)
    b = runs["cluster"]("lloyd_random", **lloyd, **{"clustering.init": "random", "clustering.init_trials": "auto"})
    _same_files(a, b)
    c0 = _cache(a, 0)
    p0 = _cache(runs["plus"], 0)
    assert any(np.asarray(c0[mk][layer]["centers"]).tobytes() != np.asarray(p0[mk][layer]["centers"]).tobytes() for mk, layer in runs["dims"])
    for mk, layer in runs["dims"]:
        assert set(c0[mk][layer]) == set(p0[mk][layer])  # the cache files keep their format


@pytest.mark.parametrize("over,words", [
    ({"clustering.init": "kmeans++"}, "needs clustering.algorithm=lloyd"),
    ({"clustering.algorithm": "lloyd", "clustering.init": "furthest"}, "clustering.init must be 'random' or 'kmeans"),
    ({"clustering.algorithm": "lloyd", "clustering.init": "kmeans++", "clustering.init_trials": 17}, "clustering.init_trials must be"),
    ({"clustering.algorithm": "lloyd", "clustering.init": "kmeans++", "clustering.ncentroids": K, "clustering.init_sample": K - 1},
     "clustering.init_sample=7 must be"),
])
def test_refusals(runs, over, words):
    with pytest.raises(ValueError) as err:
        runs["cluster"]("refused", **over)
    assert words in str(err.value)
    refused = os.path.join(runs["root"], "refused")  # refused before anything is trained or written
    assert not os.path.isdir(refused) or not [f for f in os.listdir(refused) if f.startswith("cache_epoch_")]
