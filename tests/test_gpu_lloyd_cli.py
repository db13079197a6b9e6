"""GPU: `clustering.cli cluster --clustering.algorithm=lloyd` on the synthetic shards of tests/golden/synth.py: the caches and
the assignment shards are the numpy restatement's (tests/_lloyd_np.py), row groups change no byte, a cached epoch reproduces the
shards, `evaluate` finds every row at its nearest centre and an inertia that does not rise, the front-ends compose with it, and
a run without the key keeps today's cache keys."""
import os
import shutil
import sys

import numpy as np
import pytest

from tests import _lloyd_np as L
from tests.test_gpu_whiten_cli import SHARDS, _cache, _features, _labels

pytestmark = pytest.mark.gpu

K, ITERS = 32, 4


@pytest.fixture(scope="module")
def runs(tmp_path_factory, golden_dir):
    """the shards, the Lloyd run every test looks at and its restatement -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    from oracle import oracle as O
    root = str(tmp_path_factory.mktemp("acav_lloyd_cli"))
    glob = synth.write_feature_shards(root, n_shards=4, rows=256, seed=0)
    dims = {("layer_vggish", "layer_%d" % i): d for i, d in enumerate(synth.AUDIO_DIMS)}
    dims.update({("layer_slow_fast", "layer_%d" % i): d for i, d in enumerate(synth.VIDEO_DIMS)})
    raw = _features(os.path.join(root, "features"), dims)
    common = dict(feature_path=glob, meta_path=os.path.join(root, "videos"), **{"computation.num_workers": 0})

    def cluster(out, **more):
        acav100m_amd.manual_seed(0)
        saved = Cli().cluster(out_path=out, **common, **more)
        assert len(saved) == 4
        return out

    lloyd = cluster(os.path.join(root, "lloyd"), **{"clustering.algorithm": "lloyd", "clustering.epochs": ITERS})
    # the restatement.  The generator: one torch.rand(K, d) per view when the KMeans objects are created (in view order), then one
    # randperm(N) per view, in view order
    order = [(mk, layer) for mk, per in _cache(lloyd, 0).items() for layer in per]
    assert sorted(order) == sorted(dims)
    rng = O.Rng(0)
    for v in order:
        rng.rand(K, dims[v])
    steps = {}
    for v in order:
        perm = rng.randperm(1024)[:K]
        steps[v] = L.loop(raw[v], raw[v][perm], ITERS)
    return dict(root=root, glob=glob, dims=dims, raw=raw, common=common, cluster=cluster, lloyd=lloyd, steps=steps)


def test_caches_and_shards_are_the_restatements(runs):
    files = sorted(f for f in os.listdir(runs["lloyd"]) if f.startswith("cache_epoch_"))
    assert [f.split("_")[2] for f in files] == ["0", "1", "2", "3"]
    labels, names = _labels(runs["lloyd"], runs["dims"])
    assert len(names) == 1024
    for v, steps in runs["steps"].items():
        print(v, "changed:", [st["changed"] for st in steps], "splits:", [st["splits"] for st in steps])
        for e in range(ITERS):
            dt = _cache(runs["lloyd"], e)[v[0]][v[1]]
            st = steps[min(e, len(steps) - 1)]  # a view that converged keeps its state
            assert np.asarray(dt["centers"], np.float32).tobytes() == st["centers"].tobytes(), (v, e)
            assert np.array_equal(np.asarray(dt["counts"]), st["sizes"].astype(np.float32)), (v, e)
            assert dt["count"] == 1024 * min(e + 1, len(steps)) and dt["fallback"] == 0
            assert dt["algorithm"] == "lloyd" and dt["initial_rounds"] == 0 and tuple(dt["reinit"]) == (.7, 1.0)
        assert np.array_equal(labels[v], L.nearest(runs["raw"][v], steps[-1]["centers"])), v


def test_row_groups_change_no_byte(runs):
    shard_bytes = 256 * 4 * sum(runs["dims"].values())
    out = runs["cluster"](os.path.join(runs["root"], "lloyd_groups"),
                          **{"clustering.algorithm": "lloyd", "clustering.epochs": ITERS, "data.resident_bytes": int(2.5 * shard_bytes)})
    names = sorted(f for f in os.listdir(runs["lloyd"]) if f.startswith("cache_epoch_")) + SHARDS
    assert len(names) == ITERS + 4
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(runs["lloyd"], name), "rb").read(), name


def test_a_cached_epoch_reproduces_the_shards(runs, tmp_path):
    out = str(tmp_path / "lloyd_copy")
    shutil.copytree(runs["lloyd"], out)
    for name in SHARDS:
        os.remove(os.path.join(out, name))
    runs["cluster"](out, **{"clustering.cached_epoch": ITERS - 1})  # no algorithm key: the cache says how its rows are labelled
    for name in SHARDS:
        assert open(os.path.join(out, "epoch_%d_" % (ITERS - 1) + name), "rb").read() == open(os.path.join(runs["lloyd"], name), "rb").read()


def test_evaluate_finds_no_displaced_row_and_a_falling_inertia(runs):
    from acav100m_amd.clustering.cli import Cli
    report = Cli().evaluate(out_path=runs["lloyd"], **runs["common"], **{"clustering.cached_epoch": list(range(ITERS))})
    eps = float(np.finfo(np.float32).eps)
    for v, steps in runs["steps"].items():
        per_epoch = report["views"][v[0] + "/" + v[1]]
        near = [per_epoch[str(e)]["nearest_inertia"] for e in range(ITERS)]
        print(v, near)
        for e in range(ITERS):
            assert per_epoch[str(e)]["displaced"] == 0, (v, e)
        if any(st["splits"] for st in steps):
            continue  # a split moves two centres off their means on purpose
        # With J(l, c) the inertia of labels l at centres c:  nearest(c') <= J(l, c') = J(l, mean_l) + sum_k n_k |c'_k - mean_k|^2 / N
        # and J(l, mean_l) <= J(l, c) = nearest(c), the last step because no row is displaced.  What is left is the fp32 rounding
        # of the new centres, c' = fp32(mean): second order, (eps / 2)^2 |c|^2, plus the evaluation's own float64 rounding of
        # (|x|^2 + |c|^2) -- both below eps * inertia while the squared norms stay below 10^5 inertias, as they do on these rows.
        for a, b in zip(near, near[1:]):
            assert b <= a + eps * a, v


def test_front_ends_compose(runs):
    out = runs["cluster"](os.path.join(runs["root"], "lloyd_white_pca"),
                          **{"clustering.algorithm": "lloyd", "clustering.epochs": 2, "clustering.whiten": True, "clustering.pca_dim": 8})
    nested = _cache(out, 1)
    for (mk, layer), d in runs["dims"].items():
        dt = nested[mk][layer]
        assert dt["algorithm"] == "lloyd" and dt["whiten_std"].shape == (d,)
        assert dt["pca_components"].shape == (8, d) and dt["pca_mean"].shape == (d,) and dt["pca_explained_variance"].shape == (8,)
        assert np.asarray(dt["centers"]).shape == (K, 8) and np.isfinite(np.asarray(dt["centers"])).all()
        assert int(np.asarray(dt["counts"]).sum()) == 1024
    assert all(os.path.isfile(os.path.join(out, name)) for name in SHARDS)


def test_a_run_without_the_key_keeps_its_cache_keys(runs):
    out = runs["cluster"](os.path.join(runs["root"], "plain"))
    for e in (0, 1):
        for mk, per in _cache(out, e).items():
            for layer, dt in per.items():
                assert "algorithm" not in dt and dt["initial_rounds"] == 10 and tuple(dt["reinit"]) == (.7, 5.0)
                assert set(dt) == {"args", "count", "lr", "initial_rounds", "reinit", "fallback", "sequential", "centers", "counts", "_kind"}
    lp, _ = _labels(out, runs["dims"])
    ll, _ = _labels(runs["lloyd"], runs["dims"])
    assert any(not np.array_equal(lp[v], ll[v]) for v in runs["dims"])  # the key does something
