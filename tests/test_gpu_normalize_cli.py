"""GPU: `clustering.cli cluster --clustering.normalize=True` and `--clustering.spherical=True` on the synthetic shards of
tests/golden/synth.py with every row of every view rescaled by a seeded factor in [1e-3, 1e3]: the SGD run equals the plain run on
shards that hold the restatement's normalised rows (tests/_rownorm_np.py; the path every other test pins), differs from the plain
run on the raw shards, does not depend on the row groups; the spherical Lloyd run is the restatement's; cached runs follow the
cache; and `evaluate` judges in the normalised space."""
import os
import pickle
import shutil
import sys

import numpy as np
import pytest

from tests import _lloyd_np as L
from tests import _rownorm_np as R
from tests.test_gpu_whiten_cli import SHARDS, _cache, _features, _kind, _labels

pytestmark = pytest.mark.gpu

K, ITERS = 32, 3
SPHERICAL = {"clustering.algorithm": "lloyd", "clustering.spherical": True, "clustering.epochs": ITERS}


def _rewrite_rows(src_dir, dst_dir, fn):
    """every shard pkl of src_dir with feature arrays fn((model_key, layer), global row, array) -> dst_dir"""
    os.makedirs(dst_dir, exist_ok=True)
    i = 0
    for name in SHARDS:
        rows = pickle.load(open(os.path.join(src_dir, name), "rb"))
        for r in rows:
            for kind, mk in (("audio", "layer_vggish"), ("video", "layer_slow_fast")):
                arr = r[kind + "_features"][0]["array"]
                for layer in arr:
                    arr[layer] = fn((mk, layer), i, arr[layer])
            i += 1
        with open(os.path.join(dst_dir, name), "wb") as f:
            pickle.dump(rows, f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, golden_dir):
    """the shard sets and the cluster runs every test looks at -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    root = str(tmp_path_factory.mktemp("acav_normalize_cli"))
    glob = synth.write_feature_shards(root, n_shards=4, rows=256, seed=0)
    feat = os.path.join(root, "features")
    dims = {("layer_vggish", "layer_%d" % i): d for i, d in enumerate(synth.AUDIO_DIMS)}
    dims.update({("layer_slow_fast", "layer_%d" % i): d for i, d in enumerate(synth.VIDEO_DIMS)})
    rs = np.random.RandomState(4321)
    scale = {v: np.exp(rs.uniform(np.log(1e-3), np.log(1e3), 1024)).astype(np.float32) for v in sorted(dims)}
    _rewrite_rows(feat, feat, lambda v, i, a: (np.asarray(a, np.float32) * scale[v][i]).astype(np.float32))
    raw = _features(feat, dims)
    unit = {v: R.normalize(x)[0] for v, x in raw.items()}
    # a second shard set that holds the normalised rows: the plain run on it is the path the other tests pin
    feat2 = os.path.join(root, "features_unit")
    _rewrite_rows(feat, feat2, lambda v, i, a: unit[v][i])
    assert all(_features(feat2, dims)[v].tobytes() == unit[v].tobytes() for v in dims)
    common = dict(meta_path=os.path.join(root, "videos"), **{"computation.num_workers": 0})

    def cluster(glob_, out, **more):
        acav100m_amd.manual_seed(0)
        saved = Cli().cluster(feature_path=glob_, out_path=out, **common, **more)
        assert len(saved) == 4
        return out

    norm = cluster(glob, os.path.join(root, "norm"), **{"clustering.normalize": True})
    divided = cluster(os.path.join(feat2, os.path.basename(glob)), os.path.join(root, "divided"))
    plain = cluster(glob, os.path.join(root, "plain"))
    sph = cluster(glob, os.path.join(root, "sph"), **SPHERICAL)
    return dict(root=root, glob=glob, dims=dims, raw=raw, unit=unit, common=common, cluster=cluster, norm=norm, divided=divided,
                plain=plain, sph=sph)


def test_normalized_sgd_run_is_the_plain_run_on_normalised_shards(runs):
    dims = runs["dims"]
    for name in SHARDS:
        assert open(os.path.join(runs["norm"], name), "rb").read() == open(os.path.join(runs["divided"], name), "rb").read(), name
    for epoch in (0, 1):
        cn, cd = _cache(runs["norm"], epoch), _cache(runs["divided"], epoch)
        for (mk, layer) in dims:
            a, b = cn[mk][layer], cd[mk][layer]
            for key in ("centers", "counts"):
                assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (mk, layer, key)
            assert a["count"] == b["count"] and a["fallback"] == b["fallback"]
            assert set(a) == set(b) | {"normalize"} and a["normalize"] is True  # the other run's cache keeps today's keys
            assert "algorithm" not in a and "spherical" not in a


def test_the_switch_does_something(runs):
    ln, _ = _labels(runs["norm"], runs["dims"])
    lp, _ = _labels(runs["plain"], runs["dims"])
    differ = [v for v in runs["dims"] if not np.array_equal(ln[v], lp[v])]
    print("views whose labels differ:", len(differ))
    assert differ
    for e in (0, 1):
        assert all("normalize" not in _cache(runs["plain"], e)[mk][layer] for (mk, layer) in runs["dims"])


def test_row_groups_change_nothing(runs):
    shard_bytes = 256 * 4 * sum(runs["dims"].values())
    out = runs["cluster"](runs["glob"], os.path.join(runs["root"], "norm_groups"),
                          **{"clustering.normalize": True, "data.resident_bytes": int(2.5 * shard_bytes)})
    names = sorted(f for f in os.listdir(runs["norm"]) if f.startswith("cache_epoch_")) + SHARDS
    assert len(names) == 2 + 4
    for name in names:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(runs["norm"], name), "rb").read(), name


@pytest.fixture(scope="module")
def steps(runs):
    """the restatement of the spherical run.  The generator: one torch.rand(K, d) per view when the KMeans objects are created
    (in view order), then one randperm(N) per view, in view order"""
    from oracle import oracle as O
    order = [(mk, layer) for mk, per in _cache(runs["sph"], 0).items() for layer in per]
    assert sorted(order) == sorted(runs["dims"])
    rng = O.Rng(0)
    for v in order:
        rng.rand(K, runs["dims"][v])
    out = {}
    for v in order:
        perm = rng.randperm(1024)[:K]
        out[v] = R.spherical_loop(runs["unit"][v], runs["unit"][v][perm], ITERS)
    return out


def test_spherical_lloyd_run_is_the_restatement(runs, steps):
    labels, names = _labels(runs["sph"], runs["dims"])
    assert len(names) == 1024
    for v, sts in steps.items():
        print(v, "changed:", [st["changed"] for st in sts], "splits:", [st["splits"] for st in sts])
        for e in range(ITERS):
            dt = _cache(runs["sph"], e)[v[0]][v[1]]
            st = sts[min(e, len(sts) - 1)]  # a view that converged keeps its state
            assert np.asarray(dt["centers"], np.float32).tobytes() == st["centers"].tobytes(), (v, e)
            assert np.array_equal(np.asarray(dt["counts"]), st["sizes"].astype(np.float32)), (v, e)
            assert dt["count"] == 1024 * min(e + 1, len(sts))
            assert dt["algorithm"] == "lloyd" and dt["spherical"] is True and dt["normalize"] is True
            n2 = (np.asarray(dt["centers"], np.float64) ** 2).sum(1)
            assert (np.abs(n2 - 1.0) <= 6e-7).all(), (v, e)
        assert np.array_equal(labels[v], L.nearest(runs["unit"][v], sts[-1]["centers"])), v


def test_cached_epoch_and_resume_follow_the_cache(runs, tmp_path):
    from acav100m_amd.clustering.cli import Cli
    # assign only, no switch: the cache says which space its centres live in
    out = str(tmp_path / "norm_copy")
    shutil.copytree(runs["norm"], out)
    for name in SHARDS:
        os.remove(os.path.join(out, name))
    runs["cluster"](runs["glob"], out, **{"clustering.cached_epoch": 1})
    for name in SHARDS:
        assert open(os.path.join(out, "epoch_1_" + name), "rb").read() == open(os.path.join(runs["norm"], name), "rb").read()
    # one more SGD epoch from the cache, without the switch, is the plain run's on the normalised shards
    a, b = str(tmp_path / "norm_resume"), str(tmp_path / "divided_resume")
    for src, dst in ((runs["norm"], a), (runs["divided"], b)):
        shutil.copytree(src, dst)
        for name in SHARDS:
            os.remove(os.path.join(dst, name))
    more = {"clustering.cached_epoch": 1, "clustering.resume_training": True, "clustering.epochs": 1}
    runs["cluster"](runs["glob"], a, **more)
    runs["cluster"](os.path.join(runs["root"], "features_unit", os.path.basename(runs["glob"])), b, **more)
    ca, cb = _cache(a, 1), _cache(b, 1)
    for (mk, layer) in runs["dims"]:
        assert np.asarray(ca[mk][layer]["centers"]).tobytes() == np.asarray(cb[mk][layer]["centers"]).tobytes(), (mk, layer)
        assert ca[mk][layer]["normalize"] is True and ca[mk][layer]["count"] == cb[mk][layer]["count"]
        assert ca[mk][layer]["count"] > _cache(runs["norm"], 1)[mk][layer]["count"]
    # a spherical state continues as one, whatever the switch says: one more iteration is the restatement's next one
    c = str(tmp_path / "sph_resume")
    shutil.copytree(runs["sph"], c)
    for name in SHARDS:
        os.remove(os.path.join(c, name))
    runs["cluster"](runs["glob"], c, **{"clustering.algorithm": "lloyd", "clustering.cached_epoch": ITERS - 1,
                                        "clustering.resume_training": True, "clustering.epochs": 1})
    after = _cache(c, ITERS - 1)
    for (mk, layer) in runs["dims"]:
        dt = after[mk][layer]
        assert dt["spherical"] is True and dt["normalize"] is True
        before = np.asarray(_cache(runs["sph"], ITERS - 1)[mk][layer]["centers"], np.float32)
        lab = L.nearest(runs["unit"][mk, layer], before)
        want, _sizes, _splits = R.spherical_update(runs["unit"][mk, layer], lab, K, L.shift_of(np.abs(runs["unit"][mk, layer]).max(), 1024))
        assert np.asarray(dt["centers"], np.float32).tobytes() == want.tobytes(), (mk, layer)
    # the switches that contradict a cache
    args = dict(feature_path=runs["glob"], **runs["common"])
    p = str(tmp_path / "plain_copy")
    shutil.copytree(runs["plain"], p)
    with pytest.raises(ValueError, match="holds no 'normalize' key"):
        Cli().cluster(out_path=p, **args, **{"clustering.cached_epoch": 1, "clustering.normalize": True})
    with pytest.raises(ValueError, match="not a spherical state|trained by sgd"):
        Cli().cluster(out_path=out, **args, **{"clustering.cached_epoch": 1, "clustering.resume_training": True, **SPHERICAL})


def test_evaluate_judges_in_normalised_space(runs):
    from acav100m_amd.clustering.cli import Cli
    common = dict(feature_path=runs["glob"], **runs["common"])
    rep_n = Cli().evaluate(out_path=runs["norm"], **common, **{"clustering.cached_epoch": 1})
    rep_d = Cli().evaluate(out_path=runs["divided"], **{**common, "feature_path": os.path.join(
        runs["root"], "features_unit", os.path.basename(runs["glob"]))}, **{"clustering.cached_epoch": 1})
    for name, per_epoch in rep_n["views"].items():
        a, b = dict(per_epoch["1"]), dict(rep_d["views"][name]["1"])
        assert a.pop("normalized") is True and "normalized" not in b and "mean_cosine" not in a
        assert a == b, name  # the same rows, the same centres: the same report, float for float
    rep_s = Cli().evaluate(out_path=runs["sph"], **common, **{"clustering.cached_epoch": ITERS - 1})
    labels, _ = _labels(runs["sph"], runs["dims"])
    for (mk, layer) in runs["dims"]:
        rep = rep_s["views"][mk + "/" + layer][str(ITERS - 1)]
        assert rep["normalized"] is True and rep["displaced"] == 0
        c = np.asarray(_cache(runs["sph"], ITERS - 1)[mk][layer]["centers"], np.float64)
        x = runs["unit"][mk, layer].astype(np.float64)
        a2 = ((x - c[labels[mk, layer]]) ** 2).sum(1)
        want = 1.0 - float(a2.mean()) / 2.0
        assert rep["mean_cosine"] == 1.0 - rep["inertia"] / 2.0
        assert abs(rep["mean_cosine"] - want) <= 1e-12 * abs(want), (mk, layer, rep["mean_cosine"], want)
        assert abs(rep["mean_cosine"] - float((x * c[labels[mk, layer]]).sum(1).mean())) <= 1e-6  # it is the mean cosine
    plain = Cli().evaluate(out_path=runs["plain"], **common, **{"clustering.cached_epoch": 1})
    for per_epoch in plain["views"].values():
        assert "normalized" not in per_epoch["1"] and "mean_cosine" not in per_epoch["1"]
