"""GPU: `clustering.cli cluster --clustering.whiten=True` on the synthetic shards of tests/golden/synth.py with every view's
columns rescaled by a seeded factor in [1e-3, 1e3]: the run equals the plain run on shards that hold x / std (the path every
other test pins), differs from the plain run on the raw shards, does not depend on the row groups, is resumed from its cache in
the same space, and `evaluate` judges it in that space."""
import os
import pickle
import shutil
import sys

import numpy as np
import pytest

from tests import _kmeans_quality_np as Q
from tests import _whiten_np as R

pytestmark = pytest.mark.gpu

SHARDS = ["shard-%06d.pkl" % s for s in range(4)]


def _kind(mk):
    return "audio" if mk == "layer_vggish" else "video"


def _rewrite(src_dir, dst_dir, fn):
    """every shard pkl of src_dir with feature arrays fn((model_key, layer), array) -> dst_dir"""
    os.makedirs(dst_dir, exist_ok=True)
    for name in SHARDS:
        rows = pickle.load(open(os.path.join(src_dir, name), "rb"))
        for r in rows:
            for kind, mk in (("audio", "layer_vggish"), ("video", "layer_slow_fast")):
                arr = r[kind + "_features"][0]["array"]
                for layer in arr:
                    arr[layer] = fn((mk, layer), arr[layer])
        with open(os.path.join(dst_dir, name), "wb") as f:
            pickle.dump(rows, f)


def _features(feat_dir, dims):
    """{(model_key, layer): fp32 [1024, d]}, the shards concatenated in shard order"""
    out = {v: [] for v in dims}
    for name in SHARDS:
        rows = pickle.load(open(os.path.join(feat_dir, name), "rb"))
        for (mk, layer) in dims:
            out[mk, layer].append(np.stack([r[_kind(mk) + "_features"][0]["array"][layer] for r in rows]).astype(np.float32))
    return {v: np.concatenate(parts) for v, parts in out.items()}


def _labels(out_dir, dims, prefix=""):
    """({(model_key, layer): int64 [1024]}, filenames) of a run's assignment shards"""
    labels, names = {v: [] for v in dims}, []
    for name in SHARDS:
        rows = pickle.load(open(os.path.join(out_dir, prefix + name), "rb"))
        names += [r["filename"] for r in rows]
        for (mk, layer) in dims:
            labels[mk, layer].append(np.array([int(r[_kind(mk) + "_assignments"][0]["array"][layer]) for r in rows], np.int64))
    return {v: np.concatenate(parts) for v, parts in labels.items()}, names


def _cache(out_dir, epoch=1):
    import torch
    files = [f for f in os.listdir(out_dir) if f.startswith("cache_epoch_%d_" % epoch)]
    assert len(files) == 1
    return torch.load(os.path.join(out_dir, files[0]), map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, golden_dir):
    """the shard sets and the three cluster runs every test looks at -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    root = str(tmp_path_factory.mktemp("acav_whiten_cli"))
    glob = synth.write_feature_shards(root, n_shards=4, rows=256, seed=0)
    feat = os.path.join(root, "features")
    dims = {("layer_vggish", "layer_%d" % i): d for i, d in enumerate(synth.AUDIO_DIMS)}
    dims.update({("layer_slow_fast", "layer_%d" % i): d for i, d in enumerate(synth.VIDEO_DIMS)})
    rs = np.random.RandomState(1234)
    scale = {v: np.exp(rs.uniform(np.log(1e-3), np.log(1e3), d)).astype(np.float32) for v, d in sorted(dims.items())}
    _rewrite(feat, feat, lambda v, a: (np.asarray(a, np.float32) * scale[v]).astype(np.float32))
    raw = _features(feat, dims)

    def cluster(glob_, out, **more):
        acav100m_amd.manual_seed(0)
        saved = Cli().cluster(feature_path=glob_, out_path=out, meta_path=os.path.join(root, "videos"),
                              **{"computation.num_workers": 0}, **more)
        assert len(saved) == 4
        return out

    white = cluster(glob, os.path.join(root, "white"), **{"clustering.whiten": True})
    nested = _cache(white)
    std = {(mk, layer): np.asarray(nested[mk][layer]["whiten_std"]) for (mk, layer) in dims}
    # a second shard set that holds x / std: the plain run on it is the path the other tests pin
    feat2 = os.path.join(root, "features_div")
    _rewrite(feat, feat2, lambda v, a: np.asarray(a, np.float32) / std[v])
    divided = cluster(os.path.join(feat2, os.path.basename(glob)), os.path.join(root, "divided"))
    plain = cluster(glob, os.path.join(root, "plain"))
    return dict(root=root, glob=glob, dims=dims, raw=raw, std=std, white=white, divided=divided, plain=plain, cluster=cluster)


def test_whitened_run_is_the_plain_run_on_divided_shards(runs):
    dims = runs["dims"]
    lw, names_w = _labels(runs["white"], dims)
    ld, names_d = _labels(runs["divided"], dims)
    assert names_w == names_d and len(names_w) == 1024
    for v in dims:
        assert np.array_equal(lw[v], ld[v]), v
    for epoch in (0, 1):
        cw, cd = _cache(runs["white"], epoch), _cache(runs["divided"], epoch)
        for (mk, layer), d in dims.items():
            a, b = cw[mk][layer], cd[mk][layer]
            for key in ("centers", "counts"):
                assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (mk, layer, key)
            assert a["count"] == b["count"] and a["fallback"] == b["fallback"]
            assert set(a) == set(b) | {"whiten_std"}  # the unwhitened run's cache keeps today's keys
            assert a["whiten_std"].dtype == np.float32 and a["whiten_std"].shape == (d,)
            assert a["whiten_std"].tobytes() == runs["std"][mk, layer].tobytes()  # one std for every epoch of the run


def test_cached_std_is_the_restatements(runs):
    for v, x in runs["raw"].items():
        want, zero = R.std_of(x)
        worst = int(R.ulp_diff(runs["std"][v], want).max())
        print(v, "max ulp", worst, "std", float(want.min()), float(want.max()))
        assert worst <= 1 and zero == 0
        assert want.max() / want.min() > 1e3  # the columns really are on different scales


def test_the_switch_does_something(runs):
    lw, _ = _labels(runs["white"], runs["dims"])
    lp, _ = _labels(runs["plain"], runs["dims"])
    differ = [v for v in runs["dims"] if not np.array_equal(lw[v], lp[v])]
    print("views whose labels differ:", len(differ))
    assert differ
    assert all("whiten_std" not in _cache(runs["plain"])[mk][layer] for (mk, layer) in runs["dims"])


def test_row_groups_change_nothing(runs):
    shard_bytes = 256 * 4 * sum(runs["dims"].values())
    out = runs["cluster"](runs["glob"], os.path.join(runs["root"], "white_groups"),
                          **{"clustering.whiten": True, "data.resident_bytes": int(2.5 * shard_bytes)})
    for name in SHARDS:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(runs["white"], name), "rb").read(), name
    nested = _cache(out)
    for (mk, layer) in runs["dims"]:
        assert nested[mk][layer]["whiten_std"].tobytes() == runs["std"][mk, layer].tobytes(), (mk, layer)


def test_assign_only_from_the_cache(runs, tmp_path):
    """no whiten flag: the cache says which space its centres live in"""
    out = str(tmp_path / "white_copy")
    shutil.copytree(runs["white"], out)
    for name in SHARDS:
        os.remove(os.path.join(out, name))
    runs["cluster"](runs["glob"], out, **{"clustering.cached_epoch": 1})
    want, names = _labels(runs["white"], runs["dims"])
    got, got_names = _labels(out, runs["dims"], prefix="epoch_1_")
    assert got_names == names
    for v in runs["dims"]:
        assert np.array_equal(got[v], want[v]), v
    for name in SHARDS:  # the rows a cached epoch writes are the rows the run wrote
        assert open(os.path.join(out, "epoch_1_" + name), "rb").read() == open(os.path.join(runs["white"], name), "rb").read()
    # the other way round: asking for whitening against centres trained on raw rows
    out_p = str(tmp_path / "plain_copy")
    shutil.copytree(runs["plain"], out_p)
    from acav100m_amd.clustering.cli import Cli
    with pytest.raises(ValueError, match="cache_epoch_1_"):
        Cli().cluster(feature_path=runs["glob"], out_path=out_p, meta_path=os.path.join(runs["root"], "videos"),
                      **{"computation.num_workers": 0, "clustering.cached_epoch": 1, "clustering.whiten": True})


def test_evaluate_judges_in_whitened_space(runs):
    from acav100m_amd.clustering.cli import Cli
    from tests.test_gpu_cluster_evaluate_cli import _check_against
    common = dict(feature_path=runs["glob"], meta_path=os.path.join(runs["root"], "videos"), **{"computation.num_workers": 0})
    report = Cli().evaluate(out_path=runs["white"], **common, **{"clustering.cached_epoch": 1})
    labels, _ = _labels(runs["white"], runs["dims"])
    nested = _cache(runs["white"])
    for (mk, layer) in runs["dims"]:
        rep = report["views"][mk + "/" + layer]["1"]
        assert rep["whitened"] is True and rep["zero_variance_columns"] == 0
        dt = nested[mk][layer]
        c = np.asarray(dt["centers"], np.float32)
        ref = Q.Reference(runs["raw"][mk, layer] / runs["std"][mk, layer], c, labels[mk, layer])
        _check_against(rep, ref, c, np.asarray(dt["counts"], np.float32), int(dt["count"]))
    plain = Cli().evaluate(out_path=runs["plain"], **common, **{"clustering.cached_epoch": 1})
    for per_epoch in plain["views"].values():
        assert "whitened" not in per_epoch["1"] and "zero_variance_columns" not in per_epoch["1"]
