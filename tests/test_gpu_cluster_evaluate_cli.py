"""GPU: `clustering.cli evaluate` after `clustering.cli cluster` on the synthetic shards of tests/golden/synth.py: the counts
are the assignment shards' label counts, the figures are the float64 restatement's (tests/_kmeans_quality_np.py) on the cache's
centres, the shard features and those labels; nothing is written into the cluster run's directory; row groups change nothing."""
import json
import os
import pickle
import sys

import numpy as np
import pytest

from tests import _kmeans_quality_np as R

pytestmark = pytest.mark.gpu

INT_FIELDS = ("n", "K", "empty", "empty_clusters", "sizes", "size_min", "size_median", "size_max", "displaced", "underused",
              "underused_clusters")


@pytest.fixture(scope="module")
def run(tmp_path_factory, golden_dir):
    """cluster with the defaults (2 epochs), then evaluate epochs 0 and 1 -- once for all tests"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    root = str(tmp_path_factory.mktemp("acav_quality_cli"))
    glob = synth.write_feature_shards(root, n_shards=4, rows=256, seed=0)
    out = os.path.join(root, "clusters")
    common = dict(feature_path=glob, out_path=out, meta_path=os.path.join(root, "videos"), **{"computation.num_workers": 0})
    acav100m_amd.manual_seed(0)
    saved = Cli().cluster(**common)
    assert len(saved) == 4
    before = sorted(os.listdir(out))
    json_path = os.path.join(root, "reports", "quality.json")
    report = Cli().evaluate(**common, **{"clustering.cached_epoch": [0, 1], "evaluate.out_path": json_path})
    dims = {("layer_vggish", "layer_%d" % i): d for i, d in enumerate(synth.AUDIO_DIMS)}
    dims.update({("layer_slow_fast", "layer_%d" % i): d for i, d in enumerate(synth.VIDEO_DIMS)})
    return dict(root=root, out=out, common=common, before=before, json_path=json_path, report=report, dims=dims)


@pytest.fixture(scope="module")
def references(run):
    """{view name: (Reference, centres, counts, count)} of epoch 1: the cache's centres, the shard features, the shards' labels"""
    import torch
    feats, labels = {v: [] for v in run["dims"]}, {v: [] for v in run["dims"]}
    for s in range(4):
        name = "shard-%06d.pkl" % s
        frows = pickle.load(open(os.path.join(run["root"], "features", name), "rb"))
        arows = pickle.load(open(os.path.join(run["out"], name), "rb"))
        assert [r["filename"] for r in frows] == [r["filename"] for r in arows]
        for (mk, layer) in run["dims"]:
            kind = "audio" if mk == "layer_vggish" else "video"
            feats[mk, layer].append(np.stack([r[kind + "_features"][0]["array"][layer] for r in frows]).astype(np.float32))
            labels[mk, layer].append(np.array([int(r[kind + "_assignments"][0]["array"][layer]) for r in arows], np.int64))
    cache = [f for f in os.listdir(run["out"]) if f.startswith("cache_epoch_1_")]
    assert len(cache) == 1
    nested = torch.load(os.path.join(run["out"], cache[0]), map_location="cpu", weights_only=False)
    refs = {}
    for (mk, layer) in run["dims"]:
        dt = nested[mk][layer]
        c = np.asarray(dt["centers"], np.float32)
        x, lab = np.concatenate(feats[mk, layer]), np.concatenate(labels[mk, layer])
        assert x.shape == (1024, run["dims"][mk, layer])
        refs[mk + "/" + layer] = (R.Reference(x, c, lab), c, np.asarray(dt["counts"], np.float32), int(dt["count"]))
    return refs


def _check_against(rep, ref, c, counts, count):
    """one view's report against the restatement within the propagated bounds"""
    from acav100m_amd.clustering.evaluate import compose
    want = compose(ref.cluster, c, counts, count)
    n, K = want["n"], want["K"]
    assert rep["n"] == n == 1024 and rep["K"] == K
    for key in ("empty", "empty_clusters", "sizes", "size_min", "size_median", "size_max", "underused", "underused_clusters"):
        assert rep[key] == want[key], key
    assert abs(rep["displaced"] - want["displaced"]) <= int(ref.undecided.sum())
    tol = ref.cluster_tol
    for key, col in (("inertia", R.SUM_A2), ("nearest_inertia", R.SUM_MIN), ("silhouette", R.SUM_S)):
        bound = tol[:, col].sum() / n + (K + 1) * 2.0 ** -52 * abs(want[key])
        print("{}: {!r} vs {!r}, bound {:.3g}".format(key, rep[key], want[key], bound))
        assert abs(rep[key] - want[key]) <= bound, key
    # Davies-Bouldin: S_k = sum sqrt a2 / count moves by dS_k, every ratio (S_k + S_l) / M_kl by at most 2 max dS / min M
    ne = ref.cluster[:, R.COUNT] > 0
    dS = (tol[ne, R.SUM_SQRT_A2] / ref.cluster[ne, R.COUNT]).max()
    C8 = c[ne].astype(np.float64)
    M = np.sqrt(((C8[:, None] - C8[None]) ** 2).sum(-1))
    bound = 2 * dS / M[M > 0].min() + 2.0 ** -50 * want["davies_bouldin"]
    print("davies_bouldin: {!r} vs {!r}, bound {:.3g}".format(rep["davies_bouldin"], want["davies_bouldin"], bound))
    assert abs(rep["davies_bouldin"] - want["davies_bouldin"]) <= bound


def test_counts_are_the_assignment_shards_label_counts(run, references):
    from acav100m_amd.clustering.evaluate import evaluate  # noqa: F401  (the module exists)
    assert sorted(run["report"]["views"]) == sorted(references) and run["report"]["epochs"] == [0, 1]
    for name, (ref, c, counts, count) in references.items():
        rep = run["report"]["views"][name]["1"]
        sizes = np.bincount(ref.labels, minlength=c.shape[0])
        assert rep["sizes"] == sizes.tolist()  # per cluster, exactly
        assert rep["n"] == 1024 and rep["empty_clusters"] == [int(k) for k in np.flatnonzero(sizes == 0)]
        assert (rep["size_min"], rep["size_median"], rep["size_max"]) == (int(sizes.min()), float(np.median(sizes)), int(sizes.max()))
        assert set(run["report"]["views"][name]) == {"0", "1"} and run["report"]["views"][name]["0"]["n"] == 1024


def test_figures_match_the_restatement(run, references):
    for name, (ref, c, counts, count) in references.items():
        print(name)
        _check_against(run["report"]["views"][name]["1"], ref, c, counts, count)


def test_nothing_is_written_into_the_cluster_run(run):
    assert sorted(os.listdir(run["out"])) == run["before"]
    assert not any(f.startswith("epoch_") for f in os.listdir(run["out"]))  # no assignment shard of a cached epoch


def test_json_round_trips(run):
    loaded = json.load(open(run["json_path"]))
    assert loaded == json.loads(json.dumps(run["report"]))
    assert loaded["views"].keys() == run["report"]["views"].keys()
    for name, per_epoch in run["report"]["views"].items():
        for e, rep in per_epoch.items():
            assert loaded["views"][name][e] == rep  # every figure is finite here: equal value for value


def test_row_groups_change_nothing(run, references):
    from acav100m_amd.clustering.cli import Cli
    shard_bytes = 256 * 4 * sum(run["dims"].values())
    report = Cli().evaluate(**run["common"], **{"clustering.cached_epoch": [0, 1], "data.resident_bytes": int(2.5 * shard_bytes)})
    for name, (ref, c, counts, count) in references.items():
        for key in INT_FIELDS:
            for e in ("0", "1"):
                assert report["views"][name][e][key] == run["report"]["views"][name][e][key], (name, e, key)
        _check_against(report["views"][name]["1"], ref, c, counts, count)
    assert sorted(os.listdir(run["out"])) == run["before"]


def test_rows_path_writes_per_clip_distances(run, references, tmp_path):
    from acav100m_amd.clustering.cli import Cli
    Cli().evaluate(**run["common"], **{"clustering.cached_epoch": 1, "evaluate.rows_path": str(tmp_path / "rows")})
    assert sorted(os.listdir(tmp_path / "rows")) == ["shard-%06d.quality.npz" % s for s in range(4)]
    for s in range(4):
        z = np.load(tmp_path / "rows" / ("shard-%06d.quality.npz" % s))
        frows = pickle.load(open(os.path.join(run["root"], "features", "shard-%06d.pkl" % s), "rb"))
        assert list(z["filename"]) == [r["filename"] for r in frows] and z["epochs"].tolist() == [1]
        for name, (ref, c, counts, count) in references.items():
            got = z[name]
            assert got.shape == (1, 256, 2) and got.dtype == np.float64
            sl = slice(256 * s, 256 * (s + 1))
            assert (np.abs(got[0, :, 0] - ref.a2[sl]) <= ref.ta[sl]).all() and (np.abs(got[0, :, 1] - ref.b2[sl]) <= ref.tb[sl]).all()
    assert sorted(os.listdir(run["out"])) == run["before"]
