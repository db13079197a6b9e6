"""GPU: `subset_selection.cli run --measure_name=pca_*` on tiny synthetic feature shards (tests/golden/synth.py: 3 shards of about
70 clips, 2 audio + 2 visual views of widths 12, 20, 16, 24): the csv holds exactly the clips the Python API selects in-process
from the same shards (the API's pieces are pinned by test_gpu_pca_measure.py and the PCA / whitening tests), the switches run,
a view narrower than pca.dim is refused before any kernel runs, and the chunked mode + reduce_csvs gives the union of the
per-chunk selections."""
import csv
import os
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROWS = [70, 64, 75]


@pytest.fixture(scope="module")
def shards(tmp_path_factory, golden_dir):
    sys.path.insert(0, golden_dir)
    import synth
    root = str(tmp_path_factory.mktemp("acav_pca_measure_cli"))
    glob = synth.write_feature_shards(root, n_shards=3, rows=ROWS, seed=4, comps=6, audio_dims=[12, 20], video_dims=[16, 24])
    return root, glob, os.path.join(root, "videos")


def _cli(shards, out, **more):
    from acav100m_amd.subset_selection.cli import Cli
    root, glob, meta = shards
    out = os.path.join(root, out)
    path, count = Cli().run(shards_path=glob, meta_path=meta, out_path=out, **more)
    assert str(path) == os.path.join(os.path.realpath(out), "output.csv") and count == len(_read(path))  # a directory: the csv goes inside
    return str(path)


def _read(path):
    with open(path, newline='') as f:
        return [row for row in csv.reader(f)]


def _api(shards, paths, name, k=None, dim=8, whiten=True):
    """the same selection through the Python API: (shard_name, filename) of sorted(S)"""
    from acav100m_amd import shards as io
    from acav100m_amd.clustering import pca_features, whiten as whiten_fn
    from acav100m_amd.subset_selection.measures import get_measure
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    table = io.load_feature_shards([Path(p) for p in paths])
    by_key = {(mk, layer): m for (kind, mk, layer), m in table.views.items()}
    keys = sorted(by_key)
    views = {key: by_key[key] for key in keys}
    if whiten:
        views = {key: whiten_fn(v)[0] for key, v in views.items()}
    proj = pca_features(views, dim)
    meas = get_measure(name)([proj[key] for key in keys])
    meas.init(get_cluster_pairing(keys, 'combination', None), list(range(len(table))))
    V = len(table)
    S, _, _, _ = meas.run(round(0.2 * V) if k is None else k, None)
    assert len(keys) == 4 and proj[keys[0]].shape == (V, dim if dim is not None else 12)
    return [(table.shard_name[i], table.filename[i]) for i in sorted(S)]


def _paths(shards):
    from acav100m_amd import shards as io
    return sorted(io.brace_expand(shards[1]))


def test_cli_selects_what_the_api_selects(shards):
    out = _cli(shards, "cs", measure_name="pca_cs", **{"pca.dim": 8})
    rows = _read(out)
    assert os.path.basename(out) == "output.csv"
    V = sum(ROWS)
    assert len(rows) == round(0.2 * V)
    want = _api(shards, _paths(shards), "pca_cs")
    assert [(r[0], r[1]) for r in rows] == want
    for r in rows:  # the csv layout of the other measures: shard_name, filename, id, segment
        assert len(r) == 4 and r[0].startswith("shard-") and r[1] == r[2] + "_010.mp4" and r[3] == "[10, 20]"


@pytest.mark.parametrize("name", ["pca", "pca_ip", "pca_l1", "pca_l2"])
def test_every_name_runs_from_the_cli(shards, name):
    out = _cli(shards, "name_" + name, measure_name=name, **{"pca.dim": 8, "subset.size": 17})
    assert [(r[0], r[1]) for r in _read(out)] == _api(shards, _paths(shards), name, k=17)


def test_switches(shards):
    out = _cli(shards, "plain", measure_name="pca_l2", **{"pca.whiten": False, "pca.dim": 8})
    assert [(r[0], r[1]) for r in _read(out)] == _api(shards, _paths(shards), "pca_l2", whiten=False)
    out = _cli(shards, "narrowest", measure_name="pca_ip")  # pca.dim unset: the smallest view width, 12
    assert [(r[0], r[1]) for r in _read(out)] == _api(shards, _paths(shards), "pca_ip", dim=None)


def test_a_view_narrower_than_dim_is_refused_before_any_kernel_runs(shards):
    from acav100m_amd import _lib
    lib = _lib.load_library()
    calls = []
    names = ("acav_colstats", "acav_rows_scale", "acav_rows_scatter", "acav_rows_project", "acav_pair_scores", "acav_rank_desc")
    saved = {n: getattr(lib, n) for n in names}
    try:
        for n in names:
            setattr(lib, n, lambda *a, _n=n: calls.append(_n) or saved[_n](*a))
        with pytest.raises(ValueError, match="narrower than pca.dim=13"):
            _cli(shards, "narrow", measure_name="pca_cs", **{"pca.dim": 13})
        with pytest.raises(ValueError, match="N <= p"):
            _few_clips(shards)
    finally:
        for n in names:
            setattr(lib, n, saved[n])
    assert calls == []
    assert not os.path.exists(os.path.join(shards[0], "narrow", "output.csv"))


def _few_clips(shards):
    """V <= dim: the existing ValueError, raised by the driver before the first kernel"""
    from acav100m_amd import shards as io
    from acav100m_amd.config import SUBSET_DEFAULTS, merge
    from acav100m_amd.subset_selection.run_pca import projected_views
    table = io.load_feature_shards([Path(_paths(shards)[0])])
    table.filename = table.filename[:10]
    for key in list(table.views):
        table.views[key] = table.views[key][:10]
    projected_views(merge(SUBSET_DEFAULTS, {"pca.dim": 12, "computation.device": "cuda"}), table)


def test_chunked_run_and_reduce_give_the_union_of_the_chunks(shards):
    from acav100m_amd.subset_selection.cli import Cli
    root, glob, meta = shards
    out = os.path.join(root, "chunked")
    Cli().run(shards_path=glob, meta_path=meta, out_path=out, measure_name="pca_cs", chunk_size=1, parent_pid="777",
              **{"pca.dim": 8})
    caches = sorted(os.listdir(os.path.join(out, "caches")))
    assert caches == ["cache_777_0_%d_output.csv" % i for i in range(3)]
    assert not os.path.exists(os.path.join(out, "output.csv"))
    total = Cli().reduce_csvs(shards_path=glob, meta_path=meta, out_path=out)
    want = []
    for path, n in zip(_paths(shards), ROWS):
        part = _api(shards, [path], "pca_cs", k=round(0.2 * n))
        assert len(part) == round(0.2 * n)
        want += part
    rows = _read(os.path.join(out, "output.csv"))
    assert total == len(want) and [(r[0], r[1]) for r in rows] == want
