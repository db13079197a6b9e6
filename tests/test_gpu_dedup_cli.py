"""GPU: `clustering.cli dedup` after `clustering.cli cluster` (lloyd, K = 4, 3 iterations) on three synthetic shards with two
views (24 and 40 columns, 200 rows each) into which 17 rows were copied bitwise at later positions, some into another shard: the
csv names exactly the 17 later copies with their first occurrences, the json is summarise of the float64 restatement
(tests/_neardup_np.py) on the assignment shards' labels, a second run and a streamed run change no byte, a whitened cache is
compared in its own space, the cluster directory gains nothing; and `subset_selection.cli run --exclude_path=<that csv>` selects
from the clips that remain exactly what run_greedy selects from the masked arrays."""
import csv
import json
import os
import pickle
import random
import sys

import numpy as np
import pytest

from tests import _neardup_np as R

pytestmark = pytest.mark.gpu

N_SHARDS, ROWS = 3, 200
SHARDS = ["shard-%06d.pkl" % s for s in range(N_SHARDS)]
DIMS = {("layer_vggish", "layer_0"): 24, ("layer_slow_fast", "layer_0"): 40}
VIEW = ("layer_vggish", "layer_0")
K, ITERS, THRESHOLD = 4, 3, 0.999999
# (first occurrence, later copy) as global row numbers: 17 copies, 7 of them in a later shard than their source
PLANTED = [(0, 1), (3, 150), (10, 199), (17, 200), (40, 41), (77, 402), (120, 599), (180, 181), (199 - 4, 333), (201, 202),
           (250, 398), (260, 400), (399 - 2, 401), (405, 406), (420, 590), (450, 451), (5, 300)]


def _kind(mk):
    return "audio" if mk == "layer_vggish" else "video"


def _name(g):
    return "shard-%06d" % (g // ROWS), "vid%09d_010.mp4" % g


def _column(dir_, field, cast):
    out = {v: [] for v in DIMS}
    for name in SHARDS:
        rows = pickle.load(open(os.path.join(dir_, name), "rb"))
        for (mk, layer) in DIMS:
            out[mk, layer].append(np.stack([cast(r[_kind(mk) + field][0]["array"][layer]) for r in rows]))
    return {v: np.concatenate(parts) for v, parts in out.items()}


@pytest.fixture(scope="module")
def run(tmp_path_factory, golden_dir):
    """the shards with their planted copies, a plain and a whitened Lloyd run and the dedup of one view of each -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    assert len(PLANTED) == 17 and len({t for _, t in PLANTED}) == 17 and not {s for s, _ in PLANTED} & {t for _, t in PLANTED}
    assert all(s < t for s, t in PLANTED) and sum(s // ROWS != t // ROWS for s, t in PLANTED) == 7
    root = str(tmp_path_factory.mktemp("acav_dedup_cli"))
    glob = synth.write_feature_shards(root, n_shards=N_SHARDS, rows=ROWS, seed=2, comps=6, audio_dims=[24], video_dims=[40])
    feat = os.path.join(root, "features")
    shards = [pickle.load(open(os.path.join(feat, name), "rb")) for name in SHARDS]
    for s, t in PLANTED:  # the feature arrays of both views, bitwise; the clip keeps its own name
        src, dst = shards[s // ROWS][s % ROWS], shards[t // ROWS][t % ROWS]
        for kind in ("audio", "video"):
            dst[kind + "_features"][0]["array"] = {k: v.copy() for k, v in src[kind + "_features"][0]["array"].items()}
    for name, rows in zip(SHARDS, shards):
        with open(os.path.join(feat, name), "wb") as f:
            pickle.dump(rows, f)
    base = dict(feature_path=glob, meta_path=os.path.join(root, "videos"), **{"computation.num_workers": 0})
    lloyd = {"clustering.algorithm": "lloyd", "clustering.ncentroids": K, "clustering.epochs": ITERS}
    outs = {}
    for name, more in (("plain", {}), ("white", {"clustering.whiten": True})):
        acav100m_amd.manual_seed(0)
        outs[name] = os.path.join(root, name)
        assert len(Cli().cluster(out_path=outs[name], **base, **lloyd, **more)) == N_SHARDS
    before = {name: sorted(os.listdir(out)) for name, out in outs.items()}

    def dedup(name, tag, **more):
        opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": THRESHOLD, "dedup.view": "/".join(VIEW),
                "dedup.out_path": os.path.join(root, tag + ".csv"), "dedup.report_path": os.path.join(root, tag + ".json")}
        opts.update(more)
        report = Cli().dedup(out_path=outs[name], **base, **opts)
        return report, open(opts["dedup.out_path"], "rb").read(), open(opts["dedup.report_path"], "rb").read()

    first = {name: dedup(name, name + "_first") for name in outs}
    return dict(root=root, glob=glob, base=base, outs=outs, before=before, dedup=dedup, first=first,
                x=_column(feat, "_features", lambda a: np.asarray(a, np.float32)),
                labels={name: _column(out, "_assignments", np.int64) for name, out in outs.items()})


def _cache(out_dir):
    import torch
    files = [f for f in os.listdir(out_dir) if f.startswith("cache_epoch_%d_" % (ITERS - 1))]
    assert len(files) == 1
    return torch.load(os.path.join(out_dir, files[0]), map_location="cpu", weights_only=False)[VIEW[0]][VIEW[1]]


def _check(run, name, x):
    """the csv and the json of the first dedup of run `name` against the restatement on rows x"""
    from acav100m_amd.clustering.dedup import summarise
    lab = run["labels"][name][VIEW]
    best, partner, _second = R.nearest_earlier(x, lab, K)
    copies = np.array(sorted(t for _, t in PLANTED))
    others = np.setdiff1d(np.arange(len(lab)), copies)
    print("{}: largest best of an unplanted row {:.4f}".format(name, best[others].max()))
    assert best[others].max() < 0.99  # no unplanted row comes near the threshold
    report, csv_bytes, json_bytes = run["first"][name]
    lines = list(csv.reader(csv_bytes.decode().splitlines()))
    source = dict((t, s) for s, t in PLANTED)
    assert [tuple(ln[:4]) for ln in lines] == [_name(t) + _name(source[t]) for t in copies]  # global row order
    for ln, t in zip(lines, copies):
        assert len(ln) == 5 and ln[4] == repr(float(ln[4])) and abs(float(ln[4]) - 1.0) <= R.bound(x.shape[1])
        assert abs(float(ln[4]) - best[t]) <= R.bound(x.shape[1]) and partner[t] == source[t]
    want = summarise(best, partner, lab, K, THRESHOLD)
    assert want["flagged"] == 17 and want["n"] == N_SHARDS * ROWS
    loaded = json.loads(json_bytes)
    assert {k: loaded[k] for k in want} == json.loads(json.dumps(want))
    assert set(loaded) == set(want) | {"view", "epoch", "feature_path", "clusters_path"}
    assert loaded["view"] == "/".join(VIEW) and loaded["epoch"] == ITERS - 1 and loaded == json.loads(json.dumps(report))


def test_the_csv_names_the_17_later_copies_and_the_json_is_the_restatements(run):
    _check(run, "plain", run["x"][VIEW])


def test_a_whitened_cache_is_compared_in_its_own_space(run):
    std = np.asarray(_cache(run["outs"]["white"])["whiten_std"], np.float32)
    x = run["x"][VIEW] / std  # one fp32 division per element, like the run's
    assert x.dtype == np.float32 and not np.array_equal(std, np.ones_like(std))
    _check(run, "white", x)


def test_a_second_run_and_a_streamed_run_change_no_byte(run):
    _report, csv_bytes, json_bytes = run["first"]["plain"]
    again = run["dedup"]("plain", "plain_again")
    assert again[1] == csv_bytes and again[2] == json_bytes
    shard_bytes = ROWS * 4 * sum(DIMS.values())
    streamed = run["dedup"]("plain", "plain_streamed", **{"data.resident_bytes": int(2.5 * shard_bytes)})  # one shard per group
    assert streamed[1] == csv_bytes and streamed[2] == json_bytes
    # an existing file is overwritten, not appended to
    assert run["dedup"]("plain", "plain_again")[1] == csv_bytes


def test_the_other_view_and_the_refusals(run):
    from acav100m_amd.clustering.cli import Cli
    other = run["dedup"]("plain", "plain_video", **{"dedup.view": "layer_slow_fast/layer_0"})
    assert other[0]["flagged"] == 17 and other[0]["view"] == "layer_slow_fast/layer_0"  # both views of a copy were copied
    opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": THRESHOLD, "dedup.out_path": os.path.join(run["root"], "no.csv")}
    with pytest.raises(ValueError, match="dedup.view is required"):
        Cli().dedup(out_path=run["outs"]["plain"], **run["base"], **opts)
    with pytest.raises(ValueError, match="exactly one epoch"):
        Cli().dedup(out_path=run["outs"]["plain"], **run["base"], **dict(opts, **{"clustering.cached_epoch": [1, 2]}))
    with pytest.raises(ValueError, match="dedup.threshold"):
        Cli().dedup(out_path=run["outs"]["plain"], **run["base"], **dict(opts, **{"dedup.threshold": 1.5}))
    assert not os.path.exists(os.path.join(run["root"], "no.csv"))


def test_nothing_appears_in_the_cluster_directory(run):
    for name, out in run["outs"].items():
        assert sorted(os.listdir(out)) == run["before"][name]


def test_the_selection_leaves_the_listed_clips_out(run):
    import acav100m_amd
    from acav100m_amd import shards as io
    from acav100m_amd.subset_selection import exclude
    from acav100m_amd.subset_selection.cli import Cli, prepare
    from acav100m_amd.subset_selection.run import greedy_options
    from acav100m_amd.subset_selection.run_greedy import run_greedy
    root, out = run["root"], run["outs"]["plain"]
    glob = os.path.join(out, "shard-{000000..%06d}.pkl" % (N_SHARDS - 1))
    meta = os.path.join(root, "videos")
    dups = os.path.join(root, "plain_first.csv")
    paths = [os.path.join(out, name) for name in SHARDS]

    def seeded():
        acav100m_amd.manual_seed(0)
        random.seed(0)

    def direct(csv_path, mask):
        """run_greedy on the (masked) arrays, written as run_single writes them"""
        args = prepare(shards_path=glob, meta_path=meta, out_path=csv_path)
        a, types, shard_names, filenames = io.load_assignment_shards(paths)
        ids = np.flatnonzero(mask(shard_names, filenames))
        seeded()
        rows = run_greedy(args, np.ascontiguousarray(a[ids]), [shard_names[i] for i in ids], [filenames[i] for i in ids], types,
                          args.subset.size, args.subset.ratio, **greedy_options(args))
        io.append_output_csv(rows, io.load_metas([os.path.join(out, n) for n in SHARDS], meta), args.data.output.path)
        return open(csv_path, "rb").read()

    def cli(csv_path, **more):
        seeded()
        Cli().run(shards_path=glob, meta_path=meta, out_path=csv_path, **more)
        return open(csv_path, "rb").read()

    V = N_SHARDS * ROWS
    listed = exclude.read_exclude(dups)
    assert len(listed) == 17
    got = cli(os.path.join(root, "sel_excl", "output.csv"), exclude_path=dups)
    lines = list(csv.reader(got.decode().splitlines()))
    assert not {(ln[0], os.path.splitext(ln[1])[0]) for ln in lines} & listed
    assert len(lines) == round(0.2 * (V - 17))
    keep = lambda sn, fn: exclude.keep_mask(listed, sn, fn)[0]  # noqa: E731
    assert got == direct(os.path.join(root, "sel_excl_direct", "output.csv"), keep)
    # without the key: the file of a run that never heard of it
    plain = cli(os.path.join(root, "sel_plain", "output.csv"))
    assert plain == direct(os.path.join(root, "sel_plain_direct", "output.csv"), lambda sn, fn: np.ones(len(sn), bool))
    assert len(plain.splitlines()) == round(0.2 * V) and plain != got
    # "select more, but not these": the output.csv of the first run is an exclude list too
    more = cli(os.path.join(root, "sel_more", "output.csv"), exclude_path=os.path.join(root, "sel_excl", "output.csv"))
    first = {(ln[0], ln[1]) for ln in lines}
    assert not {(ln[0], ln[1]) for ln in csv.reader(more.decode().splitlines())} & first
