"""GPU: `clustering.cli dedup --dedup.against_path=...` after `clustering.cli cluster` (lloyd, K = 4, 3 iterations): a pool of
three synthetic shards (200 rows, views of 24 and 40 columns) against a held-out set of two shards (60 rows) of which 11 rows
were copied bitwise, both views, into 13 pool rows.  The csv names exactly the 13 pool rows with the held-out clips they copy,
the json is summarise_against of the float64 restatement (tests/_crossdup_np.py) plus the verb's own keys, blocking=cluster
flags the same 13 and reports the restatement's pairs, a second run and a pool streamed one shard per group change no byte, a
whitened cache is compared in its own space, `exclude.read_exclude` accepts the csv, a run without against_path still writes
the in-cluster dedup, the refusals hold and the cluster directory gains nothing."""
import csv
import json
import os
import pickle
import sys

import numpy as np
import pytest

from tests import _crossdup_np as R
from tests import _neardup_np as RN

pytestmark = pytest.mark.gpu

POOL_SHARDS, POOL_ROWS, HELD_SHARDS, HELD_ROWS = 3, 200, 2, 60
DIMS = {("layer_vggish", "layer_0"): 24, ("layer_slow_fast", "layer_0"): 40}
VIEW = ("layer_vggish", "layer_0")
K, ITERS, THRESHOLD = 4, 3, 0.999999
# (held-out row, pool row that becomes its bitwise copy) as global row numbers: 13 pool rows copy 11 held-out rows, the rows 3
# and 60 twice; 6 of the held-out rows lie in the second held-out shard
PLANTED = [(0, 5), (3, 150), (15, 199), (30, 200), (59, 41), (60, 402), (61, 599), (75, 181), (90, 333), (100, 202), (119, 398),
           (3, 400), (60, 17)]
HELD_TWIN = (15, 70)  # held-out row 70 becomes a bitwise copy of row 15: the lower position is the partner
ZERO_POOL, ZERO_HELD = 77, 110  # an all-zero row on either side


def _kind(mk):
    return "audio" if mk == "layer_vggish" else "video"


def _name(g, rows):
    return "shard-%06d" % (g // rows), "vid%09d_010.mp4" % g


def _read(dir_, n_shards):
    return [pickle.load(open(os.path.join(dir_, "shard-%06d.pkl" % s), "rb")) for s in range(n_shards)]


def _write(dir_, shards):
    for s, rows in enumerate(shards):
        with open(os.path.join(dir_, "shard-%06d.pkl" % s), "wb") as f:
            pickle.dump(rows, f)


def _arrays(row):
    return {kind: row[kind + "_features"][0]["array"] for kind in ("audio", "video")}


def _copy(dst, src, zero=False):
    """the feature arrays of both views, bitwise (zero: zeros of their shapes); the clip keeps its own name"""
    for kind, arrays in _arrays(src).items():
        dst[kind + "_features"][0]["array"] = {k: np.zeros_like(v) if zero else v.copy() for k, v in arrays.items()}


def _features(shards):
    return {(mk, layer): np.stack([np.asarray(_arrays(r)[_kind(mk)][layer], np.float32) for rows in shards for r in rows])
            for (mk, layer) in DIMS}


@pytest.fixture(scope="module")
def run(tmp_path_factory, golden_dir):
    """the two sets, a plain and a whitened Lloyd run on the pool, and the first dedup against the held-out set of each -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    assert len(PLANTED) == 13 == len({t for _, t in PLANTED}) and len({h for h, _ in PLANTED}) == 11
    assert sum(h >= HELD_ROWS for h in {h for h, _ in PLANTED}) == 6 and ZERO_POOL not in {t for _, t in PLANTED}
    root = str(tmp_path_factory.mktemp("acav_dedup_against"))
    roots = {name: os.path.join(root, name) for name in ("pool", "held")}
    glob = synth.write_feature_shards(roots["pool"], n_shards=POOL_SHARDS, rows=POOL_ROWS, seed=2, comps=6, audio_dims=[24],
                                      video_dims=[40])
    held_glob = synth.write_feature_shards(roots["held"], n_shards=HELD_SHARDS, rows=HELD_ROWS, seed=3, comps=6, audio_dims=[24],
                                           video_dims=[40])
    feat = {name: os.path.join(r, "features") for name, r in roots.items()}
    pool, held = _read(feat["pool"], POOL_SHARDS), _read(feat["held"], HELD_SHARDS)
    at = lambda shards, g, rows: shards[g // rows][g % rows]  # noqa: E731
    _copy(at(held, HELD_TWIN[1], HELD_ROWS), at(held, HELD_TWIN[0], HELD_ROWS))
    _copy(at(held, ZERO_HELD, HELD_ROWS), at(held, ZERO_HELD, HELD_ROWS), zero=True)
    _copy(at(pool, ZERO_POOL, POOL_ROWS), at(pool, ZERO_POOL, POOL_ROWS), zero=True)
    for h, t in PLANTED:
        _copy(at(pool, t, POOL_ROWS), at(held, h, HELD_ROWS))
    _write(feat["pool"], pool)
    _write(feat["held"], held)
    base = dict(feature_path=glob, meta_path=os.path.join(roots["pool"], "videos"), **{"computation.num_workers": 0})
    lloyd = {"clustering.algorithm": "lloyd", "clustering.ncentroids": K, "clustering.epochs": ITERS}
    outs = {}
    for name, more in (("plain", {}), ("white", {"clustering.whiten": True})):
        acav100m_amd.manual_seed(0)
        outs[name] = os.path.join(root, name)
        assert len(Cli().cluster(out_path=outs[name], **base, **lloyd, **more)) == POOL_SHARDS
    before = {name: sorted(os.listdir(out)) for name, out in outs.items()}
    against = {"dedup.against_path": held_glob, "dedup.against_meta_path": os.path.join(roots["held"], "videos")}

    def dedup(name, tag, **more):
        opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": THRESHOLD, "dedup.view": "/".join(VIEW),
                "dedup.out_path": os.path.join(root, tag + ".csv"), "dedup.report_path": os.path.join(root, tag + ".json")}
        opts.update(against)
        opts.update(more)
        opts = {k: v for k, v in opts.items() if v is not None}
        report = Cli().dedup(out_path=outs[name], **base, **opts)
        return report, open(opts["dedup.out_path"], "rb").read(), open(opts["dedup.report_path"], "rb").read()

    first = {name: dedup(name, name + "_first") for name in outs}
    labels = {}
    for name, out in outs.items():  # the pool's labels as the run's assignment shards hold them
        rows = [r for s in range(POOL_SHARDS) for r in pickle.load(open(os.path.join(out, "shard-%06d.pkl" % s), "rb"))]
        labels[name] = np.array([np.int64(r[_kind(VIEW[0]) + "_assignments"][0]["array"][VIEW[1]]) for r in rows])
    return dict(root=root, roots=roots, base=base, outs=outs, before=before, dedup=dedup, first=first, against=against,
                x=_features(pool), y=_features(held), labels=labels, held_glob=held_glob)


def _cache(out_dir):
    import torch
    files = [f for f in os.listdir(out_dir) if f.startswith("cache_epoch_%d_" % (ITERS - 1))]
    assert len(files) == 1
    return torch.load(os.path.join(out_dir, files[0]), map_location="cpu", weights_only=False)[VIEW[0]][VIEW[1]]


def _held_labels(run, name, y):
    """calc_best of the cached state on the held-out rows (after the cache's front-end): the labels the verb blocks with"""
    import torch
    from acav100m_amd.clustering import KMeans
    km = KMeans.load(_cache(run["outs"][name]))
    km.args = None
    lab, _ = km.to("cuda").calc_best(torch.from_numpy(y).cuda(), need_mean=False)
    return lab.cpu().numpy().astype(np.int64) if hasattr(lab, "cpu") else np.asarray(lab, np.int64)


EXTRA = {"view", "epoch", "feature_path", "clusters_path", "against_path", "blocking", "pool_zero_rows", "against_zero_rows"}


def _check(run, result, x, y, lx=None, ly=None):
    """the csv and the json of one dedup against the restatement on the pool rows x and the held-out rows y"""
    from acav100m_amd.clustering.dedup import summarise_against
    d = x.shape[1]
    best, partner, _second = R.nearest_in(x, y, lx, ly)
    copies = np.array(sorted(t for _, t in PLANTED))
    others = np.setdiff1d(np.arange(len(x)), copies)
    print("largest best of an unplanted pool row {:.4f}".format(best[others].max()))
    assert best[others].max() < 0.99  # no unplanted row comes near the threshold
    report, csv_bytes, json_bytes = result
    lines = list(csv.reader(csv_bytes.decode().splitlines()))
    source = dict((t, h) for h, t in PLANTED)
    assert source[199] == HELD_TWIN[0]  # the copy of the held-out twins names the lower one
    assert [tuple(ln[:4]) for ln in lines] == [_name(t, POOL_ROWS) + _name(source[t], HELD_ROWS) for t in copies]  # global row order
    for ln, t in zip(lines, copies):
        assert len(ln) == 5 and ln[4] == repr(float(ln[4])) and abs(float(ln[4]) - 1.0) <= R.bound(d)
        assert abs(float(ln[4]) - best[t]) <= R.bound(d) and partner[t] == source[t]
    blocked = lx is not None
    want = summarise_against(best, partner, lx, np.bincount(ly, minlength=K) if blocked else None, K if blocked else 1, THRESHOLD, len(y))
    assert want["flagged"] == 13 and want["n"] == POOL_SHARDS * POOL_ROWS and want["m"] == HELD_SHARDS * HELD_ROWS
    loaded = json.loads(json_bytes)
    assert {k: loaded[k] for k in want} == json.loads(json.dumps(want))
    assert set(loaded) == set(want) | EXTRA
    assert loaded["view"] == "/".join(VIEW) and loaded["epoch"] == ITERS - 1 and loaded == json.loads(json.dumps(report))
    assert loaded["against_path"] == run["held_glob"] and loaded["blocking"] == ("cluster" if blocked else "none")
    assert loaded["pool_zero_rows"] == 1 and loaded["against_zero_rows"] == 1
    return want


def test_the_csv_names_the_13_copies_and_the_json_is_the_restatements(run):
    want = _check(run, run["first"]["plain"], run["x"][VIEW], run["y"][VIEW])
    assert want["pairs"] == 600 * 120 and want["without_candidates"] == 0 and "flagged_by_cluster" not in want


def test_blocking_cluster_flags_the_same_13_and_reports_the_restatements_pairs(run):
    x, y = run["x"][VIEW], run["y"][VIEW]
    lx, ly = run["labels"]["plain"], _held_labels(run, "plain", y)
    assert all(lx[t] == ly[h] for h, t in PLANTED)  # a bitwise copy gets its source's label
    result = run["dedup"]("plain", "plain_cluster", **{"dedup.blocking": "cluster"})
    want = _check(run, result, x, y, lx, ly)
    hist_x, hist_y = np.bincount(lx, minlength=K), np.bincount(ly, minlength=K)
    assert want["pairs"] == int((hist_x * hist_y).sum()) < 600 * 120 and sum(want["flagged_by_cluster"]) == 13
    print("pairs {} without_candidates {}".format(want["pairs"], want["without_candidates"]))
    again = run["dedup"]("plain", "plain_cluster_streamed", **{"dedup.blocking": "cluster", "data.resident_bytes": _one_shard_budget()})
    assert again[1:] == result[1:]


def _one_shard_budget():
    return int(2.5 * POOL_ROWS * 4 * sum(DIMS.values()))  # the pool streams one shard per group, the held-out set is resident


def test_a_whitened_cache_is_compared_in_its_own_space(run):
    std = np.asarray(_cache(run["outs"]["white"])["whiten_std"], np.float32)
    x, y = run["x"][VIEW] / std, run["y"][VIEW] / std  # one fp32 division per element, like the run's, on both sets
    assert x.dtype == np.float32 and not np.array_equal(std, np.ones_like(std))
    _check(run, run["first"]["white"], x, y)


def test_a_second_run_and_a_streamed_pool_change_no_byte(run):
    _report, csv_bytes, json_bytes = run["first"]["plain"]
    again = run["dedup"]("plain", "plain_again")
    assert again[1] == csv_bytes and again[2] == json_bytes
    streamed = run["dedup"]("plain", "plain_streamed", **{"data.resident_bytes": _one_shard_budget()})
    assert streamed[1] == csv_bytes and streamed[2] == json_bytes
    assert run["dedup"]("plain", "plain_again")[1] == csv_bytes  # an existing file is overwritten, not appended to


def test_the_exclude_reader_accepts_the_csv(run):
    from acav100m_amd.subset_selection import exclude
    listed = exclude.read_exclude(os.path.join(run["root"], "plain_first.csv"))
    assert listed == {(s, os.path.splitext(f)[0]) for s, f in (_name(t, POOL_ROWS) for _, t in PLANTED)} and len(listed) == 13


def test_without_against_path_the_verb_is_the_in_cluster_dedup(run):
    from acav100m_amd.clustering.dedup import summarise
    result = run["dedup"]("plain", "plain_inside", **{"dedup.against_path": None, "dedup.against_meta_path": None})
    x, lab = run["x"][VIEW], run["labels"]["plain"]
    best, partner, _second = RN.nearest_earlier(x, lab, K)
    flagged = np.flatnonzero(best >= THRESHOLD)
    assert flagged.tolist() == [400, 402]  # the later copies of the held-out rows 3 and 60; their first copies are 150 and 17
    lines = list(csv.reader(result[1].decode().splitlines()))
    assert [tuple(ln[:4]) for ln in lines] == [_name(400, POOL_ROWS) + _name(150, POOL_ROWS), _name(402, POOL_ROWS) + _name(17, POOL_ROWS)]
    for ln, t in zip(lines, flagged):
        assert ln[4] == repr(float(ln[4])) and abs(float(ln[4]) - best[t]) <= RN.bound(x.shape[1])
    want = summarise(best, partner, lab, K, THRESHOLD)
    loaded = json.loads(result[2])
    assert {k: loaded[k] for k in want} == json.loads(json.dumps(want))
    assert set(loaded) == set(want) | {"view", "epoch", "feature_path", "clusters_path"}


def test_the_refusals(run, tmp_path, golden_dir):
    import synth
    from acav100m_amd.clustering.cli import Cli
    no_csv = os.path.join(run["root"], "no.csv")
    opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": THRESHOLD, "dedup.view": "/".join(VIEW), "dedup.out_path": no_csv}
    call = lambda **more: Cli().dedup(out_path=run["outs"]["plain"], **run["base"], **dict(opts, **more))  # noqa: E731
    held = run["against"]
    with pytest.raises(ValueError, match="against_meta_path"):
        call(**{"dedup.against_path": held["dedup.against_path"]})
    with pytest.raises(ValueError, match="only valid with"):
        call(**{"dedup.blocking": "cluster"})
    with pytest.raises(ValueError, match="dedup.blocking"):
        call(**dict(held, **{"dedup.blocking": "nprobe"}))
    # another width of the view, and a held-out set that lacks the view the cache was clustered on
    narrow = synth.write_feature_shards(str(tmp_path / "narrow"), n_shards=1, rows=20, seed=5, comps=3, audio_dims=[16], video_dims=[40])
    with pytest.raises(ValueError, match="16 columns in the held-out shards and 24"):
        call(**{"dedup.against_path": narrow, "dedup.against_meta_path": str(tmp_path / "narrow" / "videos")})
    other = synth.write_feature_shards(str(tmp_path / "other"), n_shards=1, rows=20, seed=5, comps=3, audio_dims=[24, 24], video_dims=[40])
    rows = pickle.load(open(str(tmp_path / "other" / "features" / "shard-000000.pkl"), "rb"))
    for r in rows:
        r["audio_features"][0]["array"].pop("layer_0")
    with open(str(tmp_path / "other" / "features" / "shard-000000.pkl"), "wb") as f:
        pickle.dump(rows, f)
    with pytest.raises(ValueError, match="hold no view layer_vggish/layer_0"):
        call(**{"dedup.against_path": other, "dedup.against_meta_path": str(tmp_path / "other" / "videos")})
    # an empty held-out set: no shard of the glob has metadata
    (tmp_path / "nometa").mkdir()
    with pytest.raises(ValueError, match="held-out set is empty"):
        call(**{"dedup.against_path": held["dedup.against_path"], "dedup.against_meta_path": str(tmp_path / "nometa")})
    assert not os.path.exists(no_csv)


def test_nothing_appears_in_the_cluster_directory(run):
    for name, out in run["outs"].items():
        assert sorted(os.listdir(out)) == run["before"][name]
