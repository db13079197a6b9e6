"""GPU: `clustering.cli dedup --dedup.probes=m` after `clustering.cli cluster` (lloyd, K = 4, 3 iterations: the labels are the
plainly nearest centres) on a pool of three synthetic shards (200 rows, views of 24 and 40 columns) and a held-out set of two
(200 rows).  After the run, rows near a bisector of the trained centres get near-copies pushed across it (x_t = x_s + tau (c_b -
c_a), tau = margin / ||c_b - c_a||^2): inside the pool, and from the held-out set into the pool; the pairs the run's own
calc_best splits are the planted ones.  Without the key and with --dedup.probes=1 the verb writes the same bytes, the csv and
json of the in-cluster restatement; with probes the csv lists the planted copies with their sources and the json gains probes,
pairs and flagged_by_probes -- the restatement's (tests/_probedup_np.py); the same against the held-out set with a streamed
pool; `exclude.read_exclude` accepts the csv; the refusals come before anything is read."""
import csv
import json
import os
import pickle
import sys

import numpy as np
import pytest

from tests import _neardup_np as RN
from tests import _probedup_np as R

pytestmark = pytest.mark.gpu

POOL_SHARDS, POOL_ROWS, HELD_SHARDS, HELD_ROWS = 3, 200, 2, 200
DIMS = {("layer_vggish", "layer_0"): 24, ("layer_slow_fast", "layer_0"): 40}
VIEW = ("layer_vggish", "layer_0")
K, ITERS, THRESHOLD = 4, 3, 0.99
TRIED = 8  # near-copies written per mode; the ones calc_best splits, at a cosine clear of the threshold, are the planted pairs


def _name(g, rows):
    return "shard-%06d" % (g // rows), "vid%09d_010.mp4" % g


def _read(dir_, n_shards):
    return [pickle.load(open(os.path.join(dir_, "shard-%06d.pkl" % s), "rb")) for s in range(n_shards)]


def _write(dir_, shards):
    for s, rows in enumerate(shards):
        with open(os.path.join(dir_, "shard-%06d.pkl" % s), "wb") as f:
            pickle.dump(rows, f)


def _view(shards):
    return np.stack([np.asarray(r["audio_features"][0]["array"][VIEW[1]], np.float32) for rows in shards for r in rows])


def _set(shards, g, rows, value):
    shards[g // rows][g % rows]["audio_features"][0]["array"][VIEW[1]] = np.asarray(value, np.float32)


def _across(src, centres, count):
    """the `count` rows of src nearest a bisector, pushed across it: (row numbers, new rows)"""
    D = R.distances(src, centres)
    order = np.argsort(D, axis=1, kind='stable')
    rows = np.arange(len(src))
    margin = D[rows, order[:, 1]] - D[rows, order[:, 0]]
    pick = np.argsort(margin, kind='stable')[:count]
    step = centres[order[pick, 1]].astype(np.float64) - centres[order[pick, 0]].astype(np.float64)
    moved = src[pick].astype(np.float64) + (margin[pick] / (step * step).sum(1))[:, None] * step
    return pick, moved.astype(np.float32)


@pytest.fixture(scope="module")
def run(tmp_path_factory, golden_dir):
    """the two sets, a Lloyd run on the pool, the near-copies planted with its centres, the state and its labels -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering import KMeans
    from acav100m_amd.clustering.cli import Cli
    root = str(tmp_path_factory.mktemp("acav_dedup_probes"))
    roots = {name: os.path.join(root, name) for name in ("pool", "held")}
    glob = synth.write_feature_shards(roots["pool"], n_shards=POOL_SHARDS, rows=POOL_ROWS, seed=2, comps=6, audio_dims=[24],
                                      video_dims=[40])
    held_glob = synth.write_feature_shards(roots["held"], n_shards=HELD_SHARDS, rows=HELD_ROWS, seed=3, comps=6, audio_dims=[24],
                                           video_dims=[40])
    feat = {name: os.path.join(r, "features") for name, r in roots.items()}
    base = dict(feature_path=glob, meta_path=os.path.join(roots["pool"], "videos"), **{"computation.num_workers": 0})
    acav100m_amd.manual_seed(0)
    out = os.path.join(root, "plain")
    assert len(Cli().cluster(out_path=out, **base, **{"clustering.algorithm": "lloyd", "clustering.ncentroids": K,
                                                      "clustering.epochs": ITERS})) == POOL_SHARDS
    files = [f for f in os.listdir(out) if f.startswith("cache_epoch_%d_" % (ITERS - 1))]
    assert len(files) == 1
    km = KMeans.load(torch.load(os.path.join(out, files[0]), map_location="cpu", weights_only=False)[VIEW[0]][VIEW[1]])
    km.args = None
    km = km.to("cuda")
    centres = km.centers.numpy()

    # near-copies of pool rows of the first half at rows of the second half, and of held-out rows at other pool rows
    pool, held = _read(feat["pool"], POOL_SHARDS), _read(feat["held"], HELD_SHARDS)
    x, y = _view(pool), _view(held)
    n = len(x)
    src_in, moved_in = _across(x[:n // 2], centres, TRIED)
    tgt_in = n // 2 + 11 * np.arange(TRIED) + 5
    src_ag, moved_ag = _across(y, centres, TRIED)
    tgt_ag = n // 2 + 11 * np.arange(TRIED) + 9
    for t, v in list(zip(tgt_in, moved_in)) + list(zip(tgt_ag, moved_ag)):
        _set(pool, int(t), POOL_ROWS, v)
    _write(feat["pool"], pool)
    x = _view(pool)
    lx = np.asarray(km.calc_best(x, need_mean=False)[0], np.int64)
    ly = np.asarray(km.calc_best(y, need_mean=False)[0], np.int64)

    def cos(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        return (a @ b) / np.sqrt((a @ a) * (b @ b))

    inside = [(int(s), int(t)) for s, t in zip(src_in, tgt_in) if lx[s] != lx[t] and cos(x[s], x[t]) >= THRESHOLD + 0.001]
    across = [(int(s), int(t)) for s, t in zip(src_ag, tgt_ag) if ly[s] != lx[t] and cos(y[s], x[t]) >= THRESHOLD + 0.001]
    print("planted inside the pool {}, from the held-out set {}".format(inside, across))
    assert len(inside) >= 2 and len(across) >= 2  # the near-duplicate pairs the run's own labels split
    before = sorted(os.listdir(out))

    def dedup(tag, **more):
        opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": THRESHOLD, "dedup.view": "/".join(VIEW),
                "dedup.out_path": os.path.join(root, tag + ".csv"), "dedup.report_path": os.path.join(root, tag + ".json")}
        opts.update(more)
        report = Cli().dedup(out_path=out, **base, **opts)
        return report, open(opts["dedup.out_path"], "rb").read(), open(opts["dedup.report_path"], "rb").read()

    against = {"dedup.against_path": held_glob, "dedup.against_meta_path": os.path.join(roots["held"], "videos"),
               "dedup.blocking": "cluster"}
    return dict(root=root, out=out, base=base, before=before, dedup=dedup, against=against, km=km, centres=centres, x=x, y=y, lx=lx,
                ly=ly, inside=inside, across=across)


def _lines(csv_bytes):
    return list(csv.reader(csv_bytes.decode().splitlines()))


def _check_csv(lines, best, partner, names, partner_names, d):
    flagged = np.flatnonzero(best >= THRESHOLD)
    assert [tuple(ln[:4]) for ln in lines] == [names(t) + partner_names(partner[t]) for t in flagged]  # global row order
    for ln, t in zip(lines, flagged):
        assert len(ln) == 5 and ln[4] == repr(float(ln[4])) and abs(float(ln[4]) - best[t]) <= R.bound(d)
    return flagged


def _pool(g):
    return _name(g, POOL_ROWS)


def _held(g):
    return _name(g, HELD_ROWS)


def _probes(run, m):
    probes, _dist, gap, room = R.probe_centers(run["x"], run["centres"], run["lx"], m)
    assert (gap > 4 * room).all()  # every rank is decided: the kernel's lists are these
    assert np.array_equal(run["km"].probe_centers(run["x"], m, run["lx"]), probes)
    return probes


def test_one_probe_and_no_key_write_the_in_cluster_bytes(run):
    from acav100m_amd.clustering.dedup import summarise
    plain, one = run["dedup"]("plain"), run["dedup"]("one", **{"dedup.probes": 1})
    assert plain[1:] == one[1:]
    x, lx = run["x"], run["lx"]
    best, partner, _second = RN.nearest_earlier(x, lx, K)
    flagged = _check_csv(_lines(plain[1]), best, partner, _pool, _pool, x.shape[1])
    copies = [t for _, t in run["inside"]]
    assert not np.isin(copies, flagged).any()  # the border hides every planted pair from the in-cluster sweep
    want = summarise(best, partner, lx, K, THRESHOLD)
    loaded = json.loads(plain[2])
    assert {k: loaded[k] for k in want} == json.loads(json.dumps(want))
    assert set(loaded) == set(want) | {"view", "epoch", "feature_path", "clusters_path"}  # no new key without probes


def test_three_probes_list_the_planted_copies_with_their_sources(run):
    from acav100m_amd.clustering.dedup import summarise
    from acav100m_amd.subset_selection import exclude
    m = 3
    report, csv_bytes, json_bytes = run["dedup"]("three", **{"dedup.probes": m})
    x, lx = run["x"], run["lx"]
    probes = _probes(run, m)
    best, partner, second, each = R.nearest(x, x, probes, lx, np.arange(len(x)))
    assert (best[partner >= 0] - second[partner >= 0] > 4 * R.bound(x.shape[1])).all()
    lines = _lines(csv_bytes)
    flagged = _check_csv(lines, best, partner, _pool, _pool, x.shape[1])
    listed = {tuple(ln[:4]) for ln in lines}
    for s, t in run["inside"]:
        assert t in flagged and partner[t] == s and lx[s] != lx[t] and _pool(t) + _pool(s) in listed
    want = summarise(best, partner, lx, K, THRESHOLD, probes=probes, best_each=each)
    loaded = json.loads(json_bytes)
    assert {k: loaded[k] for k in want} == json.loads(json.dumps(want)) and loaded == json.loads(json.dumps(report))
    assert set(loaded) == set(want) | {"view", "epoch", "feature_path", "clusters_path"}
    curve = loaded["flagged_by_probes"]
    one = run["dedup"]("one_for_three", **{"dedup.probes": 1})[0]
    assert loaded["probes"] == m and len(curve) == m and curve == sorted(curve) and curve[0] == one["flagged"]
    assert curve[-1] == loaded["flagged"] >= curve[0] + len(run["inside"]) and loaded["pairs"] > 0
    # the selection's exclude reader accepts the file
    read = exclude.read_exclude(os.path.join(run["root"], "three.csv"))
    assert read == {(ln[0], os.path.splitext(ln[1])[0]) for ln in lines} and len(read) == len(lines)
    assert run["dedup"]("three_again", **{"dedup.probes": m})[1:] == (csv_bytes, json_bytes)  # a second run: the same bytes


def test_against_a_held_out_set_with_a_streamed_pool(run):
    from acav100m_amd.clustering.dedup import summarise_against
    m = 2
    x, y, lx, ly = run["x"], run["y"], run["lx"], run["ly"]
    one = run["dedup"]("held_one", **run["against"])
    assert run["dedup"]("held_one_key", **dict(run["against"], **{"dedup.probes": 1}))[1:] == one[1:]
    report, csv_bytes, json_bytes = run["dedup"]("held_two", **dict(run["against"], **{"dedup.probes": m}))
    budget = int(2.5 * POOL_ROWS * 4 * sum(DIMS.values()))  # the pool streams one shard per group, the held-out set is resident
    streamed = run["dedup"]("held_two_streamed", **dict(run["against"], **{"dedup.probes": m, "data.resident_bytes": budget}))
    assert streamed[1:] == (csv_bytes, json_bytes)
    probes = _probes(run, m)
    best, partner, second, each = R.nearest(x, y, probes, ly)
    assert (best[partner >= 0] - second[partner >= 0] > 4 * R.bound(x.shape[1])).all()
    lines = _lines(csv_bytes)
    flagged = _check_csv(lines, best, partner, _pool, _held, x.shape[1])
    first = {tuple(ln[:2]) for ln in _lines(one[1])}
    for s, t in run["across"]:
        assert t in flagged and partner[t] == s and ly[s] != lx[t] and _pool(t) not in first
    want = summarise_against(best, partner, lx, np.bincount(ly, minlength=K), K, THRESHOLD, len(y), probes_x=probes, best_each=each)
    loaded = json.loads(json_bytes)
    assert {k: loaded[k] for k in want} == json.loads(json.dumps(want)) and loaded == json.loads(json.dumps(report))
    curve = loaded["flagged_by_probes"]
    assert loaded["probes"] == m and curve == sorted(curve) and curve[0] == one[0]["flagged"]
    assert curve[-1] == loaded["flagged"] >= curve[0] + len(run["across"]) and loaded["pairs"] > one[0]["pairs"]
    assert "probes" not in one[0] and "flagged_by_probes" not in one[0]


def test_the_refusals_come_before_anything_is_read(run):
    from acav100m_amd.clustering.cli import Cli
    no_csv = os.path.join(run["root"], "no.csv")
    opts = {"clustering.cached_epoch": 99, "dedup.threshold": THRESHOLD, "dedup.view": "/".join(VIEW), "dedup.out_path": no_csv}
    call = lambda **more: Cli().dedup(out_path=run["out"], **run["base"], **dict(opts, **more))  # noqa: E731
    held = dict(run["against"])
    with pytest.raises(ValueError, match="blocking=none"):  # epoch 99 has no cache: it was not looked for
        call(**dict(held, **{"dedup.blocking": "none", "dedup.probes": 2}))
    held.pop("dedup.blocking")
    with pytest.raises(ValueError, match="blocking=none"):
        call(**dict(held, **{"dedup.probes": 2}))
    for bad in (0, 17, True, 2.5):
        with pytest.raises(ValueError, match="dedup.probes must be"):
            call(**{"dedup.probes": bad})
    with pytest.raises(ValueError, match="exceeds the K=4"):  # K is known once the cache is read
        call(**{"dedup.probes": 5, "clustering.cached_epoch": ITERS - 1})
    assert not os.path.exists(no_csv)


def test_nothing_appears_in_the_cluster_directory(run):
    assert sorted(os.listdir(run["out"])) == run["before"]
