"""GPU: `clustering.cli dedup --dedup.groups=True` after `clustering.cli cluster` (lloyd, K = 4, 3 iterations) on three synthetic
shards with two views (24 and 40 columns, 200 rows each) into which groups of noisy copies were planted: an a / b / c group whose
two earlier rows are apart (the plain verb keeps two of its rows, the groups verb one), a group of five rows across two shards,
three bitwise copies.  The csv, the groups csv and the json are the restatement's (tests/_dupgroups_np.py) on the assignment
shards' labels, keep=central keeps the row the restated distances name, a second run and a streamed run change no byte, the verb
without dedup.groups writes what it wrote before, the refusals, nothing appears in the cluster directory, and `subset_selection.cli
run --exclude_path=<that csv>` drops exactly the rows that are not kept."""
import csv
import json
import os
import pickle
import random
import sys

import numpy as np
import pytest

from tests import _dupgroups_np as G
from tests import _neardup_np as R

pytestmark = pytest.mark.gpu

N_SHARDS, ROWS = 3, 200
SHARDS = ["shard-%06d.pkl" % s for s in range(N_SHARDS)]
DIMS = {("layer_vggish", "layer_0"): 24, ("layer_slow_fast", "layer_0"): 40}
VIEW = ("layer_vggish", "layer_0")
K, ITERS, THRESHOLD = 4, 3, 0.99
ABC = (30, 95, 170)              # a < b < c: a and b are c moved by 0.12 |c| along +u and -u, u a unit vector orthogonal to c:
#                                  cos(a, c) = cos(b, c) = 1 / sqrt(1 + 0.12^2) = 0.9929, cos(a, b) = (1 - 0.12^2) / (1 + 0.12^2) = 0.9716
FIVE = (50, 120, 180, 230, 390)  # row 50 and four copies with noise of norm 0.03 |x|: every pair above 0.998; two shards
COPIES = [(3, 150), (77, 402), (250, 398)]  # bitwise


def _name(g):
    return "shard-%06d" % (g // ROWS), "vid%09d_010.mp4" % g


def _column(dir_, field, cast):
    out = {v: [] for v in DIMS}
    for name in SHARDS:
        rows = pickle.load(open(os.path.join(dir_, name), "rb"))
        for (mk, layer) in DIMS:
            kind = "audio" if mk == "layer_vggish" else "video"
            out[mk, layer].append(np.stack([cast(r[kind + field][0]["array"][layer]) for r in rows]))
    return {v: np.concatenate(parts) for v, parts in out.items()}


@pytest.fixture(scope="module")
def run(tmp_path_factory, golden_dir):
    """the shards with their planted groups, a Lloyd run, the groups dedup and the plain dedup of one view -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    root = str(tmp_path_factory.mktemp("acav_dedup_groups_cli"))
    glob = synth.write_feature_shards(root, n_shards=N_SHARDS, rows=ROWS, seed=2, comps=6, audio_dims=[24], video_dims=[40])
    feat = os.path.join(root, "features")
    shards = [pickle.load(open(os.path.join(feat, name), "rb")) for name in SHARDS]
    array = lambda g: shards[g // ROWS][g % ROWS]["audio_features"][0]["array"]  # noqa: E731
    rs = np.random.RandomState(11)
    a, b, c = ABC
    src = array(c)[VIEW[1]].astype(np.float64)
    u = rs.randn(len(src))
    u -= src * (u @ src) / (src @ src)
    u *= 0.12 * np.linalg.norm(src) / np.linalg.norm(u)
    array(a)[VIEW[1]], array(b)[VIEW[1]] = (src + u).astype(np.float32), (src - u).astype(np.float32)
    src = array(FIVE[0])[VIEW[1]].astype(np.float64)
    for g in FIVE[1:]:
        v = rs.randn(len(src))
        array(g)[VIEW[1]] = (src + v * (0.03 * np.linalg.norm(src) / np.linalg.norm(v))).astype(np.float32)
    for s, t in COPIES:
        array(t)[VIEW[1]] = array(s)[VIEW[1]].copy()
    for name, rows in zip(SHARDS, shards):
        with open(os.path.join(feat, name), "wb") as f:
            pickle.dump(rows, f)
    base = dict(feature_path=glob, meta_path=os.path.join(root, "videos"), **{"computation.num_workers": 0})
    lloyd = {"clustering.algorithm": "lloyd", "clustering.ncentroids": K, "clustering.epochs": ITERS}
    acav100m_amd.manual_seed(0)
    out = os.path.join(root, "plain")
    assert len(Cli().cluster(out_path=out, **base, **lloyd)) == N_SHARDS
    before = sorted(os.listdir(out))

    def dedup(tag, **more):
        opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": THRESHOLD, "dedup.view": "/".join(VIEW),
                "dedup.out_path": os.path.join(root, tag + ".csv"), "dedup.report_path": os.path.join(root, tag + ".json")}
        opts.update(more)
        report = Cli().dedup(out_path=out, **base, **opts)
        files = [open(opts["dedup.out_path"], "rb").read(), open(opts["dedup.report_path"], "rb").read()]
        if "dedup.groups_path" in opts:
            files.append(open(opts["dedup.groups_path"], "rb").read())
        return [report] + files

    groups = lambda tag, **more: dedup(tag, **{"dedup.groups": True, "dedup.groups_path": os.path.join(root, tag + "_groups.csv")},  # noqa: E731
                                       **more)
    x = _column(feat, "_features", lambda a: np.asarray(a, np.float32))[VIEW]
    lab = _column(out, "_assignments", np.int64)[VIEW]
    # the restatement, once: the pairs, their components, the nearest-earlier rule
    offsets, pair_j, pair_cos, margin = G.pairs(x, lab, THRESHOLD)
    print("nearest cosine to the threshold {:.3g}, bound {:.3g}".format(margin, R.bound(x.shape[1])))
    assert margin > 4 * R.bound(x.shape[1]), "the restatement does not decide every pair"
    root_ = G.components(len(lab), offsets, pair_j)
    best, partner, _second = R.nearest_earlier(x, lab, K)
    return dict(root=root, base=base, out=out, before=before, dedup=dedup, groups=groups, x=x, lab=lab, offsets=offsets, pair_j=pair_j,
                pair_cos=pair_cos, comp=root_, best=best, partner=partner, first=groups("groups_first"), plain=dedup("plain_first"))


def _expect_csv(run, kept):
    """(lines of dedup.out_path, lines of dedup.groups_path) of the restated groups with `kept`; the similarity as a float"""
    comp, n = run["comp"], len(run["lab"])
    size = np.bincount(comp, minlength=n)
    kept_of = {int(comp[i]): int(i) for i in np.flatnonzero(kept)}
    sim = np.full(n, -np.inf)
    later = np.repeat(np.arange(n), np.diff(run["offsets"]))
    np.maximum.at(sim, later, run["pair_cos"])
    np.maximum.at(sim, run["pair_j"], run["pair_cos"])
    removed = [(_name(i) + _name(kept_of[int(comp[i])]), sim[i], int(size[comp[i]])) for i in np.flatnonzero(~kept)]
    members = [i for g in np.flatnonzero(size >= 2) for i in np.flatnonzero(comp == g)]
    return removed, [[str(comp[i]), str(size[comp[i]]), str(int(kept[i]))] + list(_name(i)) for i in members]


def _check_files(run, files, kept, keep):
    from acav100m_amd.clustering.dedup import summarise_groups
    report, csv_bytes, json_bytes, groups_bytes = files
    d = run["x"].shape[1]
    removed, members = _expect_csv(run, kept)
    lines = list(csv.reader(csv_bytes.decode().splitlines()))
    assert [tuple(ln[:4]) for ln in lines] == [names for names, _sim, _size in removed]  # global row order
    for ln, (_names, sim, size) in zip(lines, removed):
        assert len(ln) == 6 and ln[4] == repr(float(ln[4])) and abs(float(ln[4]) - sim) <= R.bound(d) and ln[5] == str(size)
    assert list(csv.reader(groups_bytes.decode().splitlines())) == members
    want = summarise_groups(run["best"], run["partner"], run["lab"], K, THRESHOLD, run["offsets"], run["comp"], kept, keep)
    loaded = json.loads(json_bytes)
    assert {k: loaded[k] for k in want} == json.loads(json.dumps(want))
    assert set(loaded) == set(want) | {"view", "epoch", "feature_path", "clusters_path"}
    assert loaded["view"] == "/".join(VIEW) and loaded["epoch"] == ITERS - 1 and loaded == json.loads(json.dumps(report))
    return loaded


def test_the_planted_groups_are_what_the_restatement_sees(run):
    comp, lab = run["comp"], run["lab"]
    a, b, c = ABC
    assert len({lab[i] for i in ABC}) == 1 and len({lab[i] for i in FIVE}) == 1 and all(lab[s] == lab[t] for s, t in COPIES)
    assert np.flatnonzero(comp == a).tolist() == list(ABC) and np.flatnonzero(comp == FIVE[0]).tolist() == list(FIVE)
    row = lambda i: run["pair_j"][run["offsets"][i]:run["offsets"][i + 1]].tolist()  # noqa: E731
    assert row(b) == [] and row(c) == [a, b]  # a and b are apart: only c has earlier partners
    assert [row(g) for g in FIVE] == [list(FIVE[:i]) for i in range(5)]  # every pair of the five
    assert int(run["offsets"][-1]) == 2 + 10 + len(COPIES) and len(G.groups_as_sets(comp)) == 2 + len(COPIES)
    # the nearest-earlier rule flags c and keeps a and b; the groups keep a alone
    flagged = run["best"] >= THRESHOLD
    assert flagged[list(ABC)].tolist() == [False, False, True]


def test_the_csv_the_groups_csv_and_the_json_are_the_restatements(run, capsys):
    kept = G.choose_kept(run["comp"], 'first')
    loaded = _check_files(run, run["first"], kept, 'first')
    assert (loaded["pairs"], loaded["groups"], loaded["removed"], loaded["removed_beyond_nearest_rule"]) == (15, 5, 9, 1)
    assert loaded["group_size_counts"] == {"2": 3, "3-4": 1, "5-8": 1} and loaded["keep"] == "first"
    assert loaded["largest_groups"][:2] == [dict(size=5, cluster=int(run["lab"][50]), kept=50), dict(size=3, cluster=int(run["lab"][30]), kept=30)]
    removed = {ln[1] for ln in csv.reader(run["first"][1].decode().splitlines())}
    assert _name(ABC[1])[1] in removed and _name(ABC[2])[1] in removed and _name(ABC[0])[1] not in removed
    # the plain verb keeps two rows of the a / b / c group
    plain = {ln[1] for ln in csv.reader(run["plain"][1].decode().splitlines())}
    assert [_name(i)[1] in plain for i in ABC] == [False, False, True] and len(plain) == 8


def test_keep_central_keeps_the_row_the_restated_distances_name(run):
    import torch
    files = [f for f in os.listdir(run["out"]) if f.startswith("cache_epoch_%d_" % (ITERS - 1))]
    assert len(files) == 1
    dt = torch.load(os.path.join(run["out"], files[0]), map_location="cpu", weights_only=False)[VIEW[0]][VIEW[1]]
    centers = np.asarray(dt["centers"], np.float64)
    a2 = ((run["x"].astype(np.float64) - centers[run["lab"]]) ** 2).sum(1)
    comp = run["comp"]
    for g in np.unique(comp):  # the restated distances decide every group: apart by far more than their rounding, or bitwise ties
        m = np.flatnonzero(comp == g)
        if len(m) > 1:
            v = np.sort(a2[m])
            assert v[1] - v[0] > 1e-9 * v[1] or np.array_equal(run["x"][m[0]], run["x"][m[np.argsort(a2[m], kind='stable')[1]]])
    kept = G.choose_kept(comp, 'central', a2)
    for s, t in COPIES:  # a tie: the lower position
        assert kept[s] and not kept[t]
    assert not np.array_equal(kept, G.choose_kept(comp, 'first'))  # some group's central row is not its first
    _check_files(run, run["groups"]("groups_central", **{"dedup.keep": "central"}), kept, 'central')


def test_a_second_run_and_a_streamed_run_change_no_byte(run):
    again = run["groups"]("groups_again")
    assert again[1:] == run["first"][1:]
    shard_bytes = ROWS * 4 * sum(DIMS.values())
    streamed = run["groups"]("groups_streamed", **{"data.resident_bytes": int(2.5 * shard_bytes)})  # one shard per group
    assert streamed[1:] == run["first"][1:]
    assert run["groups"]("groups_again")[1:] == run["first"][1:]  # existing files are overwritten, not appended to


def test_without_the_key_the_verb_writes_what_it_wrote_before(run):
    """the bytes of the plain verb, rebuilt here from nearest_earlier and summarise as the verb of the parent commit wrote them:
    five columns, the json without a groups key -- and a groups run in between changes nothing about them"""
    from acav100m_amd.clustering.dedup import nearest_earlier, summarise
    best, partner = nearest_earlier(run["x"], run["lab"], K)
    want = "".join(",".join(_name(i) + _name(int(partner[i])) + (repr(float(best[i])),)) + "\r\n" for i in np.flatnonzero(best >= THRESHOLD))
    report = summarise(best, partner, run["lab"], K, THRESHOLD)
    loaded = json.loads(run["plain"][2])
    report.update(view="/".join(VIEW), epoch=ITERS - 1, feature_path=loaded["feature_path"], clusters_path=loaded["clusters_path"])
    assert run["plain"][1].decode() == want and run["plain"][2].decode() == json.dumps(report, indent=1)
    assert run["dedup"]("plain_again")[1:] == run["plain"][1:]
    assert run["dedup"]("plain_false", **{"dedup.groups": False})[1:] == run["plain"][1:]


def test_the_refusals(run):
    from acav100m_amd.clustering.cli import Cli
    opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": THRESHOLD, "dedup.view": "/".join(VIEW),
            "dedup.out_path": os.path.join(run["root"], "no.csv")}
    for more, match in (({"dedup.keep": "central"}, "only valid with --dedup.groups=True"),
                        ({"dedup.max_pairs": 100}, "only valid with --dedup.groups=True"),
                        ({"dedup.groups_path": os.path.join(run["root"], "no_groups.csv")}, "only valid with --dedup.groups=True"),
                        ({"dedup.groups": True, "dedup.probes": 2}, "follow-up"),
                        ({"dedup.groups": True, "dedup.against_path": run["base"]["feature_path"],
                          "dedup.against_meta_path": run["base"]["meta_path"]}, "bipartite"),
                        ({"dedup.groups": True, "dedup.keep": "last"}, "dedup.keep"),
                        ({"dedup.groups": True, "dedup.max_pairs": 14}, "15 pairs .* more than max_pairs = 14")):
        with pytest.raises(ValueError, match=match):
            Cli().dedup(out_path=run["out"], **run["base"], **dict(opts, **more))
    assert not os.path.exists(os.path.join(run["root"], "no.csv")) and not os.path.exists(os.path.join(run["root"], "no_groups.csv"))
    at_the_limit = run["groups"]("groups_limit", **{"dedup.max_pairs": 15})
    assert at_the_limit[1] == run["first"][1]


def test_nothing_appears_in_the_cluster_directory(run):
    assert sorted(os.listdir(run["out"])) == run["before"]


def test_the_selection_drops_exactly_the_rows_that_are_not_kept(run):
    import acav100m_amd
    from acav100m_amd import shards as io
    from acav100m_amd.subset_selection import exclude
    from acav100m_amd.subset_selection.cli import Cli
    root, out = run["root"], run["out"]
    dups = os.path.join(root, "groups_first.csv")
    kept = G.choose_kept(run["comp"], 'first')
    _a, _types, shard_names, filenames = io.load_assignment_shards([os.path.join(out, name) for name in SHARDS])
    listed = exclude.read_exclude(dups)
    keep, unknown = exclude.keep_mask(listed, shard_names, filenames)
    assert unknown == 0 and np.array_equal(keep, kept) and len(listed) == int((~kept).sum()) == 9
    acav100m_amd.manual_seed(0)
    random.seed(0)
    csv_path = os.path.join(root, "sel_groups", "output.csv")
    Cli().run(shards_path=os.path.join(out, "shard-{000000..%06d}.pkl" % (N_SHARDS - 1)), meta_path=os.path.join(root, "videos"),
              out_path=csv_path, exclude_path=dups)
    lines = list(csv.reader(open(csv_path, newline='')))
    assert not {(ln[0], os.path.splitext(ln[1])[0]) for ln in lines} & listed
    assert len(lines) == round(0.2 * (N_SHARDS * ROWS - 9))
