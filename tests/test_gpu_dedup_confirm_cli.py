"""GPU: `clustering.cli dedup --dedup.groups=True --dedup.confirm_view= --dedup.confirm_threshold=` after `clustering.cli cluster`
(lloyd, K = 4, 3 iterations) on three synthetic shards with two views (audio 24 and video 40 columns, 200 rows each).  Planted:
a group of five and two pairs copied with small noise in BOTH views, four pairs copied in the audio view only (their video rows
of different mixture components), three pairs copied in the video view only.  With view = audio, confirm_view = video, t = 0.99
and t2 = 0.9 the csv, the groups csv and the json are the restatement's (tests/_dupconfirm_np.py) on the assignment shards'
labels; the audio-only pairs are counted before the confirmation and are in no group, the video-only pairs appear nowhere; a
second run and a streamed run change no byte; without the two keys the verb writes the bytes of the groups mode; the refusals;
nothing appears in the cluster directory; the selection drops exactly the removed rows; a run without a pair in view A skips
the second pass and writes empty files."""
import csv
import json
import os
import pickle
import random
import sys

import numpy as np
import pytest

from tests import _dupconfirm_np as F
from tests import _dupgroups_np as G
from tests import _neardup_np as R

pytestmark = pytest.mark.gpu

N_SHARDS, ROWS = 3, 200
SHARDS = ["shard-%06d.pkl" % s for s in range(N_SHARDS)]
DIMS = {("layer_vggish", "layer_0"): 24, ("layer_slow_fast", "layer_0"): 40}
AUDIO, VIDEO = ("layer_vggish", "layer_0"), ("layer_slow_fast", "layer_0")
K, ITERS, T, T2 = 4, 3, 0.99, 0.9
NOISE = 0.03                     # of |x|: a copy lies at cosine 1 / sqrt(1 + 0.03^2) = 0.99955 of its source, two copies at 0.9991
FIVE = (50, 120, 180, 230, 390)  # row 50 and four noisy copies, in both views; two shards
BOTH = [(3, 150), (77, 402)]     # (source, copy) in both views
AUDIO_ONLY = [(10, 210), (21, 305), (140, 441), (260, 520)]  # the video rows stay what they were: other mixture components
VIDEO_ONLY = [(15, 333), (88, 455), (199, 577)]              # the audio rows stay what they were


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


def _plant(root, golden_dir):
    """the three shards with the planted copies; returns the shard glob"""
    sys.path.insert(0, golden_dir)
    import synth
    glob = synth.write_feature_shards(root, n_shards=N_SHARDS, rows=ROWS, seed=2, comps=6, audio_dims=[24], video_dims=[40])
    feat = os.path.join(root, "features")
    shards = [pickle.load(open(os.path.join(feat, name), "rb")) for name in SHARDS]
    rs = np.random.RandomState(17)

    def copy(s, t, kinds):
        for kind, layer in kinds:
            src = shards[s // ROWS][s % ROWS][kind + "_features"][0]["array"][layer].astype(np.float64)
            v = rs.randn(len(src))
            shards[t // ROWS][t % ROWS][kind + "_features"][0]["array"][layer] = (
                src + v * (NOISE * np.linalg.norm(src) / np.linalg.norm(v))).astype(np.float32)

    both = (("audio", AUDIO[1]), ("video", VIDEO[1]))
    for g in FIVE[1:]:
        copy(FIVE[0], g, both)
    for s, t in BOTH:
        copy(s, t, both)
    for s, t in AUDIO_ONLY:
        copy(s, t, both[:1])
    for s, t in VIDEO_ONLY:
        copy(s, t, both[1:])
    for name, rows in zip(SHARDS, shards):
        with open(os.path.join(feat, name), "wb") as f:
            pickle.dump(rows, f)
    return glob


@pytest.fixture(scope="module")
def run(tmp_path_factory, golden_dir):
    """the shards with their planted copies, a Lloyd run, the confirmed dedup, the groups dedup without the keys -- once"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    from acav100m_amd.clustering.cli import Cli
    root = str(tmp_path_factory.mktemp("acav_dedup_confirm_cli"))
    glob = _plant(root, golden_dir)
    feat = os.path.join(root, "features")
    base = dict(feature_path=glob, meta_path=os.path.join(root, "videos"), **{"computation.num_workers": 0})
    lloyd = {"clustering.algorithm": "lloyd", "clustering.ncentroids": K, "clustering.epochs": ITERS}
    acav100m_amd.manual_seed(0)
    out = os.path.join(root, "plain")
    assert len(Cli().cluster(out_path=out, **base, **lloyd)) == N_SHARDS
    before = sorted(os.listdir(out))

    def dedup(tag, **more):
        opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": T, "dedup.view": "/".join(AUDIO), "dedup.groups": True,
                "dedup.out_path": os.path.join(root, tag + ".csv"), "dedup.report_path": os.path.join(root, tag + ".json"),
                "dedup.groups_path": os.path.join(root, tag + "_groups.csv")}
        opts.update(more)
        report = Cli().dedup(out_path=out, **base, **opts)
        return [report] + [open(opts[key], "rb").read() for key in ("dedup.out_path", "dedup.report_path", "dedup.groups_path")]

    confirm = lambda tag, **more: dedup(tag, **{"dedup.confirm_view": "/".join(VIDEO), "dedup.confirm_threshold": T2}, **more)  # noqa: E731
    x = _column(feat, "_features", lambda a: np.asarray(a, np.float32))
    lab = _column(out, "_assignments", np.int64)[AUDIO]
    # the restatement, once: view A's pairs, the filter, the components before and after, the nearest-earlier rule of view A
    offsets_a, pair_j_a, _cos_a, _margin = G.pairs(x[AUDIO], lab, T)
    offsets, pair_j, pair_cos, cos_b, margin, margin_b = F.confirmed(x[AUDIO], x[VIDEO], lab, T, T2)
    print("nearest cosine to the thresholds: {:.3g} in view A (bound {:.3g}), {:.3g} in view B (bound {:.3g})".format(
        margin, R.bound(24), margin_b, R.bound(40)))
    assert margin > 4 * R.bound(24) and margin_b > 4 * R.bound(40), "the restatement does not decide every pair"
    best, partner, _second = R.nearest_earlier(x[AUDIO], lab, K)
    return dict(root=root, base=base, out=out, before=before, dedup=dedup, confirm=confirm, x=x, lab=lab, offsets_a=offsets_a,
                pair_j_a=pair_j_a, offsets=offsets, pair_j=pair_j, pair_cos=pair_cos, cos_b=cos_b,
                comp_a=G.components(len(lab), offsets_a, pair_j_a), comp=G.components(len(lab), offsets, pair_j), best=best,
                partner=partner, first=confirm("confirm_first"), groups=dedup("groups_first"))


def _pairs_of(offsets, pair_j):
    later = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return {(int(j), int(i)) for i, j in zip(later, pair_j)}


def test_the_planted_pairs_are_what_the_restatement_sees(run):
    before, after = _pairs_of(run["offsets_a"], run["pair_j_a"]), _pairs_of(run["offsets"], run["pair_j"])
    five = {(a, b) for i, a in enumerate(FIVE) for b in FIVE[i + 1:]}
    assert before == five | set(BOTH) | set(AUDIO_ONLY) and after == five | set(BOTH)
    assert (run["cos_b"] >= T2).sum() == 12 and (run["cos_b"] < 0.5).sum() == len(AUDIO_ONLY)  # the video rows are independent
    groups = G.groups_as_sets(run["comp"])
    assert groups == {frozenset(FIVE)} | {frozenset(p) for p in BOTH}
    assert G.groups_as_sets(run["comp_a"]) == groups | {frozenset(p) for p in AUDIO_ONLY}
    in_a_group = set().union(*groups)
    assert not in_a_group & {g for p in AUDIO_ONLY + VIDEO_ONLY for g in p}


def _check_files(run, files, kept, keep='first'):
    from acav100m_amd.clustering.dedup import SIMILARITY_GRID, summarise_groups
    report, csv_bytes, json_bytes, groups_bytes = files
    comp, n = run["comp"], len(run["lab"])
    size = np.bincount(comp, minlength=n)
    kept_of = {int(comp[i]): int(i) for i in np.flatnonzero(kept)}
    sim = np.full(n, -np.inf)  # of view A, over the confirmed pairs
    later = np.repeat(np.arange(n), np.diff(run["offsets"]))
    np.maximum.at(sim, later, run["pair_cos"])
    np.maximum.at(sim, run["pair_j"], run["pair_cos"])
    removed = np.flatnonzero(~kept)
    lines = list(csv.reader(csv_bytes.decode().splitlines()))
    assert [tuple(ln[:4]) for ln in lines] == [_name(i) + _name(kept_of[int(comp[i])]) for i in removed]  # global row order
    for ln, i in zip(lines, removed):
        assert len(ln) == 6 and ln[4] == repr(float(ln[4])) and abs(float(ln[4]) - sim[i]) <= R.bound(24) and ln[5] == str(size[comp[i]])
    members = [i for g in np.flatnonzero(size >= 2) for i in np.flatnonzero(comp == g)]
    assert list(csv.reader(groups_bytes.decode().splitlines())) == [[str(comp[i]), str(size[comp[i]]), str(int(kept[i]))] + list(_name(i))
                                                                   for i in members]
    want = summarise_groups(run["best"], run["partner"], run["lab"], K, T, run["offsets"], comp, kept, keep)
    size_a = np.bincount(run["comp_a"], minlength=n)
    want.update(confirm_view="/".join(VIDEO), confirm_threshold=T2, pairs_before_confirm=int(run["offsets_a"][-1]),
                groups_before_confirm=int((size_a >= 2).sum()), removed_before_confirm=int((size_a[run["comp_a"]] >= 2).sum() - (size_a >= 2).sum()),
                confirm_similarity_counts={repr(g): int((run["cos_b"] >= g).sum()) for g in SIMILARITY_GRID})
    loaded = json.loads(json_bytes)
    assert {k: loaded[k] for k in want} == json.loads(json.dumps(want))
    assert set(loaded) == set(want) | {"view", "epoch", "feature_path", "clusters_path"}
    assert loaded["view"] == "/".join(AUDIO) and loaded["epoch"] == ITERS - 1 and loaded == json.loads(json.dumps(report))
    return loaded


def test_the_csv_the_groups_csv_and_the_json_are_the_restatements(run, capsys):
    loaded = _check_files(run, run["first"], G.choose_kept(run["comp"], 'first'))
    assert (loaded["pairs_before_confirm"], loaded["pairs"], loaded["groups_before_confirm"], loaded["groups"]) == (16, 12, 7, 3)
    assert (loaded["removed_before_confirm"], loaded["removed"]) == (10, 6) and loaded["removed"] < loaded["removed_before_confirm"]
    assert loaded["confirm_similarity_counts"]["0.9"] == 12 and loaded["confirm_similarity_counts"]["0.5"] == 12
    # flagged and the similarity grid stay those of view A alone: the nearest-earlier rule flags the later row of all 16 pairs' rows
    assert loaded["flagged"] == 4 + len(BOTH) + len(AUDIO_ONLY) and loaded["similarity_counts"]["0.99"] == loaded["flagged"]
    names = {ln[1] for ln in csv.reader(run["first"][1].decode().splitlines())} | {ln[4] for ln in csv.reader(run["first"][3].decode().splitlines())}
    assert not names & {_name(g)[1] for p in AUDIO_ONLY + VIDEO_ONLY for g in p}  # in no file
    assert {_name(g)[1] for g in FIVE} <= names


def test_keep_central_uses_view_a(run):
    import torch
    files = [f for f in os.listdir(run["out"]) if f.startswith("cache_epoch_%d_" % (ITERS - 1))]
    dt = torch.load(os.path.join(run["out"], files[0]), map_location="cpu", weights_only=False)[AUDIO[0]][AUDIO[1]]
    centers = np.asarray(dt["centers"], np.float64)
    a2 = ((run["x"][AUDIO].astype(np.float64) - centers[run["lab"]]) ** 2).sum(1)
    for g in np.unique(run["comp"]):  # the restated distances decide every group
        m = np.flatnonzero(run["comp"] == g)
        if len(m) > 1:
            v = np.sort(a2[m])
            assert v[1] - v[0] > 1e-9 * v[1]
    _check_files(run, run["confirm"]("confirm_central", **{"dedup.keep": "central"}), G.choose_kept(run["comp"], 'central', a2), 'central')


def test_a_second_run_and_a_streamed_run_change_no_byte(run, capsys):
    assert run["confirm"]("confirm_again")[1:] == run["first"][1:]
    shard_bytes = ROWS * 4 * sum(DIMS.values())
    capsys.readouterr()
    streamed = run["confirm"]("confirm_streamed", **{"data.resident_bytes": int(2.5 * shard_bytes)})  # one shard per group
    assert "streaming 3 shards in 3 groups" in capsys.readouterr().out
    assert streamed[1:] == run["first"][1:]


def test_without_the_two_keys_the_verb_writes_the_bytes_of_the_groups_mode(run):
    """rebuilt here from pairs_earlier, components and summarise_groups as the verb of the parent commit wrote them -- and a
    confirmed run in between changes nothing about them"""
    from acav100m_amd.clustering.dedup import choose_kept, components, pair_similarity, pairs_earlier, summarise_groups
    x, lab, n = run["x"][AUDIO], run["lab"], len(run["lab"])
    best, partner, offsets, pair_j, pair_cos = pairs_earlier(x, lab, T, K)
    root = components(n, offsets, pair_j)
    kept = choose_kept(root, 'first')
    sim, size = pair_similarity(n, offsets, pair_j, pair_cos), np.bincount(root, minlength=n)
    want = "".join(",".join(_name(i) + _name(int(root[i])) + (repr(float(sim[i])), str(size[root[i]]))) + "\r\n" for i in np.flatnonzero(~kept))
    report = summarise_groups(best, partner, lab, K, T, offsets, root, kept, 'first')
    loaded = json.loads(run["groups"][2])
    report.update(view="/".join(AUDIO), epoch=ITERS - 1, feature_path=loaded["feature_path"], clusters_path=loaded["clusters_path"])
    assert run["groups"][1].decode() == want and run["groups"][2].decode() == json.dumps(report, indent=1)
    assert "confirm_view" not in loaded and loaded["pairs"] == 16 and loaded["removed"] == 10
    assert run["dedup"]("groups_again")[1:] == run["groups"][1:]


def test_the_refusals(run):
    from acav100m_amd.clustering.cli import Cli
    opts = {"clustering.cached_epoch": ITERS - 1, "dedup.threshold": T, "dedup.view": "/".join(AUDIO), "dedup.groups": True,
            "dedup.out_path": os.path.join(run["root"], "no.csv")}
    video = "/".join(VIDEO)
    for more, match in (({"dedup.confirm_view": video}, "go together"),
                        ({"dedup.confirm_threshold": T2}, "go together"),
                        ({"dedup.confirm_view": video, "dedup.confirm_threshold": 0}, "confirm_threshold must be a number in"),
                        ({"dedup.confirm_view": video, "dedup.confirm_threshold": 1.5}, "confirm_threshold must be a number in"),
                        ({"dedup.confirm_view": "video", "dedup.confirm_threshold": T2}, "<model_key>/<layer>"),
                        ({"dedup.confirm_view": "/".join(AUDIO), "dedup.confirm_threshold": T2}, "is dedup.view"),
                        ({"dedup.confirm_view": "layer_slow_fast/layer_9", "dedup.confirm_threshold": T2}, "not a view of the cache"),
                        ({"dedup.confirm_view": video, "dedup.confirm_threshold": T2, "dedup.groups": False},
                         "needs --dedup.groups=True: the confirmed relation is a pair list"),
                        ({"dedup.confirm_view": video, "dedup.confirm_threshold": T2, "dedup.groups": None,
                          "dedup.against_path": run["base"]["feature_path"], "dedup.against_meta_path": run["base"]["meta_path"]},
                         "refused with dedup.against_path")):
        merged = {k: v for k, v in dict(opts, **more).items() if v is not None}
        with pytest.raises(ValueError, match=match):
            Cli().dedup(out_path=run["out"], **run["base"], **merged)
    assert not os.path.exists(os.path.join(run["root"], "no.csv"))


def test_nothing_appears_in_the_cluster_directory(run):
    assert sorted(os.listdir(run["out"])) == run["before"]


def test_the_selection_drops_exactly_the_removed_rows(run):
    import acav100m_amd
    from acav100m_amd import shards as io
    from acav100m_amd.subset_selection import exclude
    from acav100m_amd.subset_selection.cli import Cli
    root, out = run["root"], run["out"]
    dups = os.path.join(root, "confirm_first.csv")
    kept = G.choose_kept(run["comp"], 'first')
    _a, _types, shard_names, filenames = io.load_assignment_shards([os.path.join(out, name) for name in SHARDS])
    listed = exclude.read_exclude(dups)
    keep, unknown = exclude.keep_mask(listed, shard_names, filenames)
    assert unknown == 0 and np.array_equal(keep, kept) and len(listed) == int((~kept).sum()) == 6
    acav100m_amd.manual_seed(0)
    random.seed(0)
    csv_path = os.path.join(root, "sel_confirm", "output.csv")
    Cli().run(shards_path=os.path.join(out, "shard-{000000..%06d}.pkl" % (N_SHARDS - 1)), meta_path=os.path.join(root, "videos"),
              out_path=csv_path, exclude_path=dups)
    lines = list(csv.reader(open(csv_path, newline='')))
    assert not {(ln[0], os.path.splitext(ln[1])[0]) for ln in lines} & listed
    assert len(lines) == round(0.2 * (N_SHARDS * ROWS - 6))


def test_a_run_without_a_pair_in_view_a_skips_the_second_pass(run, monkeypatch):
    """t = 0.9999999: the noisy copies lie at 0.99955 and nothing is bitwise equal, so view A has no pair: no row of view B is
    gathered and no cosine asked for"""
    from acav100m_amd.clustering import dedup as D
    offsets, _pj, _pc, margin = G.pairs(run["x"][AUDIO], run["lab"], 0.9999999)
    assert offsets[-1] == 0 and margin > 4 * R.bound(24)

    def never(*_a, **_k):
        raise AssertionError("the second pass ran")

    monkeypatch.setattr(D, "pair_cosines", never)
    monkeypatch.setattr(D, "pair_rows", never)
    report, csv_bytes, _json, groups_bytes = run["confirm"]("confirm_none", **{"dedup.threshold": 0.9999999})
    assert csv_bytes == b"" and groups_bytes == b""
    assert (report["pairs_before_confirm"], report["pairs"], report["groups"], report["removed"], report["removed_before_confirm"]) == (0,) * 5
    assert not any(report["confirm_similarity_counts"].values()) and report["confirm_view"] == "/".join(VIDEO)
