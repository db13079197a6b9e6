"""GPU: subset scoring (EfficientBatchMI.score_subset / acav_mi_score_subset, kernels in acav100m_amd/csrc/acav_score.hip)
against sklearn's golden scores (tests/golden/subset_scores.npz), its determinism rules, its isolation from the handle's greedy
state, the measure mask, the argument checks and the `evaluate` verb."""
import csv
import json
import os
import random
import types

import numpy as np
import pytest

from tests import _subset_scores_np as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "subset_scores.npz"))


def _cases():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subset_scores.npz"))
    return g["cases"].tolist()


def _measure(name, a, c, pairs, cand=(), **kw):
    from acav100m_amd.subset_selection import get_measure
    m = get_measure(name)(np.ascontiguousarray(a, dtype=np.int64), ncentroids=c, device="cuda:0", **kw)
    m.init([tuple(p) for p in pairs], [int(i) for i in cand])
    return m


def _case(golden, name):
    assign = golden[str(golden[name + ".assign"])].astype(np.int64)
    return (assign, int(golden[name + ".C"]), golden[name + ".pairs"].tolist(), golden[name + ".ids"].astype(np.int64),
            golden[name + ".prefix"].tolist())


def _scorer(golden, name):
    assign, C, pairs, ids, prefix = _case(golden, name)
    return _measure("batch_mi", assign, C, pairs), ids, prefix


def _same_bits(x, y):
    """two score_subset results (per_pair + stats asked for) are the same bytes"""
    assert set(x) == set(y)
    for k in x:
        if k == "per_pair":
            for m in x[k]:
                assert np.asarray(x[k][m]).tobytes() == np.asarray(y[k][m]).tobytes(), m
        elif k == "stats":
            assert x[k].tobytes() == y[k].tobytes()
        else:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


@pytest.mark.parametrize("name", _cases())
def test_golden_scores(env, golden, name):
    """per (prefix, pair): mutual_info, normalized_mutual_info and both entropies within 1e-9 of sklearn (reordering bound of
    the header: 2^20 terms x 2^-53 x 43 < 5e-9 at the largest table; these tables have <= 9e4 cells); the pair counts equal the
    numpy restatement and adjusted_rand / fowlkes_mallows / rand equal sklearn exactly; adjusted_mutual_info within
    max(100 x the float64 restatement's recorded distance from sklearn, 1e-13) -- room for another exp and summation order on
    the same ln k! table, not for a wrong term.  The mean over the pairs is the plain mean."""
    m, ids, prefix = _scorer(golden, name)
    assign, C, pairs, _, _ = _case(golden, name)
    out = m.score_subset(ids, prefixes=prefix, per_pair=True, return_stats=True)
    sk, dev, h = golden[name + ".sk"], golden[name + ".dev"], golden[name + ".h"]
    worst = dict.fromkeys(R.NAMES, 0.0)
    for q, k in enumerate(prefix):
        for p, (d1, d2) in enumerate(pairs):
            st = out["stats"][q, p]
            want = R.raw_stats(R.table(assign, ids[:k], d1, d2, C), with_emi=False)
            for f in ("tp", "fp", "fn", "tn", "n_rows", "n_cols", "n"):
                assert int(st[f]) == want[f], (name, k, p, f)
            assert abs(st["h_row"] - h[q, p, 0]) <= 1e-9 and abs(st["h_col"] - h[q, p, 1]) <= 1e-9
            for i, mname in enumerate(R.NAMES):
                got = float(out["per_pair"][mname][q, p])
                d = abs(got - sk[q, p, i])
                worst[mname] = max(worst[mname], d)
                where = "{} prefix {} pair {} {}: {!r} vs sklearn {!r}".format(name, k, p, mname, got, float(sk[q, p, i]))
                if mname in ("adjusted_rand", "fowlkes_mallows", "rand"):
                    assert got == sk[q, p, i], where
                elif mname == "adjusted_mutual_info":
                    assert d <= max(100.0 * dev[q, p, i], 1e-13), where
                else:
                    assert d <= 1e-9, where
        for mname in R.NAMES:
            col = out["per_pair"][mname][q]
            assert float(out[mname][q]) == float(sum(col.tolist()) / len(pairs))
    print(name, "largest distance from sklearn:", " ".join("{}={:.2e}".format(k, v) for k, v in worst.items()),
          "| AMI restatement:", "{:.2e}".format(float(dev[..., 2].max())))


@pytest.mark.parametrize("name", ["c64_n2500", "c300_n4000", "c2_n2500", "c7_long"])
def test_bits_do_not_depend_on_run_or_order(env, golden, name):
    m, ids, _ = _scorer(golden, name)
    first = m.score_subset(ids, per_pair=True, return_stats=True)
    _same_bits(first, m.score_subset(ids, per_pair=True, return_stats=True))
    rs = np.random.RandomState(5)
    _same_bits(first, m.score_subset(rs.permutation(ids), per_pair=True, return_stats=True))
    _same_bits(first, m.score_subset(np.sort(ids)[::-1], per_pair=True, return_stats=True))
    assert np.isfinite(first["stats"]["emi"]).all()


@pytest.mark.parametrize("name", ["c7_curve", "c300_n4000"])
def test_curve_points_equal_separate_calls(env, golden, name):
    m, ids, _ = _scorer(golden, name)
    prefix = [1, 10, 256, 257, len(ids)]
    curve = m.score_subset(ids, prefixes=prefix, per_pair=True, return_stats=True)
    assert curve["mutual_info"].shape == (5,) and curve["stats"].shape[0] == 5
    for q, k in enumerate(prefix):
        one = m.score_subset(ids[:k], per_pair=True, return_stats=True)  # the last one: a call without prefixes
        assert one["stats"].tobytes() == curve["stats"][q].tobytes(), k
        for mname in R.NAMES:
            assert float(one[mname]) == float(curve[mname][q]) or (np.isnan(one[mname]) and np.isnan(curve[mname][q]))
            assert one["per_pair"][mname].tobytes() == curve["per_pair"][mname][q].tobytes()
    short = m.score_subset(ids, prefixes=[10, 256], measures=["rand"])  # prefixes that stop short of the list
    assert short["rand"].tolist() == curve["rand"][1:3].tolist() and set(short) == {"rand"}


def test_mask_skips_the_emi_and_changes_nothing_else(env, golden):
    m, ids, _ = _scorer(golden, "c64_n2500")
    full = m.score_subset(ids, per_pair=True, return_stats=True)
    names = [n for n in R.NAMES if n != "adjusted_mutual_info"]
    part = m.score_subset(ids, measures=names, per_pair=True, return_stats=True)
    assert set(part) == set(names) | {"per_pair", "stats"}
    assert np.isnan(part["stats"]["emi"]).all() and np.isfinite(full["stats"]["emi"]).all()
    for f in full["stats"].dtype.names:
        if f != "emi":
            assert part["stats"][f].tobytes() == full["stats"][f].tobytes(), f
    for n in names:
        assert part[n] == full[n] and part["per_pair"][n].tobytes() == full["per_pair"][n].tobytes()
    one = m.score_subset(ids, measures="adjusted_mutual_info")
    assert one == {"adjusted_mutual_info": full["adjusted_mutual_info"]}


def test_greedy_runs_do_not_see_a_scoring_call(env, golden):
    """the same S and GAIN with a score_subset call made first on the same handle; acav_mi_get_counts unchanged across one"""
    assign, C, pairs, ids, _ = _case(golden, "c7_n777")
    cand = list(range(1, 600))

    def batch(score_first):
        env.manual_seed(3)
        m = _measure("batch_mi", assign, C, pairs, cand, batch_size=20, selection_size=4, keep_unselected=True)
        if score_first:
            m.score_subset(ids)
        return m.run_greedy(60, [0], None)[:2]

    def exact(score_first):
        m = _measure("arand", assign, C, pairs, cand)
        if score_first:
            m.score_subset(ids, prefixes=[5, 300])
        return m.run_greedy(12, [0])[:2]

    for run in (batch, exact):
        (s0, g0), (s1, g1) = run(False), run(True)
        assert list(s0) == list(s1) and len(s0) > 0
        assert np.asarray(g0, np.float64).tobytes() == np.asarray(g1, np.float64).tobytes()
    m = _measure("batch_mi", assign, C, pairs, cand)
    m.add_samples(ids[:100])
    before = m.cache
    m.score_subset(ids)
    after = m.cache
    assert before["n"] == after["n"] == 100
    for k in ("N", "a", "b"):
        assert np.array_equal(before[k], after[k])


def test_bad_arguments_are_refused(env, golden):
    import ctypes as C
    from acav100m_amd import _lib
    m, ids, _ = _scorer(golden, "c7_n50")
    scores = np.empty((4, 6))

    def call(ids_, n, prefix, nprefix, mask):
        ids_ = np.ascontiguousarray(ids_, np.int64)
        pre = None if prefix is None else np.ascontiguousarray(prefix, np.int64)
        return _lib._lib.acav_mi_score_subset(m._h, _lib.ptr(ids_), n, _lib.ptr(pre), nprefix, mask, _lib.ptr(scores), None, None)

    assert call(ids, 50, None, 0, 63) == 0
    assert call(ids, 0, None, 0, 63) == -1           # n < 1
    assert call(ids, 50, None, 0, 0) == -1           # empty mask
    assert call(ids, 50, None, 0, 64) == -1          # a bit beyond the six
    assert call(ids, 50, [10, 10, 50], 3, 63) == -1  # not strictly increasing
    assert call(ids, 50, [0, 50], 2, 63) == -1
    assert call(ids, 50, [10, 40], 2, 63) == -1      # does not end at n
    bad = ids.copy()
    bad[49] = 3000
    assert call(bad, 50, None, 0, 63) == -1          # id == V
    bad[49] = -1
    assert call(bad, 50, None, 0, 63) == -1
    with pytest.raises(ValueError, match="out of range"):
        m.score_subset(bad)
    with pytest.raises(ValueError, match="prefixes"):
        m.score_subset(ids, prefixes=[20, 10])
    with pytest.raises(ValueError, match="non-empty"):
        m.score_subset([])
    del C


# ------------------------------------------------------------------ CLI
@pytest.fixture(scope="module")
def assign_dir(env, tmp_path_factory):
    """two assignment shards written with the product's own helpers, in the layout of the other CLI tests
    (root/clusters/shard-00000i.pkl + root/videos/shard-00000i.json)"""
    from acav100m_amd import shards
    root = str(tmp_path_factory.mktemp("acav_eval_cli"))
    rows, layers = 150, 3
    rs = np.random.RandomState(21)
    comp = rs.randint(0, 6, size=2 * rows)
    for s in range(2):
        name = "shard-%06d" % s
        fns = ["clip_%06d_%04d.mp4" % (s, r) for r in range(rows)]
        table = types.SimpleNamespace(filename=fns, shard_size=[rows] * rows, shard_name=[name] * rows,
                                      tags={("audio", "vggish"): ("VGGishExtractor", "audioset"),
                                            ("video", "slowfast"): ("SlowFastExtractor", "kinetics")})
        labels = {}
        for kind, mk in (("audio", "vggish"), ("video", "slowfast")):
            for layer in range(layers):
                col = np.where(rs.rand(rows) < 0.6, comp[s * rows:(s + 1) * rows], rs.randint(0, 6, size=rows))
                labels[(kind, mk, "layer_%d" % layer)] = col.astype(np.int64)
        shards.dump_pickle(shards.assignment_rows(table, labels, range(rows)),
                           os.path.join(root, "clusters", name + ".pkl"))
        os.makedirs(os.path.join(root, "videos"), exist_ok=True)
        with open(os.path.join(root, "videos", name + ".json"), "w") as f:
            json.dump([{"filename": fn, "id": "vid%09d" % (s * rows + r), "segment": [10, 20]} for r, fn in enumerate(fns)], f)
    return root


def test_cli_run_then_evaluate(env, assign_dir):
    from acav100m_amd import shards
    from acav100m_amd.subset_selection.cli import Cli
    from acav100m_amd.subset_selection.evaluate import score_selection
    root = assign_dir
    glob = os.path.join(root, "clusters", "shard-{000000..000001}.pkl")
    out_csv = os.path.join(root, "sel", "output.csv")
    for _ in range(2):  # output.csv is appended to: the second run repeats every row
        random.seed(0)
        Cli().run(shards_path=glob, meta_path=os.path.join(root, "videos"), out_path=out_csv, measure_name="fm",
                  **{"subset.size": 40})
    rows = [(r[0], r[1]) for r in csv.reader(open(out_csv))]
    distinct = list(dict.fromkeys(rows))
    assert len(rows) == 2 * len(distinct) and len(distinct) > 10
    scores_json = os.path.join(root, "sel", "scores.json")
    rep = Cli().evaluate(shards_path=glob, meta_path=os.path.join(root, "videos"), selection_path=out_csv,
                         **{"evaluate.random_baselines": 2, "evaluate.out_path": scores_json, "computation.random_seed": 11})
    assert json.load(open(scores_json)) == json.loads(json.dumps(rep))
    assert rep["measures"] == list(R.NAMES) and list(rep["partitions"]) == ["-1"]
    part = rep["partitions"]["-1"]
    paths = [os.path.join(root, "clusters", "shard-%06d.pkl" % s) for s in range(2)]
    a, types_, shard_names, filenames = shards.load_assignment_shards(paths)
    index = {k: i for i, k in enumerate(zip(shard_names, filenames))}
    ids = [index[k] for k in distinct]
    assert part["n"] == len(distinct) and part["repeated_rows"] == len(distinct) and part["total"] == len(a) == 300
    assert part["selection"] == score_selection(a, types_, ids)
    assert part["whole"] == score_selection(a, types_, range(len(a)))
    assert len(part["random"]) == 2
    for r in range(2):
        draw = random.Random(11 + r).sample(range(len(a)), len(ids))
        assert part["random"][r] == score_selection(a, types_, draw)
    for name in R.NAMES:
        assert part["random_mean"][name] == float(np.mean([d[name] for d in part["random"]]))
    only = Cli().evaluate(shards_path=glob, meta_path=os.path.join(root, "videos"), selection_path=out_csv,
                          **{"evaluate.measures": "rand,adjusted_rand"})
    assert only["partitions"]["-1"]["selection"] == {k: part["selection"][k] for k in ("adjusted_rand", "rand")}
    assert only["partitions"]["-1"]["random"] == []
    with open(out_csv, "a") as f:
        f.write("shard-000001,no_such_clip.mp4,vid,x\n")
    with pytest.raises(ValueError, match="no_such_clip.mp4"):
        Cli().evaluate(shards_path=glob, meta_path=os.path.join(root, "videos"), selection_path=out_csv)
