"""GPU: the pair-counting measures fm / rand / arand and the ami / nmi average methods on the exact-greedy kernel, against the
numpy restatement (tests/_pair_measures.py, bit for bit), the reference's goldens (tests/golden/gen_golden_pair.py) and
sklearn's pair-counting scores."""
import csv
import ctypes as C
import itertools
import json
import os
import random
import types

import numpy as np
import pytest

from tests import _pair_measures as PM

pytestmark = pytest.mark.gpu

CASES = ["a", "b", "c", "d", "e"]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


def _remaining_to_original(idx, L):
    alive = list(range(L))
    return np.array([alive.pop(int(i)) for i in idx], np.int64)


def _measure(name, a, c, pairs, cand, **kw):
    from acav100m_amd.subset_selection import get_measure
    m = get_measure(name)(a, ncentroids=c, device="cuda:0", **kw)
    m.init(pairs, [int(i) for i in cand])
    return m


def _correlated(seed, v, dd, c):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    return np.stack(cols, 1).astype(np.int64)


@pytest.mark.parametrize("measure", ["fm", "rand", "arand"])
@pytest.mark.parametrize("case", CASES)
def test_golden_teacher_forced(env, golden_dir, case, measure):
    """replaying the reference's picks: S identical; every score vector and GAIN equal the restatement bit for bit (NaN in
    the same places), and the reference's fp32 values within 1e-5"""
    g = np.load(os.path.join(golden_dir, f"pair_{case}_{measure}.npz"))
    a, c, start, subset = g["assignments"].astype(np.int64), int(g["C"]), int(g["start"]), int(g["subset"])
    pairs = [tuple(p) for p in g["pairs"].tolist()]
    cand = [i for i in range(a.shape[0]) if i != start]
    m = _measure(measure, a, c, pairs, cand)
    S, GAIN, _, _ = m.run_greedy(subset, [start], record_trace=True, forced_pos=_remaining_to_original(g["idx"], len(cand)))
    assert S == g["S"].tolist()
    ref = PM.golden_pair_run(g, measure, forced=True)
    GAIN = np.array(GAIN)
    assert np.array_equal(GAIN, ref["GAIN"], equal_nan=True)
    alive = list(range(len(cand)))
    for t, k in enumerate(g["idx"]):
        row = m.trace["scores"][t][alive]
        assert np.array_equal(row, ref["scores"][t], equal_nan=True), f"iteration {t}"
        assert m.trace["argmax"][t] == alive[ref["argmax"][t]]
        alive.pop(int(k))
    gold = g["GAIN"]
    assert np.array_equal(np.isnan(GAIN), np.isnan(gold))
    ok = ~np.isnan(gold)
    np.testing.assert_allclose(GAIN[ok], gold[ok], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("measure", ["fm", "rand", "arand"])
@pytest.mark.parametrize("case", CASES)
def test_golden_free_running(env, golden_dir, case, measure):
    g = np.load(os.path.join(golden_dir, f"pair_{case}_{measure}.npz"))
    a, c, start, subset = g["assignments"].astype(np.int64), int(g["C"]), int(g["start"]), int(g["subset"])
    pairs = [tuple(p) for p in g["pairs"].tolist()]
    cand = [i for i in range(a.shape[0]) if i != start]
    S, GAIN, _, _ = _measure(measure, a, c, pairs, cand).run_greedy(subset, [start])
    ref = PM.golden_pair_run(g, measure, forced=False)
    assert S == [start] + ref["S"]
    assert np.array_equal(np.array(GAIN), ref["GAIN"], equal_nan=True)


@pytest.mark.parametrize("measure", ["fm", "rand", "arand"])
def test_free_running_large(env, measure):
    """V = 20 000, C = 256, D = 3, 300 picks: GPU == restatement pick for pick, gains bit for bit"""
    v, dd, c, subset = 20000, 3, 256, 302
    a = _correlated(41, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    order = [int(i) for i in np.random.RandomState(5).permutation(v)]
    S, GAIN, _, _ = _measure(measure, a, c, pairs, order[1:]).run_greedy(subset, order[:1])
    r = PM.PairGreedy(a, pairs, c)
    r.add_samples(order[:1])
    ref = r.run(order[1:], subset, 1, measure)
    assert len(S) == subset - 1 and S == order[:1] + ref["S"]
    assert np.array_equal(np.array(GAIN), ref["GAIN"], equal_nan=True)


def test_sklearn_known_answers_and_pair_stats(env):
    """after each pick, where no residue and no degenerate pair is left, GAIN[t] is the pair mean of sklearn's
    fowlkes_mallows_score / rand_score / adjusted_rand_score of the labels selected so far (1e-12); acav_mi_get_pair_stats
    is pair_confusion_matrix / 2 and sums to n (n - 1) / 2 exactly.  Residue-free: FM needs TP >= 1 in every pair (then a
    residue-only FP or FN adds nothing), Rand TP + TN >= 1; ARI is residue-free and only its NaN (degenerate) picks are left
    out"""
    from sklearn.metrics import adjusted_rand_score, fowlkes_mallows_score, rand_score
    from sklearn.metrics.cluster import pair_confusion_matrix
    fns = dict(fm=fowlkes_mallows_score, rand=rand_score, arand=adjusted_rand_score)
    v, dd, c, subset = 600, 3, 5, 80
    a = _correlated(12, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    checked = 0
    for measure, fn in fns.items():
        m = _measure(measure, a, c, pairs, range(1, v))
        S, GAIN, _, _ = m.run_greedy(subset, [0])
        for t in range(len(GAIN)):
            sel = S[:t + 2]
            pcms = [pair_confusion_matrix(a[sel, d0], a[sel, d1]) // 2 for d0, d1 in pairs]
            clean = {"fm": all(p[1, 1] >= 1 for p in pcms), "rand": all(p[1, 1] + p[0, 0] >= 1 for p in pcms),
                     "arand": not np.isnan(GAIN[t])}[measure]
            if not clean:
                continue
            want = np.mean([fn(a[sel, d0], a[sel, d1]) for d0, d1 in pairs])
            assert abs(GAIN[t] - want) <= 1e-12, (measure, t, GAIN[t], want)
            checked += 1
        st = m.pair_stats()
        n = len(S)
        assert np.array_equal(st["TP"] + st["FP"] + st["FN"] + st["TN"], np.full(len(pairs), n * (n - 1) // 2))
        for p, (d0, d1) in enumerate(pairs):
            pcm = pair_confusion_matrix(a[S, d0], a[S, d1]) // 2
            assert [[st["TN"][p], st["FP"][p]], [st["FN"][p], st["TP"][p]]] == pcm.tolist()
        if measure != "arand":
            assert set(m.cache) >= {"N", "a", "b", "n", "TP", "FP", "FN", "TN"}
    assert checked > 150


def _avg_replay(g, measure, method, forced_from=None):
    a, c = g["assignments"].astype(np.int64), int(g["C"])
    pairs = [tuple(p) for p in g["pairs"].tolist()]
    cand = g["candidates"].tolist()
    kw = {} if method is None else dict(average_method=method)
    m = _measure(measure, a, c, pairs, cand, **kw)
    m.add_samples(g["seeds"].tolist())
    idx = (forced_from if forced_from is not None else g)["idx"]
    S, GAIN, _, _ = m.run_greedy(int(g["subset"]), g["seeds"].tolist(), record_trace=True,
                                 forced_pos=_remaining_to_original(idx, len(cand)))
    rows, alive = [], list(range(len(cand)))
    for t, k in enumerate(idx):
        rows.append(m.trace["scores"][t][alive].copy())
        alive.pop(int(k))
    return S, np.array(GAIN), rows


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("method", ["max", "min"])
@pytest.mark.parametrize("measure", ["ami", "nmi"])
def test_average_method_goldens(env, golden_dir, measure, method, case):
    g = np.load(os.path.join(golden_dir, f"mi_avg_{measure}_{method}_{case}.npz"))
    S, GAIN, rows = _avg_replay(g, measure, method)
    assert S == g["S"].tolist()
    for t, row in enumerate(rows):
        np.testing.assert_allclose(row, g["scores"][t, :len(row)], rtol=1e-5, atol=1e-7, err_msg=f"iteration {t}")
    np.testing.assert_allclose(GAIN, g["GAIN"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("case", ["a", "b"])
def test_nmi_average_methods_ordered_and_default_unchanged(env, golden_dir, case):
    """on one trace (the max golden's picks), per candidate NMI(max) <= NMI(arithmetic) <= NMI(min); the default and an
    explicit 'arithmetic' are the same doubles"""
    g = np.load(os.path.join(golden_dir, f"mi_avg_nmi_max_{case}.npz"))
    _, _, r_max = _avg_replay(g, "nmi", "max")
    _, _, r_min = _avg_replay(g, "nmi", "min", forced_from=g)
    _, _, r_ar = _avg_replay(g, "nmi", "arithmetic", forced_from=g)
    _, _, r_def = _avg_replay(g, "nmi", None, forced_from=g)
    for t in range(len(r_max)):
        assert np.all(r_max[t] <= r_ar[t]) and np.all(r_ar[t] <= r_min[t]), f"iteration {t}"
        assert np.array_equal(r_ar[t], r_def[t])


def test_errors_are_loud(env):
    from acav100m_amd import _lib
    from acav100m_amd.subset_selection import get_measure
    a = _correlated(3, 50, 2, 4)
    with pytest.raises(ValueError, match="average_method"):
        get_measure("nmi")(a, average_method="geometric", ncentroids=4, device="cuda:0")
    m = _measure("mi", a, 4, [(0, 1)], range(1, 50))
    with pytest.raises(ValueError, match="unknown measure"):
        _lib.check(_lib._lib.acav_mi_set_measure(m._h, 7))
    with pytest.raises(ValueError, match="average_method"):
        _lib.check(_lib._lib.acav_mi_set_average_method(m._h, 3))
    with pytest.raises(ValueError, match="no sample"):
        _measure("fm", a, 4, [(0, 1)], range(50)).run_greedy(10, [])


# ------------------------------------------------------------------ an empty start, through the three entry points
def _empty_start_case(measure, seeds=((),)):
    """V = 64, D = 3, C = 4, all 3 pairs, every id a candidate; one handle per entry of `seeds`, holding those start clips"""
    a = _correlated(7, 64, 3, 4)
    pairs = list(itertools.combinations(range(3), 2))
    ms = [_measure(measure, a, 4, pairs, range(64)) for _ in seeds]
    for m, s in zip(ms, seeds):
        m.add_samples(list(s))
    return ms


def _table_n(m):
    from acav100m_amd import _lib
    n = C.c_int64(-1)
    _lib.check(_lib._lib.acav_mi_get_counts(m._h, None, None, None, C.byref(n)))
    return n.value


def _raw_exact_multi(ms, subset):
    """acav_mi_run_exact_multi on the handles' own candidate lists, ns = 0, outputs pre-filled: rc, S, G, n_selected"""
    from acav100m_amd import _lib
    n = len(ms)
    S = [np.full(subset, -7, np.int64) for _ in ms]
    G = [np.full(subset, -7.0, np.float64) for _ in ms]
    nsel = np.full(n, -7, np.int64)
    parr = lambda xs: (C.c_void_p * n)(*[x.value if isinstance(x, C.c_void_p) else x for x in xs])  # noqa: E731
    cands = [np.ascontiguousarray(m.candidate_ids, np.int64) for m in ms]
    rc = _lib._lib.acav_mi_run_exact_multi(parr([m._h for m in ms]), n, parr([_lib.ptr(c) for c in cands]),
                                           _lib.ptr(np.array([len(c) for c in cands], np.int64)), _lib.ptr(np.zeros(n, np.int32)),
                                           _lib.ptr(np.full(n, subset, np.int64)), parr([_lib.ptr(x) for x in S]),
                                           parr([_lib.ptr(x) for x in G]), _lib.ptr(nsel))
    return rc, S, G, nsel


@pytest.mark.parametrize("measure", ["fm", "rand"])
def test_empty_start_is_refused_by_every_entry_point(env, measure):
    """fm / rand on tables that hold no sample: acav_mi_run_exact, acav_mi_run_celf and acav_mi_run_exact_multi (chunk 0 holds
    one start clip, chunk 1 none) refuse, and the tables keep the n they had; the lockstep call names the chunk and leaves
    its pre-filled outputs alone"""
    from acav100m_amd import _lib
    for kw in ({}, {"celf_ratio": 0.5}):
        m, = _empty_start_case(measure)
        with pytest.raises(ValueError, match="hold no sample"):
            m.run_greedy(4, [], **kw)
        assert _table_n(m) == 0
    ms = _empty_start_case(measure, seeds=((5,), ()))
    rc, S, G, nsel = _raw_exact_multi(ms, 4)
    assert _lib._lib.acav_last_error().decode().startswith("chunk 1: ")
    with pytest.raises(ValueError, match="hold no sample"):
        _lib.check(rc)
    assert [_table_n(m) for m in ms] == [1, 0]
    assert (nsel == -7).all() and all((s == -7).all() for s in S) and all((g == -7.0).all() for g in G)


def test_arand_runs_from_an_empty_start_the_same_everywhere(env):
    """arand needs no start sample: 3 picks for a subset of 4, the same three through the plain call, the CELF call at
    celf_ratio 0.5 and the lockstep call"""
    plain, = _empty_start_case("arand")
    S_plain = plain.run_greedy(4, [])[0]
    lazy, = _empty_start_case("arand")
    S_lazy = lazy.run_greedy(4, [], celf_ratio=0.5)[0]
    ms = _empty_start_case("arand", seeds=((), ()))
    rc, S, _, nsel = _raw_exact_multi(ms, 4)
    assert rc == 0 and nsel.tolist() == [3, 3]
    assert len(S_plain) == 3 and S_plain == S_lazy == S[0][:3].tolist() == S[1][:3].tolist()
    assert [_table_n(m) for m in (plain, lazy, *ms)] == [3, 3, 3, 3]


# ------------------------------------------------------------------ CLI
@pytest.fixture(scope="module")
def assign_dir(env, tmp_path_factory):
    """two assignment shards written with the product's own helpers, in the layout of test_gpu_cli's workdir
    (root/clusters/shard-00000i.pkl + root/videos/shard-00000i.json)"""
    from acav100m_amd import shards
    root = str(tmp_path_factory.mktemp("acav_pair_cli"))
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


def test_cli_run_fm_and_compare_measures(env, assign_dir):
    from acav100m_amd import shards
    from acav100m_amd.subset_selection.cli import Cli
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    root = assign_dir
    glob = os.path.join(root, "clusters", "shard-{000000..000001}.pkl")
    out_csv = os.path.join(root, "fm", "output.csv")
    random.seed(0)
    Cli().run(shards_path=glob, meta_path=os.path.join(root, "videos"), out_path=out_csv, measure_name="fm",
              **{"subset.size": 40})
    got = [r[1] for r in csv.reader(open(out_csv))]
    paths = [os.path.join(root, "clusters", "shard-%06d.pkl" % s) for s in range(2)]
    a, ctypes_, _, filenames = shards.load_assignment_shards(paths)
    random.seed(0)
    order = list(range(len(a)))
    random.shuffle(order)
    pairs = get_cluster_pairing(ctypes_, "combination")
    r = PM.PairGreedy(a, [p[:2] for p in pairs], int(a.max()) + 1)
    r.add_samples(order[:1])
    ref = r.run(order[1:], 40, 1, "fm")
    assert len(got) == 39  # the start clip + subset - 2 picks: range(len(start), subset_size - 1), efficient.py:240-302
    assert got == [filenames[s] for s in sorted(order[:1] + ref["S"])]
    rep = Cli().compare_measures(shards_path=glob, meta_path=os.path.join(root, "videos"),
                                 out_path=os.path.join(root, "cmp", "output.csv"), measure_names=["mi", "fm", "rand", "arand"],
                                 **{"subset.size": 30})
    assert len(rep) == 6
    assert [row[1:3] for row in rep] == [(x, y) for x, y in itertools.combinations(["mi", "fm", "rand", "arand"], 2)]
