"""GPU: layer-weighted clustering pairs (`weight_type`, acav_mi_set_pair_weights) on the exact greedy (`mi`, `mem_mi`) and
the batch greedy (`batch_mi`: single chunk, lockstep chunks, the tiled and the legacy permutation paths), against the
reference's weighted runs (tests/golden/gen_golden_weights.py) and the numpy float64 restatement (tests/_weights_ref.py,
bit for bit)."""
import csv
import io as _io
import itertools
import os
import pickle
import random
import warnings

import numpy as np
import pytest

from tests import _weights_ref as WR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


def _keys(dd):
    return [(m, "layer_{}".format(i)) for m in ("SlowFast", "VGGish") for i in range(dd // 2)]


def _correlated(seed, v, dd, c):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    a = np.stack(cols, 1).astype(np.int64)
    a[0] = c - 1
    return a


def _remaining_to_original(idx, L):
    alive = list(range(L))
    return np.array([alive.pop(int(i)) for i in idx], np.int64)


def _measure(name, a, c, comb, cand, **kw):
    from acav100m_amd.subset_selection import get_measure
    m = get_measure(name)(a, ncentroids=c, device="cuda:0", **kw)
    m.init(comb, [int(i) for i in cand])
    return m


def _batch(a, c, comb, cand, B=20, k=4):
    return _measure("batch_mi", a, c, comb, cand, batch_size=B, selection_size=k, keep_unselected=True)


# ----------------------------------------------------------------------------- 1. teacher-forced on the reference
@pytest.mark.parametrize("name", ["a", "b", "c"])
@pytest.mark.parametrize("measure", ["mi", "mem_mi"])
def test_exact_golden_teacher_forced(env, golden_dir, name, measure):
    g = np.load(os.path.join(golden_dir, "weights_exact_{}_{}.npz".format(name, measure)))
    a, c, start, subset = g["assignments"].astype(np.int64), int(g["C"]), int(g["start"]), int(g["subset"])
    comb = {"pairing": [tuple(p) for p in g["pairs"]], "weights": list(g["weights"])}
    # correspondence_retrieval's run adds the start clip to the tables first; EfficientMI also drops it from the candidates,
    # EfficientMemMI's add_samples (mem_mi.py:142-150) leaves it there
    cand = list(range(len(a))) if measure == "mem_mi" else [i for i in range(len(a)) if i != start]
    L = len(cand)
    m = _measure(measure, a, c, comb, cand)
    m.add_samples([start])
    idx = g["idx"]
    S, GAIN, _, _ = m.run_greedy(subset, [start], None, record_trace=True, forced_pos=_remaining_to_original(idx, L))
    assert S == g["S"].tolist()
    np.testing.assert_allclose(GAIN, g["GAIN"], rtol=1e-5, atol=1e-6)
    alive, diff = list(range(L)), 0
    for t in range(len(idx)):
        row, ref = m.trace["scores"][t][alive], g["scores"][t, :len(alive)].astype(np.float64)
        np.testing.assert_allclose(row, ref, rtol=1e-5, atol=1e-6)
        ours = alive.index(int(m.trace["argmax"][t]))
        if ours != int(idx[t]):  # a near-tie of the reference's fp32 scores
            assert abs(ref[ours] - ref[int(idx[t])]) <= 2e-6 * max(abs(ref[int(idx[t])]), 1e-3), (t, ref[ours], ref[idx[t]])
            diff += 1
        alive.pop(int(idx[t]))
    print("weights_exact_{}_{}: {}/{} picks differ from the reference's, all at near-ties".format(name, measure, diff, len(idx)))


@pytest.mark.parametrize("name", ["a", "b"])
def test_batch_golden_teacher_forced(env, golden_dir, name):
    g = np.load(os.path.join(golden_dir, "weights_batch_{}.npz".format(name)))
    a, c, start, subset = g["assignments"].astype(np.int64), int(g["C"]), int(g["start"]), int(g["subset"])
    B, k = int(g["B"]), int(g["k"])
    comb = {"pairing": [tuple(p) for p in g["pairs"]], "weights": list(g["weights"])}
    cand = [i for i in range(len(a)) if i != start]
    env.manual_seed(int(g["seed"]))
    m = _batch(a, c, comb, cand, B, k)
    pos = g["pos"]
    S, GAIN, _, _ = m.run_greedy(subset, [start], None, record_trace=True, forced_pos=pos)
    n = min(len(m.trace["ids"]), len(g["ids"]))
    assert n >= len(g["ids"]) - 1 and n > 10
    assert np.array_equal(m.trace["ids"][:n], g["ids"][:n])  # the same permutation stream and re-queue order
    picks_ref = [s for s in g["S"].tolist() if s != start]
    assert S[:len(picks_ref)] == picks_ref[:len(S)]
    ref_sc = g["scores"][:n].astype(np.float64)
    np.testing.assert_allclose(m.trace["scores"][:n], ref_sc, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(GAIN[:n * k], g["GAIN"][:n * k], rtol=1e-5, atol=1e-6)
    diff = 0
    for t in range(n):
        if set(m.trace["pos"][t]) != set(pos[t]):
            srt = np.sort(ref_sc[t])[::-1]
            assert abs(srt[k - 1] - srt[k]) <= 2e-6 * max(abs(srt[k - 1]), 1e-3), (t, srt[:k + 1])
            diff += 1
    print("weights_batch_{}: {}/{} iterations pick differently from the reference, all at near-ties".format(name, diff, n))


# ----------------------------------------------------------------------------- 2. free-running == the restatement
def _weighted_case(dd, pairing, weight_type, v, c, seed):
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    a = _correlated(seed, v, dd, c)
    comb = get_cluster_pairing(_keys(dd), pairing, weight_type)
    rs = np.random.RandomState(seed + 1)
    order = [int(i) for i in rs.permutation(v)]
    return a, comb, order[:1], order[1:]


@pytest.mark.parametrize("dd,weight_type,v,c,subset", [(10, "linear_1", 600, 32, 300), (24, "exp_0.5", 400, 8, 60)])
def test_exact_free_running_equals_restatement(env, dd, weight_type, v, c, subset):
    a, comb, start, cand = _weighted_case(dd, "combination", weight_type, v, c, dd)
    assert len(comb["pairing"]) == dd * (dd - 1) // 2
    m = _measure("mi", a, c, comb, cand)
    S, GAIN, _, _ = m.run_greedy(subset, start, None)
    ref = WR.WeightedMI(a, comb["pairing"], c, comb["weights"])
    S_ref, G_ref = ref.run_exact(cand, subset - 2)
    assert S[1:] == S_ref and np.array_equal(np.array(GAIN), np.array(G_ref))


@pytest.mark.parametrize("dd,weight_type,v,c,subset,legacy", [
    (10, "linear_1", 3000, 32, 1200, False),   # P = 45, 300 iterations
    (10, "log_-1", 3000, 32, 400, True),       # the same on the global-atomic permutation kernels
    (24, "exp_0.5", 4000, 8, 200, False),      # P = 276 > SEL_LDSP: weights beyond the staged pairs read from memory
])
def test_batch_free_running_equals_restatement(env, monkeypatch, dd, weight_type, v, c, subset, legacy):
    if legacy:
        monkeypatch.setenv("ACAV_FY_LEGACY", "1")
    a, comb, start, cand = _weighted_case(dd, "combination", weight_type, v, c, dd + v)
    env.manual_seed(5)
    m = _batch(a, c, comb, cand)
    S, GAIN, _, _ = m.run_greedy(subset, start, None, record_trace=True)
    ref = WR.WeightedMI(a, comb["pairing"], c, comb["weights"])
    S_ref, G_ref, sc_ref, pos_ref = ref.run_batch_traced(start, m.trace["ids"], m.k)
    assert np.array_equal(m.trace["scores"], sc_ref)
    assert np.array_equal(m.trace["pos"], pos_ref)
    assert S == S_ref[:len(S)] and np.array_equal(np.array(GAIN), np.array(G_ref))


def test_batch_tiled_first_iterations_at_one_million(env):
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    v, dd, c = 1_000_000, 4, 64
    a = _correlated(77, v, dd, c)
    comb = get_cluster_pairing(_keys(dd), "combination", "exp_1")
    rs = np.random.RandomState(78)
    order = rs.permutation(v).astype(np.int64)
    env.manual_seed(11)
    m = _batch(a, c, comb, order[1:])
    S, GAIN, _, _ = m.run_greedy(200_000, [int(order[0])], None, record_trace=True, max_iters=40)
    assert len(m.trace["ids"]) == 40
    ref = WR.WeightedMI(a, comb["pairing"], c, comb["weights"])
    S_ref, G_ref, sc_ref, _ = ref.run_batch_traced([int(order[0])], m.trace["ids"], m.k)
    assert np.array_equal(m.trace["scores"], sc_ref)
    assert S == S_ref[:len(S)] and np.array_equal(np.array(GAIN), np.array(G_ref[:len(GAIN)]))


# ----------------------------------------------------------------------------- 3. all-ones weights == unweighted
def test_all_ones_weights_are_bit_identical_to_unweighted(env):
    from acav100m_amd.subset_selection.measures import EfficientBatchMI
    from acav100m_amd.rng import Generator
    dd, v, c = 10, 2000, 16
    a, comb, start, cand = _weighted_case(dd, "combination", "linear_0", v, c, 3)
    assert all(w == 1.0 for w in comb["weights"])
    plain = comb["pairing"]
    for meas in ("mi", "mem_mi"):
        r = [_measure(meas, a, c, x, cand).run_greedy(120, start, None)[:2] for x in (plain, comb)]
        assert r[0][0] == r[1][0] and np.array_equal(np.array(r[0][1]), np.array(r[1][1]))
    out = []
    for x in (plain, comb):
        env.manual_seed(2)
        out.append(_batch(a, c, x, cand).run_greedy(400, start, None)[:2])
    assert out[0][0] == out[1][0] and np.array_equal(np.array(out[0][1]), np.array(out[1][1]))
    lock = []
    for x in (plain, comb):
        ms = []
        for i in range(3):
            m = _measure("batch_mi", a, c, x, cand, batch_size=20, selection_size=4, keep_unselected=True,
                         generator=Generator(40 + i))
            ms.append(m)
        lock.append(EfficientBatchMI.run_greedy_multi(ms, [200, 240, 160], [start] * 3))
    for r0, r1 in zip(*lock):
        assert r0[0] == r1[0] and np.array_equal(np.array(r0[1]), np.array(r1[1]))


# ----------------------------------------------------------------------------- 4. lockstep == individual runs
def test_lockstep_weighted_chunks_equal_individual_runs(env):
    from acav100m_amd.subset_selection.measures import EfficientBatchMI
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    from acav100m_amd.rng import Generator
    dd, c = 10, 16
    specs = [(1500, "linear_2", 300), (1800, None, 360), (1200, "onehot_1", 240), (1600, "exp_-1", 320)]
    cases = []
    for i, (v, wt, sub) in enumerate(specs):
        a = _correlated(100 + i, v, dd, c)
        comb = get_cluster_pairing(_keys(dd), "combination", wt)
        order = [int(x) for x in np.random.RandomState(200 + i).permutation(v)]
        cases.append((a, comb, order[:1], order[1:], sub))

    def make(i):
        a, comb, start, cand, sub = cases[i]
        return _measure("batch_mi", a, c, comb, cand, batch_size=20, selection_size=4, keep_unselected=True,
                        generator=Generator(70 + i))
    multi = EfficientBatchMI.run_greedy_multi([make(i) for i in range(len(cases))], [x[4] for x in cases],
                                              [x[2] for x in cases])
    for i, (a, comb, start, cand, sub) in enumerate(cases):
        S, G, _, _ = make(i).run_greedy(sub, start, None)
        assert multi[i][0] == S and np.array_equal(np.array(multi[i][1]), np.array(G)), i


def test_legacy_weighted_chunks_equal_individual_runs(env, monkeypatch):
    """The same with ACAV_FY_LEGACY=1, where the chunks of one call run one after another: weighted and unweighted
    handles mixed in one call."""
    monkeypatch.setenv("ACAV_FY_LEGACY", "1")
    test_lockstep_weighted_chunks_equal_individual_runs(env)


# ----------------------------------------------------------------------------- 5. onehot_4 == penultimate
def test_onehot_penultimate_selects_what_a_penultimate_run_selects(env):
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    dd, v, c, subset = 10, 800, 12, 200
    a = _correlated(9, v, dd, c)
    keys = _keys(dd)
    order = [int(x) for x in np.random.RandomState(10).permutation(v)]
    start, cand = order[:1], order[1:]
    pen = _measure("mi", a, c, get_cluster_pairing(keys, "penultimate"), cand)
    S_pen, _, _, _ = pen.run_greedy(subset, start, None, record_trace=True)
    comb = get_cluster_pairing(keys, "combination", "onehot_4")
    assert sum(w != 0 for w in comb["weights"]) == 1 and comb["pairing"][int(np.argmax(comb["weights"]))] == (4, 9)
    one = _measure("mi", a, c, comb, cand)
    pos = {x: i for i, x in enumerate(cand)}
    forced = np.array([pos[s] for s in S_pen[1:]], np.int64)  # replay the penultimate run's picks
    S_one, _, _, _ = one.run_greedy(subset, start, None, record_trace=True, forced_pos=forced)
    assert S_one == S_pen
    ties = 0
    for t in range(len(forced)):
        got, want = int(one.trace["argmax"][t]), int(forced[t])
        if got != want:
            s1, sp = one.trace["scores"][t], pen.trace["scores"][t]
            assert s1[got] == s1[want] and sp[want] > sp[got], (t, s1[got], s1[want], sp[want], sp[got])
            ties += 1
    print("onehot_4 vs penultimate: {}/{} picks differ, each where / 45 rounds two scores together".format(ties, len(forced)))


# ----------------------------------------------------------------------------- 6. CLI end to end
def _write_shards(root, a, keys, rows_per_shard):
    os.makedirs(os.path.join(root, "clusters"), exist_ok=True)
    names, files = [], []
    for s in range(len(a) // rows_per_shard):
        rows = []
        for r in range(rows_per_shard):
            i = s * rows_per_shard + r
            row = {"shard_name": "shard-%06d" % s, "filename": "clip_%06d.mp4" % i}
            for view, model in (("video_assignments", "SlowFast"), ("audio_assignments", "VGGish")):
                row[view] = [{"model_key": model, "array": {l: int(a[i, d]) for d, (m, l) in enumerate(keys) if m == model}}]
            rows.append(row)
            names.append(row["shard_name"])
            files.append(row["filename"])
        with open(os.path.join(root, "clusters", "shard-%06d.pkl" % s), "wb") as f:
            pickle.dump(rows, f)
    return os.path.join(root, "clusters", "shard-{000000..%06d}.pkl" % (len(a) // rows_per_shard - 1)), files


def test_cli_weight_type_end_to_end(env, tmp_path):
    from oracle import oracle as O
    from acav100m_amd.subset_selection.cli import Cli
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    dd, c, per = 10, 12, 150
    keys = _keys(dd)
    a = _correlated(31, 4 * per, dd, c)
    glob, files = _write_shards(str(tmp_path), a, keys, per)
    comb = get_cluster_pairing(keys, "combination", "linear_1")

    def expect(rows, seed_py, rng_seed):
        random.seed(seed_py)
        cand = list(range(len(rows)))
        random.shuffle(cand)
        ref = WR.WeightedMI(a[rows], comb["pairing"], int(a[rows].max()) + 1, comb["weights"])
        S, _ = ref.run_batch(cand[1:], cand[:1], round(0.2 * len(rows)), 20, 4, O.Rng(rng_seed))
        return sorted(files[rows[s]] for s in S)

    def read(path):
        return [r[1] for r in csv.reader(_io.StringIO(open(path).read()))]

    # one chunk
    out = os.path.join(str(tmp_path), "single", "output.csv")
    random.seed(0)
    env.manual_seed(0)
    Cli().run(shards_path=glob, out_path=out, **{"clustering.weight_type": "linear_1"})
    assert read(out) == expect(np.arange(4 * per), 0, 0)
    # two chunks in lockstep (chunk `num` draws from Generator(random_seed + 1 + num))
    out = os.path.join(str(tmp_path), "lockstep", "output.csv")
    random.seed(1)
    Cli().run(shards_path=glob, out_path=out, chunk_size=2,
              **{"clustering.weight_type": "linear_1", "computation.concurrent_chunks": 2, "computation.random_seed": 7})
    Cli().reduce_csvs(out_path=out)
    random.seed(1)
    want = []
    for num in range(2):
        rows = np.arange(2 * num * per, (2 * num + 2) * per)
        cand = list(range(len(rows)))
        random.shuffle(cand)
        ref = WR.WeightedMI(a[rows], comb["pairing"], int(a[rows].max()) + 1, comb["weights"])
        S, _ = ref.run_batch(cand[1:], cand[:1], round(0.2 * len(rows)), 20, 4, O.Rng(7 + 1 + num))
        want += sorted(files[rows[s]] for s in S)
    assert read(out) == want


def test_measures_that_ignore_weights_warn_and_run_unweighted(env):
    dd, v, c = 4, 300, 6
    a, comb, start, cand = _weighted_case(dd, "combination", "linear_2", v, c, 1)
    for name in ("ami", "nmi", "fm"):
        with pytest.warns(UserWarning, match="ignored"):
            m = _measure(name, a, c, comb, cand)
        S, G, _, _ = m.run_greedy(30, start, None)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            p = _measure(name, a, c, comb["pairing"], cand)
        S2, G2, _, _ = p.run_greedy(30, start, None)
        assert S == S2 and np.array_equal(np.array(G), np.array(G2), equal_nan=True)
