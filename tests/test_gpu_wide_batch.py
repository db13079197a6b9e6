"""GPU tests of the WIDE batch greedy: batch_mi with 64 < batch_size <= 1024 (selection_size up to batch_size, batch_size x pairs
<= 8192).  Yardsticks: the reference's own traces at the paper grid's batch setting (tests/golden/mi_wide_*.npz, teacher-forced),
the oracle bit for bit wherever it can go (selection_size <= 64), the numpy restatement tests/_weights_ref.py beyond (tied to
both by tests/test_wide_batch_ref.py), every route through the library against each other, and the narrow path at its boundary."""
import itertools
import os
import random
import sys
import warnings

import numpy as np
import pytest

from tests._weights_ref import WeightedMI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    from oracle import oracle as O
    return torch, acav100m_amd, O


def _measure(a, c, pairs, cand, B, k, keep=True, generator=None, weights=None):
    from acav100m_amd.subset_selection import get_measure
    kw = {} if generator is None else dict(generator=generator)
    m = get_measure("batch_mi")(a, ncentroids=c, batch_size=B, selection_size=k, device="cuda:0", keep_unselected=keep, **kw)
    m.init(pairs if weights is None else dict(pairing=pairs, weights=weights), cand)
    return m


def _correlated(seed, v, dd, c):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    a = np.stack(cols, 1).astype(np.int64)
    a[0] = c - 1
    return a


def _inputs(v, dd, c):
    a = _correlated(v + dd, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    cand = [int(i) for i in np.random.RandomState(v).permutation(v)]
    return a, pairs, cand[:1], cand[1:]


# ------------------------------------------------------------------ 1. the reference's traces, teacher-forced
@pytest.mark.parametrize("name", ["a", "b"])
def test_golden_trace_teacher_forced(env, golden_dir, name):
    torch, acav, O = env
    g = np.load(os.path.join(golden_dir, f"mi_wide_{name}.npz"))
    a, c, seed = g["assignments"], int(g["C"]), int(g["seed"])
    B, k = int(g["B"]), int(g["k"])
    v, dd = a.shape
    pairs = list(itertools.combinations(range(dd), 2))
    subset = round(float(g["ratio"]) * v)
    cand = list(g["shuffled"])
    start, cand = [cand[0]], cand[1:]
    acav.manual_seed(seed)
    m = _measure(a, c, pairs, cand, B, k)
    S, GAIN, _, _ = m.run_greedy(subset, start, None, record_trace=True, forced_pos=g["pick_pos"])
    # permutation stream, batch slicing and re-queue order are exactly the reference's
    assert m.trace["ids"].shape == g["ids"].shape
    assert np.array_equal(m.trace["ids"], g["ids"])
    assert S == list(g["S"])
    ref_mean = g["scores"].astype(np.float64).mean(-1)
    np.testing.assert_allclose(m.trace["scores"], ref_mean, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(GAIN, g["GAIN"], rtol=1e-5, atol=1e-6)
    # our own picks differ from the reference's only at fp32 near-ties of the reference scores
    diff = 0
    for t in range(len(g["ids"])):
        if set(m.trace["pos"][t]) != set(g["pick_pos"][t]):
            srt = np.sort(ref_mean[t])[::-1]
            assert abs(srt[k - 1] - srt[k]) <= 2e-6 * max(abs(srt[k - 1]), 1e-3), (t, srt[:k + 1])
            diff += 1
    print(f"mi_wide_{name}: {diff}/{len(g['ids'])} iterations differ from the reference picks, all at near-ties")


# ------------------------------------------------------------------ 2. free-running == the oracle, bit for bit
def _check_equals_oracle(env, v, dd, c, B, k, keep, subset):
    torch, acav, O = env
    a, pairs, start, cand = _inputs(v, dd, c)
    acav.manual_seed(9)
    m = _measure(a, c, pairs, cand, B, k, keep=keep)
    S, GAIN, _, _ = m.run_greedy(subset, start, None, record_trace=True)
    rng = O.Rng(9)
    om = O.BatchMI(a, c, pairs)
    assert m.k <= 64  # the oracle holds at most 64 picks per iteration
    ref = om.run_greedy(cand, start, subset, B, m.k, rng, keep_unselected=keep, trace=True)
    assert np.array_equal(m.trace["ids"], ref["ids"])
    assert np.array_equal(m.trace["pos"], ref["pos"])
    assert S == list(ref["S"])
    assert np.array_equal(np.array(GAIN), ref["GAIN"])  # same float64 operations, same order
    assert len(set(S)) == len(S) == subset and start[0] not in S
    Nc, ac, bc, nc = om.counts()
    cache = m.cache
    assert np.array_equal(cache["N"], Nc) and np.array_equal(cache["a"], ac) and np.array_equal(cache["b"], bc)
    assert cache["n"] == nc == 1 + len(GAIN)
    mt_o, idx_o = rng.get_state()
    mt_p, idx_p = acav.default_generator.get_state()
    assert idx_o == idx_p and np.array_equal(mt_o, mt_p)
    return m


@pytest.mark.parametrize("B,k,dd,c,keep,v,subset", [
    (65, 1, 2, 16, True, 700, 40),       # the first batch size beyond one wave
    (65, 64, 2, 16, True, 900, 256),     # selection_size 64: the oracle's limit; one id re-queued
    (100, 25, 2, 64, True, 1500, 300),   # fast commit, the scoring's phi kept
    (100, 25, 3, 16, True, 1500, 300),   # fast commit, phi re-read
    (129, 32, 2, 32, False, 2100, 592),  # wave boundary; nothing re-queued; modify_k raises selection_size to 37
    (160, 40, 10, 32, True, 1200, 200),  # plain commit: batch_size x pairs = 7200
    (257, 64, 2, 16, True, 2000, 320),   # more positions than the workgroup has threads
    (1024, 64, 2, 8, True, 5000, 640),   # the cap
])
def test_free_running_equals_oracle(env, B, k, dd, c, keep, v, subset):
    m = _check_equals_oracle(env, v, dd, c, B, k, keep, subset)
    assert m.k == (37 if not keep else k)


# ------------------------------------------------------------------ 3. selection_size > 64 == the numpy restatement
@pytest.mark.parametrize("B,k,dd,c,v,subset", [(160, 80, 2, 16, 2000, 400), (200, 100, 4, 16, 2000, 400),
                                               (128, 128, 2, 16, 1500, 512), (1024, 512, 2, 8, 5000, 2048)])
def test_large_selection_equals_restatement(env, B, k, dd, c, v, subset):
    torch, acav, O = env
    a, pairs, start, cand = _inputs(v, dd, c)
    acav.manual_seed(11)
    m = _measure(a, c, pairs, cand, B, k)
    S, GAIN, _, _ = m.run_greedy(subset, start, None)
    rng = O.Rng(11)
    Sr, Gr = WeightedMI(a, pairs, c).run_batch(cand, start, subset, B, k, rng)
    assert S == Sr and len(set(S)) == subset
    assert np.array_equal(np.array(GAIN), np.array(Gr))  # float64, bit for bit
    mt_o, idx_o = rng.get_state()
    mt_p, idx_p = acav.default_generator.get_state()
    assert idx_o == idx_p and np.array_equal(mt_o, mt_p)


# ------------------------------------------------------------------ 4. the same results by every route
@pytest.fixture(scope="module")
def route_case(env):
    """(100, 25) on three clusterings: inputs and the oracle's result, computed once"""
    torch, acav, O = env
    v, dd, c, subset = 1500, 3, 16, 300
    a, pairs, start, cand = _inputs(v, dd, c)
    ref = O.BatchMI(a, c, pairs).run_greedy(cand, start, subset, 100, 25, O.Rng(21), keep_unselected=True, trace=True)
    return a, c, pairs, start, cand, subset, ref


@pytest.mark.parametrize("switch", [("ACAV_FY_LEGACY", "1"), ("ACAV_FY_ECAP", "64")])
def test_permutation_variants_equal_oracle(env, route_case, switch, monkeypatch):
    torch, acav, O = env
    a, c, pairs, start, cand, subset, ref = route_case
    monkeypatch.setenv(*switch)
    acav.manual_seed(21)
    m = _measure(a, c, pairs, cand, 100, 25)
    S, GAIN, _, _ = m.run_greedy(subset, start, None, record_trace=True)
    assert np.array_equal(m.trace["ids"], ref["ids"]) and np.array_equal(m.trace["pos"], ref["pos"])
    assert S == list(ref["S"]) and np.array_equal(np.array(GAIN), ref["GAIN"])


def test_unit_weights_equal_unweighted(env, route_case):
    torch, acav, O = env
    a, c, pairs, start, cand, subset, ref = route_case
    acav.manual_seed(21)
    m = _measure(a, c, pairs, cand, 100, 25, weights=[1.0] * len(pairs))
    S, GAIN, _, _ = m.run_greedy(subset, start, None)
    assert S == list(ref["S"]) and np.array_equal(np.array(GAIN), ref["GAIN"])


def test_lockstep_chunks_equal_individual_runs(env, route_case):
    torch, acav, O = env
    from acav100m_amd.rng import Generator
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    a, c, pairs, start, cand, subset, ref = route_case
    a2, pairs2, start2, cand2 = _inputs(1100, 2, 40)
    data = [(a, c, pairs, start, cand, subset), (a2, 40, pairs2, start2, cand2, 170)]
    for legacy in (False, True):
        if legacy:
            os.environ["ACAV_FY_LEGACY"] = "1"
        try:
            alone, tails = [], []
            for i, (aa, cc, pp, st, cd, sub) in enumerate(data):
                m = _measure(aa, cc, pp, cd, 100, 25, generator=Generator(50 + i))
                alone.append(m.run_greedy(sub, st, None))
                tails.append(m._generator.u32())
            ms = [_measure(aa, cc, pp, cd, 100, 25, generator=Generator(50 + i)) for i, (aa, cc, pp, st, cd, sub) in enumerate(data)]
            multi = EfficientBatchMI.run_greedy_multi(ms, [d[5] for d in data], [d[3] for d in data])
        finally:
            os.environ.pop("ACAV_FY_LEGACY", None)
        for i, (aa, cc, pp, st, cd, sub) in enumerate(data):
            assert multi[i][0] == alone[i][0] and multi[i][1] == alone[i][1], (legacy, i)
            assert ms[i]._generator.u32() == tails[i]
            r = O.BatchMI(aa, cc, pp).run_greedy(cd, st, sub, 100, 25, O.Rng(50 + i))
            assert multi[i][0] == r["S"].tolist() and np.array_equal(np.array(multi[i][1]), r["GAIN"])


def test_score_batch_of_100(env, route_case):
    torch, acav, O = env
    a, c, pairs, start, cand, subset, ref = route_case
    m = _measure(a, c, pairs, cand, 100, 25)
    sel = cand[:400]
    m.add_samples(sel)
    om = O.BatchMI(a, c, pairs)
    om.add_samples(sel)
    ids = np.array(cand[400:500])
    assert np.array_equal(m.score_batch(ids), om.scores_canon(ids))
    ids = np.array(cand[400:1424])  # 1024 ids x 3 pairs
    assert np.array_equal(m.score_batch(ids), om.scores_canon(ids))


# ------------------------------------------------------------------ 5. the narrow path at its boundary
@pytest.mark.parametrize("B,k,v,subset", [(64, 16, 1500, 320), (20, 4, 600, 120)])
def test_narrow_path_equals_oracle(env, B, k, v, subset):
    _check_equals_oracle(env, v, 3, 16, B, k, True, subset)


# ------------------------------------------------------------------ 6. refusals
def test_refusals_name_the_limit(env):
    torch, acav, O = env
    a, pairs, start, cand = _inputs(3000, 2, 8)
    with pytest.raises(ValueError, match=r"batch_size 1025 .*<= 1024"):
        _measure(a, 8, pairs, cand, 1025, 25).run_greedy(100, start, None)
    with pytest.raises(ValueError, match=r"selection_size 101 .*selection_size <= batch_size"):
        _measure(a, 8, pairs, cand, 100, 101).run_greedy(202, start, None)
    with pytest.raises(ValueError, match=r"1025 .*B<=1024"):
        _measure(a, 8, pairs, cand, 100, 25).score_batch(np.arange(1025))
    a10, pairs10, start10, cand10 = _inputs(1000, 10, 8)
    with pytest.raises(ValueError, match=r"B\*P<=8192"):
        _measure(a10, 8, pairs10, cand10, 200, 50).run_greedy(100, start10, None)
    from acav100m_amd.rng import Generator
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    ms = [_measure(a10, 8, pairs10, cand10, 200, 50, generator=Generator(i)) for i in range(2)]
    with pytest.raises(ValueError, match=r"B\*P <= 8192"):
        EfficientBatchMI.run_greedy_multi(ms, [100, 100], [start10, start10])
    m = _measure(a, 8, pairs, cand, 100, 25)  # the handle still works after a refusal elsewhere
    assert len(m.run_greedy(50, start, None)[0]) == 50


# ------------------------------------------------------------------ 7. the CLI at the paper grid's setting
def test_cli_run_batch_100_selection_25(env, tmp_path_factory, golden_dir, monkeypatch):
    """`cli.py run --batch.batch_size=100 --batch.selection_size=25` on the synthetic shards of the CLI tests: the selected set
    is the oracle's for the same seed (ACAV_SEED)"""
    torch, acav, O = env
    import csv
    sys.path.insert(0, golden_dir)
    import synth
    from acav100m_amd import shards as io
    from acav100m_amd.clustering.cli import Cli as ClusterCli
    from acav100m_amd.subset_selection import cli as subset_cli
    root = str(tmp_path_factory.mktemp("acav_cli_wide"))
    glob = synth.write_feature_shards(root, n_shards=4, rows=256, seed=0)
    acav.manual_seed(0)
    ClusterCli().cluster(feature_path=glob, out_path=os.path.join(root, "clusters"), meta_path=os.path.join(root, "videos"),
                         **{"computation.num_workers": 0})
    out_csv = os.path.join(root, "output.csv")
    monkeypatch.setenv("ACAV_SEED", "3")
    monkeypatch.setenv("ACAV_NO_GROUP", "1")
    for key in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(key, raising=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # configure_runtime() after the first device call of the test process
        subset_cli.main(["run", "--shards_path=" + os.path.join(root, "clusters", "shard-{000000..000003}.pkl"),
                         "--meta_path=" + os.path.join(root, "videos"), "--out_path=" + out_csv,
                         "--batch.batch_size=100", "--batch.selection_size=25"])
    rows = list(csv.reader(open(out_csv)))
    assert len(rows) == 205
    paths = [os.path.join(root, "clusters", "shard-%06d.pkl" % s) for s in range(4)]
    a, types, shard_names, filenames = io.load_assignment_shards(paths)
    random.seed(3)
    cand = list(range(len(a)))
    random.shuffle(cand)
    pairs = list(itertools.combinations(range(len(types)), 2))
    res = O.BatchMI(a, int(a.max()) + 1, pairs).run_greedy(cand[1:], cand[:1], 205, 100, 25, O.Rng(3))
    assert [r[1] for r in rows] == [filenames[s] for s in sorted(res["S"])]
