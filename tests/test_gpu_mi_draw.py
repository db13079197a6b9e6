"""GPU tests of batch.sampler=draw (acav_mi_run_draw, k_mi_draw): the device result equals the numpy restatement
(tests/_draw_sampler_np.py) bit for bit -- batches, picks, S, GAIN as float64, tables and the generator state afterwards.  The
restatement takes its draws, scores and commits from the oracle (O.Rng.u32, O.BatchMI.scores_canon / add_samples / counts), or,
for weighted pairs, from a second device handle's score_batch / add_samples.

Sizes crossed: B <= 64 (one wave ranks) and B > 64 (the workgroup ranks), B P up to and beyond the staged limits of the selection
(2048, 256), windows so small that steps swap inside the batch (one thread walks the steps) and lists so long that none does
(the steps resolve in parallel), generator blocks (624 words), launches (ACAV_DRAW_GROUP), more chunks than compute units.
Not crossed: lists beyond 16 Mi candidates (nothing in the kernel depends on that size)."""
import itertools

import numpy as np
import pytest

from tests import _draw_sampler_np as R

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


def _correlated(seed, v, dd, c):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    a = np.stack(cols, 1).astype(np.int64)
    a[0] = c - 1
    return a


def _measure(a, c, pairs, cand, B, k, keep, seed, sampler='draw', weights=None):
    from acav100m_amd.rng import Generator
    from acav100m_amd.subset_selection import get_measure
    m = get_measure("batch_mi")(a, ncentroids=c, batch_size=B, selection_size=k, device="cuda:0", keep_unselected=keep,
                                generator=Generator(seed), sampler=sampler)
    m.init(pairs if weights is None else {'pairing': pairs, 'weights': weights}, cand)
    return m


def _problem(v, dd, c, seed=0):
    a = _correlated(v + dd + seed, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    cand = [int(i) for i in np.random.RandomState(v + seed).permutation(v)]
    return a, pairs, cand[:1], cand[1:]


def _restate(O, a, c, pairs, cand, start, subset, B, k, keep, seed, weights=None, max_iters=-1):
    """-> (restatement's result, its tables (N, a, b, n), the generator it drew from)"""
    rng = O.Rng(seed)
    if weights is None:
        om = O.BatchMI(a, c, pairs)
        om.add_samples(start)
        ref = R.run_draw(cand, subset, B, k, keep, rng.u32, om.scores_canon, om.add_samples, max_iters)
        return ref, om.counts(), rng
    m2 = _measure(a, c, pairs, cand, B, k, keep, 0, sampler='permutation', weights=weights)  # scores and commits only
    m2.add_samples(start)
    ref = R.run_draw(cand, subset, B, k, keep, rng.u32, m2.score_batch, m2.add_samples, max_iters)
    t = m2.cache
    return ref, (t['N'], t['a'], t['b'], t['n']), rng


def _check(m, S, GAIN, ref, tables, rng, trace=True):
    if trace:
        assert np.array_equal(m.trace["ids"], ref["ids"])
        assert np.array_equal(m.trace["pos"], ref["pos"])
        assert m.trace["scores"].tobytes() == ref["scores"].tobytes()
    assert list(S) == ref["S"].tolist()
    assert np.array(GAIN, np.float64).tobytes() == ref["GAIN"].tobytes()
    t = m.cache
    assert np.array_equal(t["N"], tables[0]) and np.array_equal(t["a"], tables[1]) and np.array_equal(t["b"], tables[2])
    assert t["n"] == tables[3]
    (mt_o, idx_o), (mt_p, idx_p) = rng.get_state(), m._generator.get_state()
    assert idx_o == idx_p and np.array_equal(mt_o, mt_p)


FREE = {
    "keep": (600, 3, 16, 20, 4, True, 120, None),
    "no-keep": (500, 2, 8, 20, 4, False, 60, None),
    "p45": (900, 10, 32, 20, 4, True, 180, None),
    "wide": (3000, 2, 32, 100, 25, True, 500, None),
    "b1024-p1": (3000, 2, 8, 1024, 256, True, 512, None),
    "b300-long-list": (200000, 2, 16, 300, 60, True, 600, None),  # more than one batch position per thread, targets outside
    "b-equals-k": (600, 3, 16, 20, 20, True, 100, None),
    "k1": (600, 3, 16, 20, 1, True, 30, None),
    "weighted": (600, 3, 16, 20, 4, True, 120, [0.5, 2.0, 1.25]),
    "weighted-wide": (1500, 3, 16, 100, 25, True, 200, [0.5, 2.0, 1.25]),
}


@pytest.mark.parametrize("name", list(FREE))
def test_free_run_equals_restatement(env, name):
    torch, acav, O = env
    v, dd, c, B, k, keep, subset, weights = FREE[name]
    a, pairs, start, cand = _problem(v, dd, c)
    m = _measure(a, c, pairs, cand, B, k, keep, 9, weights=weights)
    S, GAIN, _, _ = m.run_greedy(subset, start, None, record_trace=True)
    assert m.k == k
    ref, tables, rng = _restate(O, a, c, pairs, cand, start, subset, B, k, keep, 9, weights)
    _check(m, S, GAIN, ref, tables, rng)
    assert len(set(S)) == len(S) == subset and start[0] not in S
    assert len(GAIN) == ref["iters"] * k


# L0 between B and 2 B (most targets fall inside the window, several steps share a target); the last iteration starts at L == B
SMALL = {
    "keep-30": (31, 20, 4, True, 12),      # L0 = 30: iterations at L = 30, 26, 22
    "keep-last-B": (29, 20, 4, True, 12),  # L0 = 28: 28, 24, 20
    "no-keep-last-B": (61, 20, 4, False, 12),  # L0 = 60: 60, 40, 20
    "wide-last-B": (151, 100, 25, True, 75),   # L0 = 150: 150, 125, 100
    "wide-b-equals-l": (101, 100, 100, False, 100),  # L0 = B = k: one iteration, the batch is the whole list
}


@pytest.mark.parametrize("name", list(SMALL))
def test_small_windows(env, name):
    torch, acav, O = env
    v, B, k, keep, subset = SMALL[name]
    a, pairs, start, cand = _problem(v, 3, 8, seed=3)
    m = _measure(a, 8, pairs, cand, B, k, keep, 4)
    S, GAIN, _, _ = m.run_greedy(subset, start, None, record_trace=True)
    assert m.k == k
    ref, tables, rng = _restate(O, a, 8, pairs, cand, start, subset, B, k, keep, 4)
    # the case is what it claims: in the first iteration steps swap inside the batch and (but for L0 == B) share a target
    probe, L0 = O.Rng(4), len(cand)
    targets = [t + probe.u32() % (L0 - t) for t in range(B)]
    assert sum(1 for t, j in enumerate(targets) if t < j < B) > 0
    assert L0 == B or len(set(j for j in targets if j >= B)) < sum(1 for j in targets if j >= B)
    assert L0 - (ref["iters"] - 1) * (k if keep else B) == B or name == "keep-30"
    _check(m, S, GAIN, ref, tables, rng)


def test_launch_groups(env, monkeypatch):
    """ACAV_DRAW_GROUP=7: many launches; the window start, the tables and the generator pass between them in device memory"""
    torch, acav, O = env
    a, pairs, start, cand = _problem(600, 3, 16)
    monkeypatch.delenv("ACAV_DRAW_GROUP", raising=False)
    m = _measure(a, 16, pairs, cand, 20, 4, True, 9)
    S, GAIN, _, _ = m.run_greedy(120, start, None, record_trace=True)
    monkeypatch.setenv("ACAV_DRAW_GROUP", "7")
    from acav100m_amd.subset_selection.measures.batch import draw_form
    assert draw_form([len(cand)], [120], 20, 4, True)['launches'] == 5
    m7 = _measure(a, 16, pairs, cand, 20, 4, True, 9)
    S7, GAIN7, _, _ = m7.run_greedy(120, start, None, record_trace=True)
    assert S7 == S and GAIN7 == GAIN
    for key in ("ids", "pos", "scores"):
        assert np.array_equal(m7.trace[key], m.trace[key])
    ref, tables, rng = _restate(O, a, 16, pairs, cand, start, 120, 20, 4, True, 9)
    _check(m7, S7, GAIN7, ref, tables, rng)


@pytest.mark.parametrize("group", [None, "7"])
def test_generator_blocks(env, monkeypatch, group):
    """iters B = 2000 > 3 x 624 words: the draws cross generator blocks, within an iteration and at its edge"""
    torch, acav, O = env
    if group is None:
        monkeypatch.delenv("ACAV_DRAW_GROUP", raising=False)
    else:
        monkeypatch.setenv("ACAV_DRAW_GROUP", group)
    a, pairs, start, cand = _problem(2000, 2, 32)
    m = _measure(a, 32, pairs, cand, 20, 4, True, 21)
    S, GAIN, _, _ = m.run_greedy(400, start, None, record_trace=True)
    ref, tables, rng = _restate(O, a, 32, pairs, cand, start, 400, 20, 4, True, 21)
    assert ref["iters"] * 20 > 3 * 624
    _check(m, S, GAIN, ref, tables, rng)


@pytest.mark.parametrize("B,k", [(20, 4), (100, 25)])
def test_first_batch_is_the_permutation_samplers(env, B, k):
    torch, acav, O = env
    a, pairs, start, cand = _problem(3000, 2, 32)
    md = _measure(a, 32, pairs, cand, B, k, True, 5)
    md.run_greedy(10 * k, start, None, record_trace=True, max_iters=1)
    mp = _measure(a, 32, pairs, cand, B, k, True, 5, sampler='permutation')
    mp.run_greedy(10 * k, start, None, record_trace=True, max_iters=1)
    assert md.trace["ids"].shape == (1, B) and np.array_equal(md.trace["ids"], mp.trace["ids"])
    assert np.array_equal(md.trace["pos"], mp.trace["pos"]) and np.array_equal(md.trace["scores"], mp.trace["scores"])


def _chunks(specs):
    """specs: (rows, seed) -> per chunk (a, pairs, start, cand)"""
    return [_problem(v, 2, 8, seed=s) for v, s in specs]


def test_eight_unequal_chunks_each_as_alone(env):
    torch, acav, O = env
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    specs = [(300 + 97 * i, i) for i in range(8)]
    subsets = [40 + 12 * i for i in range(8)]  # 10 .. 31 iterations: the chunks end at different iterations of the launch
    probs = _chunks(specs)
    ms = [_measure(a, 8, pairs, cand, 20, 4, True, 70 + i) for i, (a, pairs, start, cand) in enumerate(probs)]
    res = EfficientBatchMI.run_greedy_multi(ms, subsets, [p[2] for p in probs])
    for i, (a, pairs, start, cand) in enumerate(probs):
        alone = _measure(a, 8, pairs, cand, 20, 4, True, 70 + i)
        S, GAIN, _, _ = alone.run_greedy(subsets[i], start, None)
        assert res[i][0] == S and res[i][1] == GAIN and len(S) == subsets[i]
        ta, tm = alone.cache, ms[i].cache
        assert all(np.array_equal(ta[key], tm[key]) for key in ("N", "a", "b")) and ta["n"] == tm["n"]
        (mt_a, idx_a), (mt_m, idx_m) = alone._generator.get_state(), ms[i]._generator.get_state()
        assert idx_a == idx_m and np.array_equal(mt_a, mt_m)


def test_more_chunks_than_compute_units(env):
    """one workgroup per chunk: with more chunks than the device has compute units a second round of workgroups runs"""
    torch, acav, O = env
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    n = torch.cuda.get_device_properties(0).multi_processor_count + 9
    a, pairs, _, _ = _problem(96, 2, 4)
    rs = np.random.RandomState(1)
    cands, starts, ms = [], [], []
    for i in range(n):
        order = [int(x) for x in rs.permutation(96)[:40 + i % 7]]
        starts.append(order[:1])
        cands.append(order[1:])
        ms.append(_measure(a, 4, pairs, cands[-1], 8, 2, True, 1000 + i))
    res = EfficientBatchMI.run_greedy_multi(ms, [6] * n, starts)
    for i in range(n):
        ref, tables, rng = _restate(O, a, 4, pairs, cands[i], starts[i], 6, 8, 2, True, 1000 + i)
        _check(ms[i], res[i][0], res[i][1], ref, tables, rng, trace=False)


def test_error_paths(env):
    torch, acav, O = env
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    a, pairs, start, cand = _problem(40, 3, 8)
    # 39 candidates, B = 20, k = 4, keep: iteration 5 would start at 19 < 20 -- refused up front, nothing touched
    m = _measure(a, 8, pairs, cand, 20, 4, True, 3)
    before = m._generator.get_state()
    S, G = np.full(40, -7, np.int64), np.full(40, -7.0, np.float64)
    with pytest.raises(RuntimeError, match="candidates left"):
        EfficientBatchMI._run_draw([m], [24], [np.array(start, np.int64)], [S], [G], [(None,) * 3], -1)
    assert (S == -7).all() and (G == -7.0).all() and m.cache["n"] == 0  # not even the start indices were added
    after = m._generator.get_state()
    assert before[1] == after[1] and np.array_equal(before[0], after[0])
    S20, _, _, _ = m.run_greedy(20, start, None)  # five iterations fit: 39, 35, 31, 27, 23
    assert len(S20) == 20
    # a short chunk refuses the whole call: no earlier chunk ran
    m0, m1 = _measure(a, 8, pairs, cand, 20, 4, True, 3), _measure(a, 8, pairs, cand[:21], 20, 4, True, 4)
    with pytest.raises(RuntimeError, match="chunk 1"):
        EfficientBatchMI.run_greedy_multi([m0, m1], [8, 12], [start, start])
    assert m0.cache["n"] == 0 and m1.cache["n"] == 0
    # the limits: selection_size > batch_size, B P > 8192
    with pytest.raises(ValueError, match="selection_size"):
        _measure(a, 8, pairs, cand, 20, 21, True, 3).run_greedy(21, start, None)
    a5, pairs5, start5, cand5 = _problem(1200, 5, 8)
    with pytest.raises(ValueError, match="8192"):
        _measure(a5, 8, pairs5, cand5, 1024, 256, True, 3).run_greedy(256, start5, None)
    # no teacher forcing
    with pytest.raises(ValueError, match="forced_pos"):
        _measure(a, 8, pairs, cand, 20, 4, True, 3).run_greedy(8, start, None, forced_pos=np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match="sampler"):
        _measure(a, 8, pairs, cand, 20, 4, True, 3, sampler='shuffle')
