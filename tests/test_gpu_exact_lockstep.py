"""GPU: the exact-greedy and pair-counting measures over several chunks in lockstep (acav_mi_run_exact_multi,
EfficientMI.run_greedy_multi).  The loop has no generator in it and its order (score descending, original position
ascending, NaN first for the pair scores) is total, so chunk c of a lockstep call must yield BIT FOR BIT what
measures[c].run_greedy yields alone: picks, gains, tables, pair sums and the shrunken candidate list.  Every chunk is built
twice from the same seeded data; one copy runs alone, the other in the multi call.  No tolerance anywhere."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (V, D, C, subset): L = V - 1 candidates beside the start clip.  L = 255: one workgroup with an idle lane; 256: exactly
# one; 257: a second workgroup that holds one candidate; 1000: four.  Low C and correlated labels make exact ties frequent.
# D / P / C differ (P = 1 ... 6); the subset sizes differ, so the chunks finish at different launches; chunk 1 asks for
# more picks than it has candidates (the whole list is taken); chunk 4 has subset - 1 - ns = 0: nothing is selected.
SPECS = [(256, 2, 8, 60), (257, 3, 8, 300), (258, 4, 16, 90), (1001, 3, 12, 130), (38, 2, 8, 2)]

MEASURES = [("mi", None), ("mem_mi", None), ("ami", "arithmetic"), ("ami", "max"), ("nmi", "min"), ("constant", None),
            ("fm", None), ("rand", None), ("arand", None)]
PAIR = ("fm", "rand", "arand")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


def _correlated(seed, v, dd, c):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    a = np.stack(cols, 1).astype(np.int64)
    a[0] = c - 1
    return a


def _data(specs=SPECS):
    data = []
    for i, (v, dd, c, subset) in enumerate(specs):
        a = _correlated(700 + i, v, dd, c)
        cand = [int(j) for j in np.random.RandomState(i).permutation(v)]
        data.append((a, c, list(itertools.combinations(range(dd), 2)), cand, subset))
    return data


def _build(name, avg, d, comb=None):
    from acav100m_amd.subset_selection import get_measure
    a, c, pairs, cand, _ = d
    kw = {} if avg is None else {"average_method": avg}
    m = get_measure(name)(a, ncentroids=c, device="cuda:0", **kw)
    m.init(pairs if comb is None else comb, cand[1:])
    return m


def _state(m):
    """everything a run leaves behind: the tables, the pair counts (pair measures) and the candidate list"""
    st = dict(m.cache)
    if hasattr(m, "pair_stats"):
        st.update(m.pair_stats())
    st["candidate_ids"] = np.array(m.candidate_ids)
    return st


def _same_state(x, y):
    return x.keys() == y.keys() and all(np.array_equal(x[k], y[k]) for k in x)


def _same_result(multi, alone):
    """S with ==; GAIN with == too, NaN-aware (arand scores 0/0 while the selection is degenerate); timelapse / LOOKUPS by shape"""
    assert multi[0] == alone[0]
    assert len(multi[1]) == len(alone[1])
    assert np.array_equal(np.array(multi[1], np.float64), np.array(alone[1], np.float64), equal_nan=True)
    if not any(g != g for g in alone[1]):
        assert multi[1] == alone[1]
    assert len(multi[2]) == len(alone[2]) == len(alone[1])
    assert multi[3] == alone[3] == [0] * len(alone[1])


def _tied_picks(m, cand, S, ns):
    """picks of a traced single run made among >= 2 remaining candidates of equal top score (NaN counts as equal to NaN)"""
    pos_of = {c: p for p, c in enumerate(cand)}
    alive = np.ones(len(cand), bool)
    tied = 0
    for t, s in enumerate(S[ns:]):
        row, p = m.trace["scores"][t], pos_of[s]
        assert alive[p]
        top = row[p]
        same = np.isnan(row[alive]) if top != top else row[alive] == top
        assert same.sum() >= 1 and (top != top or not (row[alive] > top).any())
        tied += int(same.sum() >= 2)
        alive[p] = False
    return tied


@pytest.mark.parametrize("name,avg", MEASURES, ids=["{}-{}".format(n, a) if a else n for n, a in MEASURES])
def test_mixed_chunks_equal_single_runs(env, name, avg):
    from acav100m_amd.subset_selection import get_measure
    data = _data()
    n = len(data)
    alone, states, tied = [], [], 0
    for d in data:
        m = _build(name, avg, d)
        cand = [int(c) for c in m.candidate_ids]
        alone.append(m.run_greedy(d[4], [d[3][0]], None, record_trace=True))
        tied += _tied_picks(m, cand, alone[-1][0], 1)
        states.append(_state(m))
    assert tied >= 1, "no pick among equal top scores: the position rule is not exercised"
    if name == "arand":  # one start clip: the first picks are taken while every score is 0/0 (NaN first, lowest position)
        assert all(g != g for r in alone[:4] for g in r[1][:1])
    ms = [_build(name, avg, d) for d in data]
    before = _state(ms[4])
    multi = get_measure(name).run_greedy_multi(ms, [d[4] for d in data], [[d[3][0]] for d in data])
    assert len(multi) == n
    for i in range(n):
        _same_result(multi[i], alone[i])
        assert _same_state(_state(ms[i]), states[i]), "chunk {}".format(i)
    assert len(multi[1][0]) == 1 + 256 and len(ms[1].candidate_ids) == 0  # more picks asked for than candidates: all taken
    assert multi[4][0] == [data[4][3][0]] and multi[4][1] == []            # subset - 1 - ns = 0: nothing selected
    if name not in PAIR:  # (a pair measure's start clip has joined its tables, as in run_greedy)
        assert _same_state(_state(ms[4]), before)
    assert [len(r[1]) for r in multi] == [58, 256, 88, 128, 0]


def test_weighted_mi_equals_single_runs_and_mixing_raises(env):
    from acav100m_amd.subset_selection import get_measure
    from acav100m_amd.subset_selection.pairing import get_weights
    specs = [(400, 4, 8, 70), (258, 4, 16, 40), (700, 4, 12, 100)]
    data = _data(specs)
    combs = [get_weights(None, d[2], "linear_1") for d in data]
    assert len(combs[0]["weights"]) == 6 and len(set(combs[0]["weights"])) > 1
    alone, states = [], []
    for d, comb in zip(data, combs):
        m = _build("mi", None, d, comb)
        alone.append(m.run_greedy(d[4], [d[3][0]], None))
        states.append(_state(m))
    plain = _build("mi", None, data[0]).run_greedy(data[0][4], [data[0][3][0]], None)
    assert plain[0] != alone[0][0] or plain[1] != alone[0][1], "the weights change nothing: the case does not test them"
    ms = [_build("mi", None, d, comb) for d, comb in zip(data, combs)]
    multi = get_measure("mi").run_greedy_multi(ms, [d[4] for d in data], [[d[3][0]] for d in data])
    for i in range(len(data)):
        _same_result(multi[i], alone[i])
        assert _same_state(_state(ms[i]), states[i])
    # a weighted handle beside an unweighted one: refused, both left as they were
    mw, mu = _build("mi", None, data[0], combs[0]), _build("mi", None, data[1])
    sw, su = _state(mw), _state(mu)
    with pytest.raises(ValueError, match="chunks 0 and 1 differ"):
        get_measure("mi").run_greedy_multi([mw, mu], [30, 30], [[data[0][3][0]], [data[1][3][0]]])
    assert _same_state(_state(mw), sw) and _same_state(_state(mu), su)


def _raw_single(m, cand, ns, subset):
    from acav100m_amd import _lib
    cand = np.ascontiguousarray(cand, np.int64)
    S, G, nsel = np.full(int(subset) + 1, -1, np.int64), np.zeros(int(subset) + 1, np.float64), C.c_int64(-7)
    _lib.check(_lib._lib.acav_mi_run_exact(m._h, _lib.ptr(cand), len(cand), int(ns), int(subset), _lib.ptr(S), _lib.ptr(G),
                                           C.byref(nsel), None, None, None))
    return S[:nsel.value].tolist(), G[:nsel.value].tolist()


def test_second_call_carries_the_pair_sums(env):
    """fm, two chunks: a multi call for a subset of 40, then a second multi call for 40 more picks, equals the same two calls
    made with run_greedy alone.  run_greedy re-derives the pair sums (its add_samples resets the residues, as the
    reference's does), so the same is then done through the C ABI with nothing in between, on tables sparse enough (C = 48,
    6 picks) that the float64-eps residues of the first call are still alive when the second starts: the pair sums and
    their validity flag are carried from call to call as acav_mi_run_exact carries them."""
    from acav100m_amd.subset_selection import get_measure
    data = _data([(300, 3, 8, 40), (500, 2, 6, 40)])
    alone, states = [], []
    for d in data:
        m = _build("fm", None, d)
        alone.append((m.run_greedy(40, [d[3][0]], None), m.run_greedy(41, [], None)))
        states.append(_state(m))
    ms = [_build("fm", None, d) for d in data]
    first = get_measure("fm").run_greedy_multi(ms, [40, 40], [[d[3][0]] for d in data])
    second = get_measure("fm").run_greedy_multi(ms, [41, 41], [[], []])
    for i in range(2):
        _same_result(first[i], alone[i][0])
        _same_result(second[i], alone[i][1])
        assert len(first[i][1]) == 38 and len(second[i][1]) == 40
        assert not set(first[i][0]) & set(second[i][0])
        assert _same_state(_state(ms[i]), states[i])
    # the C ABI, no add_samples between the calls
    data = _data([(300, 3, 64, 0), (500, 2, 48, 0)])
    want = []
    for d in data:
        m = _build("fm", None, d)
        m.add_samples(d[3][:1])
        S1, G1 = _raw_single(m, d[3][1:], 1, 8)
        rest = [c for c in d[3][1:] if c not in set(S1)]
        S2, G2 = _raw_single(m, rest, 7, 14)
        assert len(S1) == 6 and len(S2) == 6
        want.append((S1, G1, rest, S2, G2, _state(m)))
    ms = [_build("fm", None, d) for d in data]
    for m, d in zip(ms, data):
        m.add_samples(d[3][:1])
    rc, S, G, nsel = _raw_multi(ms, [d[3][1:] for d in data], [1, 1], [8, 8])
    assert rc == 0 and nsel.tolist() == [6, 6]
    for i in range(2):
        assert S[i][:6].tolist() == want[i][0] and G[i][:6].tolist() == want[i][1]
    rc, S, G, nsel = _raw_multi(ms, [w[2] for w in want], [7, 7], [14, 14])
    assert rc == 0 and nsel.tolist() == [6, 6]
    for i in range(2):
        assert S[i][:6].tolist() == want[i][3] and G[i][:6].tolist() == want[i][4]
        ms[i].candidate_ids = want[i][5]["candidate_ids"]  # the raw calls do not maintain the Python-side list
        assert _same_state(_state(ms[i]), want[i][5])


def test_golden_chunk_in_a_group(env, golden_dir):
    """One chunk of a `mi` group is the committed exact-greedy golden case mi_exact_a, built as test_gpu_mi's exact-greedy
    test builds it.  That test replays the reference's recorded picks (forced positions); the lockstep call takes none, so
    the chunk runs free here and is held to (1) the oracle's free-running exact greedy, S and GAIN bit for bit -- the
    oracle is what test_oracle_golden ties to the reference's trace -- and (2) the golden S itself up to the first pick at
    which the reference's fp32 scores chose another member of an exact tie of the canonical float64 scores."""
    from acav100m_amd.subset_selection import get_measure
    from oracle import oracle as O
    g = np.load(os.path.join(golden_dir, "mi_exact_a.npz"))
    a, c, subset, cand = g["assignments"], int(g["C"]), int(g["subset"]), [int(i) for i in g["shuffled"]]
    pairs = list(itertools.combinations(range(a.shape[1]), 2))
    gold = (a, c, pairs, cand, subset)
    others = _data(SPECS[:2])
    group = [others[0], gold, others[1]]
    single = _build("mi", None, gold)
    cand0 = [int(i) for i in single.candidate_ids]
    alone = single.run_greedy(subset, cand[:1], None, record_trace=True)
    ms = [_build("mi", None, d) for d in group]
    multi = get_measure("mi").run_greedy_multi(ms, [d[4] for d in group], [[d[3][0]] for d in group])
    _same_result(multi[1], alone)
    assert _same_state(_state(ms[1]), _state(single))
    ref = O.BatchMI(a, c, pairs).run_exact(np.array(cand[1:]), np.array(cand[:1]), subset)
    assert multi[1][0][1:] == [int(s) for s in ref["S"]] and len(multi[1][0]) == subset - 1
    assert np.array_equal(np.array(multi[1][1]), ref["GAIN"])  # float64, bit for bit
    S_gold = g["mi_S"].tolist()
    assert len(S_gold) == len(multi[1][0]) and S_gold[0] == multi[1][0][0]
    t = next((i for i in range(1, len(S_gold)) if S_gold[i] != multi[1][0][i]), None)
    if t is not None:  # the reference's pick at the first divergence scores exactly what ours does
        row = single.trace["scores"][t - 1]
        assert row[cand0.index(S_gold[t])] == row[cand0.index(multi[1][0][t])] == alone[1][t - 1]


def _raw_multi(ms, cands, ns, subset):
    from acav100m_amd import _lib
    n = len(ms)
    S = [np.full(int(s) + 1, -1, np.int64) for s in subset]
    G = [np.zeros(int(s) + 1, np.float64) for s in subset]

    def parr(ptrs):
        return (C.c_void_p * n)(*[p.value if isinstance(p, C.c_void_p) else p for p in ptrs])
    cands = [np.ascontiguousarray(c, np.int64) for c in cands]
    L = np.array([len(c) for c in cands], np.int64)
    nsel = np.full(n, -7, np.int64)
    rc = _lib._lib.acav_mi_run_exact_multi(parr([m._h for m in ms]), n, parr([_lib.ptr(c) for c in cands]), _lib.ptr(L),
                                           _lib.ptr(np.array(ns, np.int32)), _lib.ptr(np.array(subset, np.int64)),
                                           parr([_lib.ptr(x) for x in S]), parr([_lib.ptr(x) for x in G]), _lib.ptr(nsel))
    return rc, S, G, nsel


def test_errors_leave_every_handle_as_it_was(env):
    from acav100m_amd import _lib
    from acav100m_amd.subset_selection import get_measure
    EINVAL = -1  # ACAV_EINVAL (include/acav_hip.h); _lib.check turns it into ValueError

    def last_error():
        return _lib._lib.acav_last_error().decode()
    data = _data(SPECS[:3])
    starts = [[d[3][0]] for d in data]

    def untouched(ms, states):
        for m, st in zip(ms, states):
            assert _same_state(_state(m), st) and st["n"] == m.cache["n"]

    # two measure classes (mi and mem_mi are two): ValueError before any device call
    ms = [_build("mi", None, data[0]), _build("mem_mi", None, data[1]), _build("mi", None, data[2])]
    states = [_state(m) for m in ms]
    with pytest.raises(ValueError, match="share their measure"):
        get_measure("mi").run_greedy_multi(ms, [20, 20, 20], starts)
    untouched(ms, states)
    ms = [_build("ami", "arithmetic", data[0]), _build("ami", "max", data[1])]
    states = [_state(m) for m in ms]
    with pytest.raises(ValueError, match="average_method"):
        get_measure("ami").run_greedy_multi(ms, [20, 20], starts[:2])
    untouched(ms, states)
    # a pair measure's start clips join no table before the arguments are checked
    ms = [_build("fm", None, data[0]), _build("rand", None, data[1])]
    states = [_state(m) for m in ms]
    with pytest.raises(ValueError, match="share their measure"):
        get_measure("fm").run_greedy_multi(ms, [20, 20], starts[:2])
    untouched(ms, states)
    # the same measure object twice, through Python and through the raw call
    ms = [_build("mi", None, data[0]), _build("mi", None, data[1])]
    states = [_state(m) for m in ms]
    with pytest.raises(ValueError, match="twice"):
        get_measure("mi").run_greedy_multi([ms[0], ms[1], ms[0]], [20, 20, 20], starts)
    rc, _, _, nsel = _raw_multi([ms[0], ms[1], ms[0]], [data[0][3][1:], data[1][3][1:], data[0][3][1:]], [1, 1, 1], [20, 20, 20])
    assert rc == EINVAL and "chunks 0 and 2 share a handle" in last_error() and (nsel == -7).all()
    untouched(ms, states)
    # fm with an empty table in the LAST chunk, through the raw call (run_greedy_multi would add the start clips)
    ms = [_build("fm", None, data[0]), _build("fm", None, data[1])]
    ms[0].add_samples(starts[0])
    states = [_state(m) for m in ms]
    rc, _, _, nsel = _raw_multi(ms, [ms[0].candidate_ids, ms[1].candidate_ids], [1, 1], [20, 20])
    assert rc == EINVAL and "chunk 1" in last_error() and "no sample" in last_error()
    assert (nsel == -7).all()
    untouched(ms, states)
    # a candidate id >= V in the last chunk
    ms = [_build("mi", None, d) for d in data]
    states = [_state(m) for m in ms]
    bad = np.array(ms[2].candidate_ids)
    bad[-1] = data[2][0].shape[0]
    ms[2].candidate_ids = bad
    states[2]["candidate_ids"] = bad.copy()
    with pytest.raises(ValueError, match="chunk 2: candidate id 258 outside"):
        get_measure("mi").run_greedy_multi(ms, [20, 20, 20], starts)
    untouched(ms, states)
    # chunk counts outside 1 .. 64
    good = [_build("mi", None, data[0])]
    st = _state(good[0])
    rc, _, _, nsel = _raw_multi(good * 65, [data[0][3][1:]] * 65, [1] * 65, [20] * 65)
    assert rc == EINVAL and "65 chunks" in last_error() and (nsel == -7).all()
    cand = np.ascontiguousarray(data[0][3][1:], np.int64)
    S, G, nsel = np.full(21, -1, np.int64), np.zeros(21, np.float64), np.full(1, -7, np.int64)
    one = lambda x: (C.c_void_p * 1)(x.value)  # noqa: E731
    rc = _lib._lib.acav_mi_run_exact_multi(one(good[0]._h), 0, one(_lib.ptr(cand)), _lib.ptr(np.array([len(cand)], np.int64)),
                                           _lib.ptr(np.array([1], np.int32)), _lib.ptr(np.array([20], np.int64)),
                                           one(_lib.ptr(S)), one(_lib.ptr(G)), _lib.ptr(nsel))
    assert rc == EINVAL and "0 chunks" in last_error() and nsel[0] == -7 and S[0] == -1
    untouched(good, [st])


def test_one_chunk_equals_the_single_run(env):
    from acav100m_amd.subset_selection import get_measure
    for name in ("mi", "arand"):
        d = _data(SPECS[3:4])[0]
        m1, m2 = _build(name, None, d), _build(name, None, d)
        alone = m1.run_greedy(d[4], [d[3][0]], None)
        multi = get_measure(name).run_greedy_multi([m2], [d[4]], [[d[3][0]]])
        _same_result(multi[0], alone)
        assert _same_state(_state(m1), _state(m2))
