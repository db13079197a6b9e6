"""The tiled Fisher-Yates with 4-byte bucket entries (the default for lists of at most 4 Mi candidates) against the
8-byte entries (ACAV_FY_PACK=0): the same selected ids, traces, float64 gains and generator state, over list lengths that
are not multiples of the part block (8192 steps) or of a tile, lists a few tiles long, the forced tile overload path,
lockstep chunks of unequal length, and both sides of the longest list the packed form takes."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PACK_MAX = 512 * 8192  # part workgroups of one iteration the entry can name (6 bits + the shard) x steps per workgroup


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    from oracle import oracle as O
    return torch, acav100m_amd, O


def _labels(seed, v, dd, c):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, size=v)
    a = np.stack([np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)], 1).astype(np.int64)
    a[0] = c - 1
    return a


def _run(acav, a, c, subset, seed, max_iters=-1):
    from acav100m_amd.subset_selection import get_measure
    v, dd = a.shape
    cand = [int(i) for i in np.random.RandomState(seed).permutation(v)]
    acav.manual_seed(seed)
    m = get_measure("batch_mi")(a, ncentroids=c, batch_size=20, selection_size=4, device="cuda:0", keep_unselected=True)
    m.init(list(itertools.combinations(range(dd), 2)), cand[1:])
    S, G, _, _ = m.run_greedy(subset, cand[:1], None, record_trace=True, max_iters=max_iters)
    mt, idx = acav.default_generator.get_state()
    return S, np.array(G), np.array(m.trace["ids"]), np.array(mt), idx


def _same(x, y):
    assert x[0] == y[0]
    for p, q in zip(x[1:], y[1:]):
        assert np.array_equal(p, q)


@pytest.mark.parametrize("v,subset,ecap", [
    (40, 12, None),           # a list of one tile, a few iterations
    (300, 60, None),          # a few tiles
    (20000, 1200, None),      # several part blocks: not a multiple of 8192
    (20000, 1200, "64"),      # every loaded tile sub-ranged (ACAV_FY_ECAP)
    (140001, 400, None),      # more than 8 part blocks: shards receive several workgroups each
])
def test_packed_equals_int2_entries(env, monkeypatch, v, subset, ecap):
    torch, acav, O = env
    if ecap:
        monkeypatch.setenv("ACAV_FY_ECAP", ecap)
    a = _labels(v, v, 2, 32)
    monkeypatch.setenv("ACAV_FY_PACK", "0")
    wide = _run(acav, a, 32, subset, 7)
    monkeypatch.delenv("ACAV_FY_PACK")
    packed = _run(acav, a, 32, subset, 7)
    _same(packed, wide)


@pytest.mark.parametrize("v", [PACK_MAX, PACK_MAX + 1])
def test_longest_packed_list_vs_oracle(env, v):
    """4 Mi candidates: part workgroups 0..511, the largest the entry can name (the packed form); one more candidate
    and the loop keeps the 8-byte entries -- both equal the oracle over the first iterations."""
    torch, acav, O = env
    c, iters = 64, 6
    rs = np.random.RandomState(4)
    a = rs.randint(0, c, (v, 2)).astype(np.int64)
    a[0] = c - 1
    S, G, _, mt, idx = _run(acav, a, c, 4 * iters, 11, max_iters=iters)
    cand = [int(i) for i in np.random.RandomState(11).permutation(v)]
    rng = O.Rng(11)
    ref = O.BatchMI(a, c, [(0, 1)]).run_greedy(cand[1:], cand[:1], 4 * iters, 20, 4, rng, max_iters=iters)
    assert S == list(ref["S"]) and np.array_equal(G, ref["GAIN"])
    mt_o, idx_o = rng.get_state()
    assert idx_o == idx and np.array_equal(mt_o, mt)


def test_lockstep_unequal_chunks_packed_equals_int2(env, monkeypatch):
    torch, acav, O = env
    from acav100m_amd.rng import Generator
    from acav100m_amd.subset_selection import get_measure
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    specs = [(3000, 2, 16, 300), (70001, 2, 64, 120), (900, 3, 8, 100), (16385, 2, 32, 37)]

    def run():
        ms, subsets, starts = [], [], []
        for i, (v, dd, c, subset) in enumerate(specs):
            a = _labels(300 + i, v, dd, c)
            cand = np.random.RandomState(i).permutation(v)
            m = get_measure("batch_mi")(a, ncentroids=c, batch_size=20, selection_size=4, device="cuda:0",
                                        keep_unselected=True, generator=Generator(80 + i))
            m.init(list(itertools.combinations(range(dd), 2)), [int(j) for j in cand[1:]])
            ms.append(m)
            subsets.append(subset)
            starts.append([int(cand[0])])
        out = EfficientBatchMI.run_greedy_multi(ms, subsets, starts)
        return out, [m._generator.u32() for m in ms]

    monkeypatch.setenv("ACAV_FY_PACK", "0")
    wide, wide_tails = run()
    monkeypatch.delenv("ACAV_FY_PACK")
    packed, packed_tails = run()
    assert packed_tails == wide_tails
    for p, w in zip(packed, wide):
        assert list(p[0]) == list(w[0]) and np.array_equal(np.array(p[1]), np.array(w[1]))
