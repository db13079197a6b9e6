"""GPU tests of the XCD-affine grids of k_fy_tile_multi / k_fy_resolve_multi (fy_block_map; ACAV_FY_XCD_AFFINE=0 restores the
3-D grids): the placement of the workgroups must not change a result.  The free-running selection (picks in pick order, gains)
is compared bit for bit between the two settings and with the oracle, at shapes where the position kernels take every path:
several tiles and sub-ranged tiles, full groups of 16 iterations plus a partial one, fewer than 8 iterations (the old order
inside the 1-D grid), lists that are no multiple of 256 or 8 192, chunks of unequal length in lockstep, and a wide batch.
The switch is read at every call, so one process runs both settings."""
import itertools
import re

import numpy as np
import pytest

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


def _inputs(seed, v, dd, c):
    a = _correlated(seed, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    cand = [int(i) for i in np.random.RandomState(seed + 1).permutation(v)]
    return a, pairs, cand[:1], cand[1:]


def _build(a, c, pairs, cand, B, k, generator=None):
    from acav100m_amd.subset_selection import get_measure
    kw = {} if generator is None else dict(generator=generator)
    m = get_measure("batch_mi")(a, ncentroids=c, batch_size=B, selection_size=k, device="cuda:0", keep_unselected=True, **kw)
    m.init(pairs, cand)
    return m


# V = 20 011: a list of 20 010 candidates (78 resolve workgroups and a part of one, 3 part workgroups), tiles of 256 positions
# (ACAV_FY_CAP) whose LDS holds 64 entries (ACAV_FY_ECAP): dozens of tiles, the loaded ones sub-ranged
# (test_single_chunk_switches_give_subranged_tiles_and_both_grids asserts both)
SINGLE = dict(seed=31, v=20011, dd=2, c=16, B=20, k=4)
_oracle_cache = {}


def _single_inputs():
    return _inputs(SINGLE["seed"], SINGLE["v"], SINGLE["dd"], SINGLE["c"])


def _single_oracle(O, subset):
    """the oracle's run of the single-chunk case, computed once per subset and shared"""
    if subset not in _oracle_cache:
        a, pairs, start, cand = _single_inputs()
        _oracle_cache[subset] = O.BatchMI(a, SINGLE["c"], pairs).run_greedy(cand, start, subset, SINGLE["B"], SINGLE["k"], O.Rng(17),
                                                                           keep_unselected=True)
    return _oracle_cache[subset]


def _single_run(acav, monkeypatch, affine, subset):
    monkeypatch.setenv("ACAV_FY_XCD_AFFINE", affine)
    a, pairs, start, cand = _single_inputs()
    acav.manual_seed(17)
    m = _build(a, SINGLE["c"], pairs, cand, SINGLE["B"], SINGLE["k"])
    assert m.k == SINGLE["k"]
    S, GAIN, _, _ = m.run_greedy(subset, start, None)
    return list(S), np.array(GAIN)


# 150 picks of 4: two full groups of 16 iterations and a partial third; 22 picks: fewer than 8 iterations, the old order
@pytest.mark.parametrize("subset", [150, 22])
def test_single_chunk_same_selection_either_grid(env, monkeypatch, subset):
    torch, acav, O = env
    monkeypatch.setenv("ACAV_FY_CAP", "256")
    monkeypatch.setenv("ACAV_FY_ECAP", "64")
    S1, G1 = _single_run(acav, monkeypatch, "1", subset)
    S0, G0 = _single_run(acav, monkeypatch, "0", subset)
    iters = -(-len(S1) // SINGLE["k"])
    assert (iters > 2 * 16 and iters % 16 != 0) if subset == 150 else 0 < iters < 8
    assert S1 == S0 and np.array_equal(G1, G0)
    ref = _single_oracle(O, subset)
    assert S1 == list(ref["S"]) and np.array_equal(G1, ref["GAIN"])


def test_single_chunk_switches_give_subranged_tiles_and_both_grids(env, monkeypatch, capfd):
    """What the single-chunk cases above rely on, read from the loop's own ACAV_MI_TIMING line.  Several tiles, and at least one
    sub-ranged: a tile is sub-ranged when it holds more entries than its LDS lists (ACAV_FY_ECAP = 64, below the plan's 256), every
    step of an iteration whose draw moves an item is one entry (L - 1 steps, of which ln L = 10 on average draw themselves), so
    with tiles x 64 < (L - 1) / 2 some tile of the first iteration holds more than 64.  And the switch picks the launch form:
    150 picks of 4 are 3 groups, all 1-D under =1 and all 3-D under =0."""
    torch, acav, O = env
    monkeypatch.setenv("ACAV_FY_CAP", "256")
    monkeypatch.setenv("ACAV_FY_ECAP", "64")
    monkeypatch.setenv("ACAV_MI_TIMING", "1")
    for affine, forms in (("1", (3, 0)), ("0", (0, 3))):
        capfd.readouterr()
        _single_run(acav, monkeypatch, affine, 150)
        err = capfd.readouterr().err
        print(err)
        m = re.search(r"tiles (\d+), cap (\d+), .*1-D XCD-affine in (\d+) group\(s\), 3-D in (\d+)", err)
        assert m, err
        tiles, cap = int(m.group(1)), int(m.group(2))
        assert tiles > 8 and 64 < cap and tiles * 64 < (SINGLE["v"] - 2) // 2
        assert (int(m.group(3)), int(m.group(4))) == forms


def test_single_chunk_default_tiles(env, monkeypatch):
    """the tiling the product runs with (no capacity switch), the switch unset against =0"""
    torch, acav, O = env
    monkeypatch.delenv("ACAV_FY_XCD_AFFINE", raising=False)
    a, pairs, start, cand = _single_inputs()
    acav.manual_seed(17)
    m = _build(a, SINGLE["c"], pairs, cand, SINGLE["B"], SINGLE["k"])
    S, GAIN, _, _ = m.run_greedy(150, start, None)
    S0, G0 = _single_run(acav, monkeypatch, "0", 150)
    assert list(S) == S0 and np.array_equal(np.array(GAIN), G0)
    ref = _single_oracle(O, 150)
    assert S0 == list(ref["S"]) and np.array_equal(G0, ref["GAIN"])


def test_lockstep_chunks_same_selection_either_grid(env, monkeypatch):
    """three chunks of unequal length and unequal iteration counts in lockstep: 21, 11 and 41 iterations in the order of
    the specs (84, 44 and 164 picks of 4), so the second chunk leaves in the first group, the first in the second, and the last
    group of the launch holds 9 iterations of the third chunk alone"""
    torch, acav, O = env
    from acav100m_amd.rng import Generator
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    specs = [(3000, 2, 16, 84), (5001, 3, 24, 44), (9000, 2, 64, 164)]
    data = [_inputs(200 + i, v, dd, c) for i, (v, dd, c, _) in enumerate(specs)]

    def run(affine):
        monkeypatch.setenv("ACAV_FY_XCD_AFFINE", affine)
        ms = [_build(a, specs[i][2], pairs, cand, 20, 4, generator=Generator(70 + i)) for i, (a, pairs, start, cand) in enumerate(data)]
        out = EfficientBatchMI.run_greedy_multi(ms, [s[3] for s in specs], [d[2] for d in data])
        return [(list(o[0]), np.array(o[1])) for o in out]

    on, off = run("1"), run("0")
    its = set()
    for i, (a, pairs, start, cand) in enumerate(data):
        assert on[i][0] == off[i][0] and np.array_equal(on[i][1], off[i][1]), f"chunk {i}"
        ref = O.BatchMI(a, specs[i][2], pairs).run_greedy(cand, start, specs[i][3], 20, 4, O.Rng(70 + i), keep_unselected=True)
        assert on[i][0] == ref["S"].tolist() and np.array_equal(on[i][1], ref["GAIN"]), f"chunk {i}"
        its.add(-(-len(on[i][1]) // 4))
    assert len(its) == 3 and max(its) > 32 and min(its) < 16


def test_wide_batch_same_selection_either_grid(env, monkeypatch):
    """B = 100, k = 25 (the wide launches: k_fy_resolve_multi<true>), 21 iterations"""
    torch, acav, O = env
    a, pairs, start, cand = _inputs(77, 6007, 2, 32)

    def run(affine):
        monkeypatch.setenv("ACAV_FY_XCD_AFFINE", affine)
        acav.manual_seed(5)
        m = _build(a, 32, pairs, cand, 100, 25)
        assert m.k == 25
        S, GAIN, _, _ = m.run_greedy(520, start, None)
        return list(S), np.array(GAIN)

    (S1, G1), (S0, G0) = run("1"), run("0")
    assert S1 == S0 and np.array_equal(G1, G0) and len(G1) > 16 * 25
    ref = O.BatchMI(a, 32, pairs).run_greedy(cand, start, 520, 100, 25, O.Rng(5), keep_unselected=True)
    assert S1 == list(ref["S"]) and np.array_equal(G1, ref["GAIN"])


@pytest.mark.parametrize("affine", ["1", "0"])
def test_overflow_flag_still_fires(env, monkeypatch, affine):
    """A tile whose LDS holds 16 entries (the smallest ACAV_FY_ECAP) is sub-ranged down to single positions; the last list
    position is pulled by step j with probability 1 / (L - j), H(L) - 1 = 9.5 times on average at L = 20 010, and more than 16
    times in about one iteration of 50 (Poisson tail).  Over 600 iterations some sub-range overflows (all pass: 0.98^600 < 1e-5):
    the error flag is raised in k_fy_tile_multi and the run is refused, under either grid."""
    torch, acav, O = env
    monkeypatch.setenv("ACAV_FY_ECAP", "16")
    monkeypatch.setenv("ACAV_FY_XCD_AFFINE", affine)
    a, pairs, start, cand = _single_inputs()
    acav.manual_seed(17)
    m = _build(a, SINGLE["c"], pairs, cand, SINGLE["B"], SINGLE["k"])
    with pytest.raises(RuntimeError, match="overflowed"):
        m.run_greedy(2401, start, None)
