"""GPU tests of the XCD subset of the gather (gs_block_map; ACAV_GS_XCDS = 1, 2, 4 runs the gather workgroups of
k_fy_gather_select_multi on that many of the eight XCDs, ACAV_GS_XCD_ROT=1 moves the set every launch, 8 is the grid without
padding): where the workgroups run must not change a result.  The free-running selection (picks in pick order, gains) is
compared bit for bit between 8 and every other setting and with the oracle, at the smallest shapes that take every path: a grid
that populates every class and loses a workgroup mid-run, a grid shorter than one row of eight, the wide and the weighted
instantiations, and chunks in lockstep, which keep their grid.  ACAV_GS_XCD_MIN_L=0 lets lists this short take the subset form;
the switches are read at every call, so one process runs all settings."""
import itertools
import re

import numpy as np
import pytest

from tests import _weights_ref as WR

pytestmark = pytest.mark.gpu

SETTINGS = [(n, rot) for n in (4, 2, 1) for rot in (0, 1)]
TIMING = re.compile(r"gather grid: (\d+) XCD\(s\), rotation (\d+), subset form in (\d+) launch\(es\), all eight in (\d+)")


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


def _set(monkeypatch, n, rot):
    monkeypatch.setenv("ACAV_GS_XCD_MIN_L", "0")
    monkeypatch.setenv("ACAV_GS_XCDS", str(n))
    monkeypatch.setenv("ACAV_GS_XCD_ROT", str(rot))


def _single(acav, monkeypatch, n, rot, data, c, B, k, subset, seed):
    _set(monkeypatch, n, rot)
    a, pairs, start, cand = data
    acav.manual_seed(seed)
    m = _build(a, c, pairs, cand, B, k)
    assert m.k == k
    S, GAIN, _, _ = m.run_greedy(subset, start, None)
    return list(S), np.array(GAIN)


def _check_single(env, monkeypatch, v, c, B, k, subset, seed):
    torch, acav, O = env
    data = _inputs(seed + 100, v, 2, c)
    a, pairs, start, cand = data
    ref = O.BatchMI(a, c, pairs).run_greedy(cand, start, subset, B, k, O.Rng(seed), keep_unselected=True)
    S8, G8 = _single(acav, monkeypatch, 8, 0, data, c, B, k, subset, seed)
    assert S8 == list(ref["S"]) and np.array_equal(G8, ref["GAIN"])
    for n, rot in SETTINGS:
        S, G = _single(acav, monkeypatch, n, rot, data, c, B, k, subset, seed)
        assert S == S8 and np.array_equal(G, G8), (n, rot)
    return len(G8)


def test_the_grid_loses_a_block_mid_run(env, monkeypatch):
    """V = 19 533, 150 picks: the list shrinks from 19 532 to 19 384 over the 38 iterations and crosses 19 x 1 024 = 19 456, so the
    grid goes from 20 gather workgroups to 19 mid-run (V = 20 011 below stays at 20: 20 010 - 4 x 37 = 19 862)"""
    picks = _check_single(env, monkeypatch, 19533, 16, 20, 4, 150, 23)
    assert -(-picks // 4) == 38 and -(-19532 // 1024) == 20 and -(-(19532 - 4 * 37) // 1024) == 19


def test_every_class_populated(env, monkeypatch, capfd):
    """V = 20 011, B = 20, k = 4, 150 picks: 20 gather workgroups of 1 024 outputs, so every XCD class is populated; 38 iterations
    are two full groups of 16 and a partial one.  The loop's own ACAV_MI_TIMING line names the setting it ran with."""
    torch, acav, O = env
    picks = _check_single(env, monkeypatch, 20011, 16, 20, 4, 150, 17)
    iters = -(-picks // 4)
    assert iters == 38 and -(-20010 // 1024) == 20
    monkeypatch.setenv("ACAV_MI_TIMING", "1")
    data = _inputs(117, 20011, 2, 16)
    for n, rot in [(8, 0)] + SETTINGS:
        capfd.readouterr()
        _single(acav, monkeypatch, n, rot, data, 16, 20, 4, 150, 17)
        err = capfd.readouterr().err
        print(err)
        m = TIMING.search(err)
        assert m, err
        assert (int(m.group(1)), int(m.group(2))) == (n, rot)
        assert (int(m.group(3)), int(m.group(4))) == ((0, iters) if n == 8 else (iters, 0))


def test_fewer_blocks_than_one_row(env, monkeypatch):
    """V = 3 001, 22 picks: 3 gather workgroups, fewer than one row of 8, so some classes are empty; the list length is no
    multiple of 1 024"""
    assert 0 < -(-_check_single(env, monkeypatch, 3001, 16, 20, 4, 22, 9) // 4) < 8


def test_wide_batch(env, monkeypatch):
    """V = 6 007, B = 100, k = 25, 520 picks: the WIDE instantiations, where the hand-over loops over the re-queued positions"""
    assert _check_single(env, monkeypatch, 6007, 32, 100, 25, 520, 5) > 16 * 25


def test_weighted(env, monkeypatch):
    """layer weights (weight_type linear_1) at V = 3 001: the W instantiation.  The setting without a subset against the numpy
    float64 restatement of the weighted scores on the batches it drew, every other setting against it bit for bit."""
    torch, acav, O = env
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    v, dd, c, subset = 3001, 4, 16, 60
    a = _correlated(41, v, dd, c)
    keys = [(m, "layer_{}".format(i)) for m in ("SlowFast", "VGGish") for i in range(dd // 2)]
    comb = get_cluster_pairing(keys, "combination", "linear_1")
    order = [int(i) for i in np.random.RandomState(42).permutation(v)]
    start, cand = order[:1], order[1:]

    def run(n, rot, trace):
        _set(monkeypatch, n, rot)
        acav.manual_seed(5)
        m = _build(a, c, comb, cand, 20, 4)
        S, GAIN, _, _ = m.run_greedy(subset, start, None, record_trace=trace)
        return m, list(S), np.array(GAIN)

    m8, S8, G8 = run(8, 0, True)
    ref = WR.WeightedMI(a, comb["pairing"], c, comb["weights"])
    S_ref, G_ref, sc_ref, pos_ref = ref.run_batch_traced(start, m8.trace["ids"], m8.k)
    assert np.array_equal(m8.trace["scores"], sc_ref) and np.array_equal(m8.trace["pos"], pos_ref)
    assert S8 == S_ref[:len(S8)] and np.array_equal(G8, np.array(G_ref))
    for n, rot in SETTINGS:
        _, S, G = run(n, rot, False)
        assert S == S8 and np.array_equal(G, G8), (n, rot)


def test_lockstep_keeps_its_grid(env, monkeypatch, capfd):
    """three chunks (3 000 / 5 001 / 9 000) in lockstep with the switch at 2: the results equal the switch at 8 and the oracle,
    and the loop reports no launch in the subset form"""
    torch, acav, O = env
    from acav100m_amd.rng import Generator
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    specs = [(3000, 2, 16, 84), (5001, 3, 24, 44), (9000, 2, 64, 164)]
    data = [_inputs(200 + i, v, dd, c) for i, (v, dd, c, _) in enumerate(specs)]
    monkeypatch.setenv("ACAV_MI_TIMING", "1")

    def run(n):
        _set(monkeypatch, n, 0)
        capfd.readouterr()
        ms = [_build(a, specs[i][2], pairs, cand, 20, 4, generator=Generator(70 + i)) for i, (a, pairs, start, cand) in enumerate(data)]
        out = EfficientBatchMI.run_greedy_multi(ms, [s[3] for s in specs], [d[2] for d in data])
        err = capfd.readouterr().err
        print(err)
        m = TIMING.search(err)
        assert m and "3 chunk(s)" in err, err
        assert int(m.group(1)) == n and int(m.group(3)) == 0 and int(m.group(4)) == 41  # the longest chunk's iterations
        return [(list(o[0]), np.array(o[1])) for o in out]

    two, eight = run(2), run(8)
    for i, (a, pairs, start, cand) in enumerate(data):
        assert two[i][0] == eight[i][0] and np.array_equal(two[i][1], eight[i][1]), f"chunk {i}"
        ref = O.BatchMI(a, specs[i][2], pairs).run_greedy(cand, start, specs[i][3], 20, 4, O.Rng(70 + i), keep_unselected=True)
        assert two[i][0] == ref["S"].tolist() and np.array_equal(two[i][1], ref["GAIN"]), f"chunk {i}"
