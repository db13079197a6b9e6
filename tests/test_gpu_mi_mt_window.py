"""One free-running batch_mi selection long enough to take its draws from many generator lanes, against the oracle bit
for bit: V = 40 000 clips, C = 16, two views, B = 20, k = 4, 1 500 iterations.  The 1 500 permutations of 39 999 down to
34 003 candidates take about 55 M draws: 22 lane blocks of 624 * 4096 words, so 22 generator workgroups each sliding their
LDS window some 450 times, and every lane but the first placed by the streaming jump kernel (one to four hops of the lane
spread).  One wrong word anywhere in the stream changes a permutation and, with it, the selection."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_long_free_running_selection_equals_oracle():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd as acav
    acav.load_library()
    from acav100m_amd.subset_selection import get_measure
    from oracle import oracle as O
    v, c, dd, B, k, iters = 40_000, 16, 2, 20, 4, 1500
    subset = iters * k
    rs = np.random.RandomState(16)
    comp = rs.randint(0, c, size=v)
    a = np.stack([np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)], 1).astype(np.int64)
    a[0] = c - 1
    pairs = list(itertools.combinations(range(dd), 2))
    cand = [int(i) for i in rs.permutation(v)]
    start, cand = [cand[0]], cand[1:]
    acav.manual_seed(16)
    m = get_measure("batch_mi")(a, ncentroids=c, batch_size=B, selection_size=k, device="cuda:0", keep_unselected=True)
    m.init(pairs, cand)
    S, GAIN, _, _ = m.run_greedy(subset, start, None)
    rng = O.Rng(16)
    ref = O.BatchMI(a, c, pairs).run_greedy(cand, start, subset, B, k, rng)
    assert ref["iters"] == iters
    assert len(S) == subset and list(S) == list(ref["S"])
    assert np.array_equal(np.array(GAIN), ref["GAIN"])  # same float64 operations, same order
    # the host generator continues where the device stream ended
    mt_o, idx_o = rng.get_state()
    mt_p, idx_p = acav.default_generator.get_state()
    assert idx_o == idx_p and np.array_equal(mt_o, mt_p)
