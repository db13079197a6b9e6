"""The yardstick of the wide batch greedy (batch_size > 64) beyond the oracle's reach.

The oracle's batch greedy takes any batch_size but at most 64 picks per iteration; for larger selection sizes the GPU tests
(test_gpu_wide_batch.py) compare against tests/_weights_ref.py WeightedMI(..., weights=None).run_batch, the numpy restatement
of the same float64 operations in the same order.  Here that restatement is tied to the pinned yardsticks, on the CPU:
bit for bit to the oracle at (batch_size, selection_size) = (100, 25) and (160, 40), and to the reference's own recorded
traces at those settings (tests/golden/mi_wide_*.npz, teacher-forced on the reference's picks)."""
import itertools
import os

import numpy as np
import pytest

from tests._weights_ref import WeightedMI


def _correlated(seed, v, dd, c):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    a = np.stack(cols, 1).astype(np.int64)
    a[0] = c - 1
    return a


@pytest.mark.parametrize("v,dd,c,B,k,subset,keep", [(1500, 2, 16, 100, 25, 300, True), (2000, 4, 32, 160, 40, 400, True),
                                                    (1500, 3, 16, 100, 25, 250, False)])
def test_restatement_equals_oracle(v, dd, c, B, k, subset, keep):
    from oracle import oracle as O
    a = _correlated(v + dd, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    cand = [int(i) for i in np.random.RandomState(v).permutation(v)]
    start, cand = cand[:1], cand[1:]
    rng_o, rng_r = O.Rng(13), O.Rng(13)
    ref = O.BatchMI(a, c, pairs).run_greedy(cand, start, subset, B, k, rng_o, keep_unselected=keep)
    S, G = WeightedMI(a, pairs, c).run_batch(cand, start, subset, B, k, rng_r, keep_unselected=keep)
    assert S == ref["S"].tolist()
    assert np.array_equal(np.array(G), ref["GAIN"])  # float64, bit for bit
    assert rng_o.u32() == rng_r.u32()  # the same number of draws


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_follows_the_reference_traces(golden_dir, name):
    """teacher-forced on the reference's picks: its batches give the restatement's scores to fp32 accuracy (the tolerances of
    test_gpu_mi.py::test_golden_trace_teacher_forced), and where the restatement's own top k differs the reference was at a
    near-tie"""
    g = np.load(os.path.join(golden_dir, f"mi_wide_{name}.npz"))
    a, c = g["assignments"], int(g["C"])
    B, k = int(g["B"]), int(g["k"])
    pairs = list(itertools.combinations(range(a.shape[1]), 2))
    assert g["ids"].shape[1] == B and g["pick_pos"].shape[1] == k and B > 64
    m = WeightedMI(a, pairs, c)
    m.commit([int(g["shuffled"][0])])
    ref_mean = g["scores"].astype(np.float64).mean(-1)
    S, GAIN, diff = [], [], 0
    for t, batch in enumerate(g["ids"]):
        sc = m.scores(batch)
        np.testing.assert_allclose(sc, ref_mean[t], rtol=1e-5, atol=1e-6)
        own = np.lexsort((np.arange(B), -sc))[:k]
        if set(own.tolist()) != set(g["pick_pos"][t].tolist()):
            srt = np.sort(ref_mean[t])[::-1]
            assert abs(srt[k - 1] - srt[k]) <= 2e-6 * max(abs(srt[k - 1]), 1e-3), (t, srt[:k + 1])
            diff += 1
        picks = [int(batch[p]) for p in g["pick_pos"][t]]
        GAIN += [float(sc[p]) for p in g["pick_pos"][t]]
        S += picks
        m.commit(picks)
    assert S[:len(g["S"])] == g["S"].tolist()
    np.testing.assert_allclose(GAIN, g["GAIN"], rtol=1e-5, atol=1e-6)
    print(f"mi_wide_{name}: {diff}/{len(g['ids'])} iterations differ from the reference picks, all at near-ties")
