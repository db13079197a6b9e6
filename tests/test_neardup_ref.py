"""CPU: the numpy restatement of the near-duplicate rule (tests/_neardup_np.py) against a brute force over all pairs, on
planted copies, a chain, singletons and zero rows; and clustering/dedup.py's pure functions flag and summarise."""
import numpy as np

from tests import _neardup_np as R


def _rows(seed, n, d, k):
    rs = np.random.RandomState(seed)
    return rs.randn(n, d).astype(np.float32), rs.randint(0, k, n).astype(np.int64)


def test_the_restatement_equals_a_brute_force_over_all_pairs():
    x, lab = _rows(0, 90, 7, 3)
    x[17] = 0.0
    x[89] = x[3]  # a bitwise copy, as the last row: no later row sees the two as an exact tie
    lab[89] = lab[3]
    best, partner, second = R.nearest_earlier(x, lab)
    want_best, want_partner = R.brute_force(x, lab)
    ok = np.isfinite(want_best)
    assert np.array_equal(np.isfinite(best), ok)
    assert np.abs(best[ok] - want_best[ok]).max() <= 2 * R.bound(7)
    assert (best[ok] - second[ok]).min() > 4 * R.bound(7)  # every partner is decided
    assert np.array_equal(partner, want_partner)
    assert (second <= best).all()


def test_planted_bitwise_copies_are_found_at_their_first_occurrence():
    x, lab = _rows(1, 200, 24, 4)
    src = np.array([0, 5, 9, 33, 70])
    dst = np.array([100, 101, 150, 160, 199])
    x[dst], lab[dst] = x[src], lab[src]
    x[180], lab[180] = x[9], lab[9]  # a third copy: the partner is the FIRST occurrence, not the nearer copy
    best, partner, _ = R.nearest_earlier(x, lab)
    for s, t in list(zip(src, dst)) + [(9, 180)]:
        assert abs(best[t] - 1.0) <= R.bound(24) and partner[t] == s
    others = np.setdiff1d(np.arange(200), np.append(dst, 180))
    assert best[others].max() < 0.99


def test_a_chain_flags_b_and_c_and_keeps_a():
    from acav100m_amd.clustering.dedup import flag
    a = np.array([1.0, 0.0, 0.0], np.float32)
    b = np.array([np.cos(0.3), np.sin(0.3), 0.0], np.float32)
    c = np.array([np.cos(0.6), np.sin(0.6), 0.0], np.float32)
    best, partner, _ = R.nearest_earlier(np.stack([a, b, c]), np.zeros(3, np.int64))
    thr = float(np.cos(0.4))  # a ~ b and b ~ c, a and c apart
    assert abs(best[1] - np.cos(0.3)) < 1e-6 and abs(best[2] - np.cos(0.3)) < 1e-6
    assert list(partner) == [-1, 0, 1]  # c's nearest earlier row is b, flagged or not: the rule is not transitive
    assert list(flag(best, thr)) == [False, True, True]


def test_singletons_and_zero_rows():
    x = np.array([[1, 2], [0, 0], [3, 4], [0, 0], [5, 6], [2, 4]], np.float32)
    lab = np.array([0, 1, 1, 1, 2, 1], np.int64)
    best, partner, _ = R.nearest_earlier(x, lab, 4)
    # row 0 and row 4 are alone; row 1 is a zero row and first; row 2 has only a zero row before it; row 3 is a zero row;
    # row 5 = 2 * row 0 in another cluster: it sees row 2 only
    assert list(partner) == [-1, -1, -1, -1, -1, 2]
    assert np.isneginf(best[:5]).all() and best[5] == (3 * 2 + 4 * 4) / np.sqrt(25.0 * 20.0)


def test_flag_and_summarise_on_hand_made_arrays():
    from acav100m_amd.clustering.dedup import SIMILARITY_GRID, flag, summarise
    best = np.array([-np.inf, 0.97, 0.2, -np.inf, 1.0, -np.inf, 0.9999, 0.55])
    partner = np.array([-1, 0, 0, -1, 3, -1, 4, 1], np.int64)
    labels = np.array([0, 0, 0, 2, 2, 0, 2, 0], np.int64)  # row 5: a zero row of cluster 0
    assert list(flag(best, 0.97)) == [False, True, False, False, True, False, True, False]
    assert list(flag(best, 1.0)) == [False, False, False, False, True, False, False, False]
    rep = summarise(best, partner, labels, 3, 0.97)
    assert SIMILARITY_GRID == (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99, 0.999, 0.9999)
    assert rep == {'n': 8, 'K': 3, 'threshold': 0.97, 'flagged': 3, 'flagged_share': 3 / 8, 'flagged_by_cluster': [1, 0, 2],
                   'zero_rows': 1,
                   'similarity_counts': {'0.5': 4, '0.6': 3, '0.7': 3, '0.8': 3, '0.9': 3, '0.95': 3, '0.98': 2, '0.99': 2,
                                         '0.999': 2, '0.9999': 2}}
    assert list(rep['similarity_counts']) == [repr(g) for g in SIMILARITY_GRID]
