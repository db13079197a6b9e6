"""GPU: acav_kmeanspp_weights and acav_kmeanspp_seed at the trial counts the LDS split and init_trials='auto' really produce, and
at a sample of more than 256 blocks, bit for bit.

Trial counts: a sweep is instantiated for NT = 1, 2, 4, 8, 16 trials and runs ntau <= NT of them; T = 3, 5, 6, 7, 9, 12, 15 are the
partial ones, and when T x dpad floats exceed the 64 KB of LDS the trials go in several sweeps with a ragged last one.  Against
the numpy restatement (tests/_kmeanspp_np.py).

More than 256 blocks of 1024 rows: k_kpp_sample scans the block sums in chunks of 256, k_kpp_best sums them strided, and the
sweep and select kernels (grids capped at 8 and 4 workgroups per compute unit) take a second round of rows.  The restatement is
too slow there (its draw is a python loop), so the rows are INTEGERS in [-512, 512]: every difference, square and partial sum
is then an exact float64 integer whatever the order of the sum, the weight is ((x_i - x_c)^2).sum() << t in int64, and the draw
is np.cumsum + searchsorted(side='right').  That shortcut is tied to the restatement at m = 2100 below."""
import numpy as np
import pytest

from tests import _kmeanspp_np as P

pytestmark = pytest.mark.gpu

B = P.BLOCK
PARTIAL_TS = [3, 5, 6, 7, 9, 12, 15]
AUTO = {32: 5, 64: 6, 256: 7}  # K -> 2 + floor(ln K)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def cus(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rows(seed, m, d):
    rs = np.random.RandomState(seed)
    return (rs.randn(m, d) * np.exp(rs.uniform(-2, 2, d))).astype(np.float32)


def _u(seed, k, T):
    return np.random.RandomState(seed).random_sample(1 + (k - 1) * T)


def _sweeps(d, T):
    """the trials per sweep: floor(16384 / dpad) at a time, at most 16"""
    per = min(16, 16384 // (-(-d // 256) * 256))
    return [min(per, T - a) for a in range(0, T, per)]


# ---- partial trial counts

@pytest.fixture(scope="module")
def small(torch):
    """per d: the rows (m = B + 1) on both sides and their shift"""
    out = {}
    for d in (65, 100, 1100, 2304):
        x = _rows(d, B + 1, d)
        out[d] = (x, torch.from_numpy(x).cuda(), P.shift_of(np.abs(x).max(), B + 1, d))
    return out


@pytest.mark.parametrize("T", PARTIAL_TS)
@pytest.mark.parametrize("d", [65, 100, 2304])
def test_weights_and_seeds_with_a_partial_trial_count(torch, small, d, T):
    from acav100m_amd.clustering import kmeanspp
    x, xt, t = small[d]
    m = len(x)
    if d == 2304:
        assert _sweeps(d, T) == {3: [3], 5: [5], 6: [6], 7: [7], 9: [7, 2], 12: [7, 5], 15: [7, 7, 1]}[T]
    else:
        assert _sweeps(d, T) == [T]
    rs = np.random.RandomState(100 * d + T)
    cand = rs.randint(0, m, T).astype(np.int64)
    cand[0], cand[-1] = m - 1, 0
    want = P.weights(x, cand, t)
    assert np.array_equal(kmeanspp.weights(xt, cand, t), want)
    assert np.array_equal(kmeanspp.weights(x, cand, t), want)  # host rows
    k = 3 if d < 1000 else 2  # (the restatement's cost is k T sweeps in numpy)
    u = _u(d + T, k, T)
    want = P.seed(x, k, T, u)
    got = kmeanspp.seed(xt, k, T, u=u)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_sixteen_trials_in_sweeps_of_twelve_and_four(torch, small):
    from acav100m_amd.clustering import kmeanspp
    d, T, k = 1100, 16, 2
    x, xt, t = small[d]
    m = len(x)
    assert -(-d // 256) * 256 == 1280 and _sweeps(d, T) == [12, 4]
    cand = np.random.RandomState(1).randint(0, m, T).astype(np.int64)
    cand[0], cand[11], cand[12], cand[-1] = m - 1, 5, B, 0
    assert np.array_equal(kmeanspp.weights(xt, cand, t), P.weights(x, cand, t))
    u = _u(2, k, T)
    want = P.seed(x, k, T, u)
    got = kmeanspp.seed(xt, k, T, u=u)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("K", sorted(AUTO))
def test_auto_trials_resolve_to_partial_counts_and_seed_the_restatements_rows(torch, small, K):
    """init_trials='auto' at K = 32, 64, 256 is T = 5, 6, 7: K seeds with that many trials, resolved by the driver"""
    from acav100m_amd.clustering import kmeanspp
    T = kmeanspp.trials_for(K, 'auto')
    assert T == AUTO[K] == P.trials_for(K, 'auto') and T in PARTIAL_TS
    x, xt, _t = small[65]
    u = _u(K, K, T)
    want = P.seed(x, K, T, u)
    got = kmeanspp.seed(xt, K, 'auto', u=u)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(set(got[0].tolist())) == K


# ---- more than 256 blocks: integer rows and an integer reference

def _int_weights(x, cand_rows, t):
    """-> int64 [T, m]: exact for integer-valued rows, whatever the order of the sum"""
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi.astype(np.float32), x) and t >= 0
    return np.stack([((xi - xi[int(c)]) ** 2).sum(axis=1) << t for c in cand_rows])


def _int_seed(x, k, T, u, t):
    """the picks of the module's definition with integer weights -> (rows, potential, the candidate rows of every pick)"""
    m = len(x)
    rows, potential, tried = np.empty(k, np.int64), np.empty(k, np.int64), []
    rows[0] = min(m - 1, int(u[0] * m))
    w = _int_weights(x, [rows[0]], t)[0]
    potential[0] = int(w.sum())
    for s in range(1, k):
        run = np.cumsum(w)
        total = int(run[-1])
        assert 0 < total < 2 ** 62
        best, cands = None, []
        for tau in range(T):
            target = min(total - 1, int(float(u[1 + (s - 1) * T + tau]) * float(total)))
            r = int(np.searchsorted(run, target, side='right'))  # the least i with w_0 + ... + w_i > target
            cands.append(r)
            cand = np.minimum(w, _int_weights(x, [r], t)[0])
            pot = int(cand.sum())
            if best is None or pot < best[0]:
                best = (pot, r, cand)
        potential[s], rows[s], w = best
        tried.append(cands)
    return rows, potential, tried


def _int_rows(seed, m, d=4):
    x = np.random.RandomState(seed).randint(-512, 513, size=(m, d)).astype(np.float32)
    x[m // 2, 0] = 512  # (absmax is 512 whatever was drawn)
    return x


def test_the_integer_reference_is_the_restatement():
    """(no device) the shortcut and tests/_kmeanspp_np agree where the latter is affordable"""
    for m, d in ((2100, 4), (1500, 7), (1100, 300)):
        x = _int_rows(m + d, m, d)
        t = P.shift_of(512, m, d)
        cand = np.array([0, m - 1, m // 2, 17, B + 3], np.int64)
        assert np.array_equal(_int_weights(x, cand, t), P.weights(x, cand, t)), (m, d)
    x = _int_rows(1, 2100)
    t = P.shift_of(512, 2100, 4)
    u = _u(2, 3, 5)
    u[3], u[8] = 0.0, 1 - 2.0 ** -53
    got, want = _int_seed(x, 3, 5, u, t), P.seed(x, 3, 5, u)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.fixture(scope="module")
def large(torch, cus):
    """integer rows in more than 256 blocks, and past one round of the sweep's and the select kernel's grids"""
    m = max(257, cus + 1) * B + 5  # 257 x 1024 + 5 at 256 units: the last block holds five rows
    nb = -(-m // B)
    x = _int_rows(3, m)
    t = P.shift_of(np.abs(x).max(), m, 4)
    assert nb > 256 + 1                                    # k_kpp_sample: a second chunk of block sums; k_kpp_best: strided
    assert -(-m // 16) > 4 * 8 * cus                       # k_kpp_sweep: runs of 16 rows, four per workgroup, 8 per unit
    assert m > 256 * 4 * cus                               # k_kpp_select: 4 workgroups of 256 threads per unit
    assert np.abs(x).max() == 512 and (cus != 256 or (m == 257 * B + 5 and t == 18))
    return x, torch.from_numpy(x).cuda(), t, m, nb


def test_weights_at_more_than_256_blocks(torch, large):
    from acav100m_amd.clustering import kmeanspp
    x, xt, t, m, nb = large
    assert kmeanspp.weight_shift(512, m, 4) == t
    cand = np.array([0, m - 1, m - 3, 255 * B + 1023, 256 * B], np.int64)  # the first and the last row, one of the last block
    want = _int_weights(x, cand, t)
    assert int(want.sum(axis=1).max()) < 2 ** 62
    got = kmeanspp.weights(xt, cand, t)
    assert got.shape == (5, m) and np.array_equal(got, want)
    assert np.array_equal(kmeanspp.weights(x, cand, t), want)  # host rows


def _aimed(x, t, u0, T, blocks):
    """per block b of `blocks` a u whose pick-1 target falls in the middle of block b's share of the weight, given pick 0"""
    m = len(x)
    w = _int_weights(x, [min(m - 1, int(u0 * m))], t)[0]
    run = np.cumsum(w)
    total = int(run[-1])
    out = []
    for b in blocks:
        lo = int(run[b * B - 1]) if b else 0
        hi = int(run[min(m, (b + 1) * B) - 1])
        assert hi - lo > 2 ** 20  # (a target in the middle stays inside whatever u x total rounds to)
        out.append(((lo + hi) // 2) / total)
    return out


def test_seeds_at_more_than_256_blocks(torch, large):
    from acav100m_amd.clustering import kmeanspp
    x, xt, t, m, nb = large
    k, T = 3, 5

    def check(u, host=False):
        want = _int_seed(x, k, T, u, t)
        got = kmeanspp.seed(xt, k, T, u=u)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), u
        if host:
            got = kmeanspp.seed(x, k, T, u=u)  # host rows
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), u
        return want

    want = check(_u(4, k, T), host=True)  # random uniforms
    assert int(want[1].max()) < 2 ** 62
    # all five trials of pick 1 aimed at one block -- block 0, the last block of the first chunk of 256, the first block of the
    # second chunk, the last (five-row) block: the pick is that block's row whichever trial wins; pick 2 from random uniforms
    u0 = 0.37
    blocks = [0, 255, 256, nb - 1]
    for b, ub in zip(blocks, _aimed(x, t, u0, T, blocks)):
        u = _u(5 + b, k, T)
        u[0], u[1:1 + T] = u0, ub
        want = check(u)
        assert want[2][0] == [want[0][1]] * T and want[0][1] // B == b, b
    # one trial each in those blocks and a random one, then the edge uniforms in pick 2
    u = _u(6, k, T)
    u[0], u[1:1 + len(blocks)] = u0, _aimed(x, t, u0, T, blocks)
    u[1 + T], u[2 + T] = 0.0, 1 - 2.0 ** -53
    want = check(u, host=True)
    assert [r // B for r in want[2][0][:len(blocks)]] == blocks
    # u = 0 and the largest double below 1 in every trial: the first and the last row of non-zero weight
    for edge, row in ((0.0, 0), (1 - 2.0 ** -53, m - 1)):
        u = np.full(1 + (k - 1) * T, edge)
        u[0] = u0
        want = check(u)
        assert want[0][1] == row
