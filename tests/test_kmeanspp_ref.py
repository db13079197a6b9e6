"""CPU: the numpy restatement of the k-means++ seeding (tests/_kmeanspp_np.py) pinned against plain numpy, the host functions of
clustering/kmeanspp.py against the restatement, the refusals of the three keys, and the blob property the GPU tests rely on."""
import math

import numpy as np
import pytest

from tests import _kmeanspp_np as P


def _args(**over):
    from acav100m_amd.config import CLUSTERING_DEFAULTS, merge
    return merge(CLUSTERING_DEFAULTS, over)


def blobs(seed=0):
    """16 blobs of 64 rows in d = 32: centre 1000 e_b, sigma 1 -> (x fp32 [1024, 32] in a shuffled order, blob ids)"""
    rs = np.random.RandomState(seed)
    ids = np.repeat(np.arange(16), 64)
    rs.shuffle(ids)
    x = rs.randn(1024, 32)
    x[np.arange(1024), ids] += 1000.0
    return x.astype(np.float32), ids


@pytest.mark.parametrize("d", [1, 3, 63, 64, 65, 100, 257, 600])
def test_restated_distance_is_the_float64_sum_of_squares(d):
    rs = np.random.RandomState(d)
    x = (rs.randn(37, d) * 3).astype(np.float32)
    for c in (0, 36):
        got = P.sq_dist(x, x[c])
        want = ((x.astype(np.float64) - x[c].astype(np.float64)) ** 2).sum(axis=1)
        assert got[c] == 0.0
        # d additions of non-negative terms, each rounded once: relative error below d 2^-52 (one ulp = 2^-52 per addition)
        assert (np.abs(got - want) <= d * 2.0 ** -52 * want).all()
    t = P.shift_of(np.abs(x).max(), 37, d)
    w = P.weights(x, [0, 5], t)
    assert w.dtype == np.int64 and w.shape == (2, 37) and w[0, 0] == 0 and w[1, 5] == 0 and (w >= 0).all()


def test_draw_is_searchsorted_on_the_cumulative_sum():
    rs = np.random.RandomState(3)
    w = rs.randint(0, 5, 200).astype(np.int64) * rs.randint(0, 2, 200)  # many zeros, runs of them at both ends
    w[:7] = 0
    w[-9:] = 0
    total = int(w.sum())
    for target in [0, 1, total // 2, total - 2, total - 1] + list(rs.randint(0, total, 50)):
        i = P.draw(w, int(target))
        assert i == int(np.searchsorted(np.cumsum(w), target, side='right')) and w[i] > 0


@pytest.mark.parametrize("absmax", [1e-30, 1.0, 3e38])
def test_weight_shift_keeps_every_sum_below_2_62(absmax):
    from acav100m_amd.clustering.kmeanspp import weight_shift
    for m in (1, 2, 3, 1024, 1025, 2 ** 20 + 1, 2 ** 31 - 1):
        for d in (1, 2, 3, 64, 1000, 16384):
            t = weight_shift(absmax, m, d)
            assert t == P.shift_of(absmax, m, d) == 59 - P.bl(m) - P.bl(d) - 2 * math.frexp(absmax)[1]
            # the largest weight: every |e_j| = 2 absmax (fp32 values, so the products and, d a small integer, the sum are what
            # float64 gives for the bound), in python integers: the sum of m of them needs up to 62 bits
            a = float(np.float32(absmax))
            big = (2 * a) * (2 * a) * d * 2.0 ** t
            assert math.isfinite(big)
            assert m * int(round(big)) < 2 ** 62, (m, d, t)
            assert abs(t) <= 1000
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError):
            weight_shift(bad, 10, 4)
    with pytest.raises(ValueError):
        weight_shift(1.0, 0, 4)


def test_trials_for():
    from acav100m_amd.clustering.kmeanspp import trials_for
    assert trials_for(8, 1) == 1 and trials_for(8, 16) == 16 and trials_for(8, 5) == 5
    for k in (1, 2, 7, 8, 20, 21, 256, 1024, 10 ** 6, 10 ** 9):
        assert trials_for(k, 'auto') == P.trials_for(k, 'auto') == min(16, 2 + int(math.log(k)))
    assert trials_for(1, 'auto') == 2 and trials_for(8, 'auto') == 4 and trials_for(256, 'auto') == 7 and trials_for(1024, 'auto') == 8
    assert trials_for(10 ** 9, 'auto') == 16
    for bad in (0, 17, -1, 1.5, True, 'many', None):
        with pytest.raises(ValueError, match="init_trials"):
            trials_for(8, bad)


def test_uniforms_are_genrand_res53():
    from acav100m_amd.clustering.kmeanspp import uniforms

    class Words:
        def __init__(self, words):
            self.words = list(words)

        def u32(self):
            return self.words.pop(0)

    words = [0, 0, 2 ** 32 - 1, 2 ** 32 - 1, 1 << 31, 0, 31, 63, 32, 64, 0x12345678, 0x9abcdef0]
    got = uniforms(Words(words), 6)
    want = P.uniforms(Words(words).u32, 6)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert got[0] == 0.0 and got[1] == 1 - 2.0 ** -53 and got[2] == 0.5 and got[3] == 0.0 and got[4] == (2 ** 26 + 1) / 2.0 ** 53
    assert ((got >= 0) & (got < 1)).all()


def test_keys_parse_default_to_random_and_are_refused_when_wrong():
    from acav100m_amd.clustering.kmeanspp import check_init, sample_size
    from acav100m_amd.config import CLUSTERING_DEFAULTS, parse_cli
    c = CLUSTERING_DEFAULTS["clustering"]
    assert c["init"] == "random" and c["init_trials"] == 1 and c["init_sample"] is None
    command, kwargs = parse_cli(["cluster", "--clustering.algorithm=lloyd", "--clustering.init=kmeans++", "--clustering.init_trials=auto",
                                 "--clustering.init_sample=4096", "--feature_path=x"])
    assert command == "cluster" and kwargs["clustering.init"] == "kmeans++" and kwargs["clustering.init_trials"] == "auto"
    assert kwargs["clustering.init_sample"] == 4096
    assert check_init(_args(**kwargs)) == "kmeans++" and check_init(_args()) == "random"
    lloyd = {"clustering.algorithm": "lloyd", "clustering.init": "kmeans++", "clustering.ncentroids": 8}
    assert check_init(_args(**lloyd)) == "kmeans++"
    assert check_init(_args(**lloyd, **{"clustering.init_trials": 16, "clustering.init_sample": 8})) == "kmeans++"
    with pytest.raises(ValueError, match="algorithm=lloyd"):
        check_init(_args(**{"clustering.init": "kmeans++"}))  # sgd
    with pytest.raises(ValueError, match="algorithm=lloyd"):
        check_init(_args(**{"clustering.init": "kmeans++", "clustering.algorithm": "sgd"}))
    for bad in ("kmeans", "k-means++", "++", "", 1, True):
        with pytest.raises(ValueError, match="clustering.init must be"):
            check_init(_args(**{"clustering.algorithm": "lloyd", "clustering.init": bad}))
    for bad in (0, 17, "many", 2.5, True):
        with pytest.raises(ValueError, match="init_trials"):
            check_init(_args(**lloyd, **{"clustering.init_trials": bad}))
    for bad in (7, 0, -1, "all", 8.0, True):
        with pytest.raises(ValueError, match="init_sample"):
            check_init(_args(**lloyd, **{"clustering.init_sample": bad}))
    # init=random: the other two keys are not looked at
    check_init(_args(**{"clustering.init_trials": 99, "clustering.init_sample": 1}))
    assert sample_size(10 ** 6, 8) == 2048 and sample_size(1000, 8) == 1000 and sample_size(1000, 8, 500) == 500 and sample_size(100, 8, 500) == 100


def test_the_stage_refuses_the_keys_before_a_shard_is_read(tmp_path):
    from acav100m_amd.clustering import run_clustering as rc
    for over, words in (({"clustering.init": "kmeans++"}, "algorithm=lloyd"),
                        ({"clustering.algorithm": "lloyd", "clustering.init": "best"}, "clustering.init must be"),
                        ({"clustering.algorithm": "lloyd", "clustering.init": "kmeans++", "clustering.init_trials": 17}, "init_trials"),
                        ({"clustering.algorithm": "lloyd", "clustering.init": "kmeans++", "clustering.init_sample": 3}, "init_sample")):
        args = _args(**over, **{"data.output.path": str(tmp_path / "out"),
                                "data.path": str(tmp_path / "nowhere" / "shard-{000000..000003}.pkl")})
        with pytest.raises(ValueError, match=words):
            rc.run_clustering(args)


def test_library_refuses_bad_sizes_without_a_device():
    import ctypes as C
    import acav100m_amd
    lib = acav100m_amd.load_library()
    x = np.zeros((10, 4), np.float32)
    cand, out = np.zeros(2, np.int64), np.full((2, 10), 7, np.int64)
    u, rows, pot = np.zeros(5), np.full(3, 7, np.int64), np.full(3, 7, np.int64)
    xp, cp, op, up, rp, pp = (a.ctypes.data_as(C.c_void_p) for a in (x, cand, out, u, rows, pot))
    for args in ((0, None, 10, 4, cp, 2, 0, op), (0, xp, 10, 4, None, 2, 0, op), (0, xp, 10, 4, cp, 2, 0, None),
                 (0, xp, 0, 4, cp, 2, 0, op), (0, xp, 2 ** 31, 4, cp, 2, 0, op), (0, xp, 10, 0, cp, 2, 0, op),
                 (0, xp, 10, 16385, cp, 2, 0, op), (0, xp, 10, 4, cp, 0, 0, op), (0, xp, 10, 4, cp, 17, 0, op),
                 (0, xp, 10, 4, cp, 2, 1001, op), (0, xp, 10, 4, cp, 2, -1001, op)):
        assert lib.acav_kmeanspp_weights(*args, None) == -1, args
    for args in ((0, None, 10, 4, 3, 2, up, 0, rp, pp), (0, xp, 10, 4, 3, 2, None, 0, rp, pp), (0, xp, 10, 4, 3, 2, up, 0, None, pp),
                 (0, xp, 10, 4, 3, 2, up, 0, rp, None), (0, xp, 0, 4, 3, 2, up, 0, rp, pp), (0, xp, 10, 16385, 3, 2, up, 0, rp, pp),
                 (0, xp, 10, 4, 0, 2, up, 0, rp, pp), (0, xp, 10, 4, 11, 2, up, 0, rp, pp), (0, xp, 10, 4, 3, 0, up, 0, rp, pp),
                 (0, xp, 10, 4, 3, 17, up, 0, rp, pp), (0, xp, 10, 4, 3, 2, up, 1001, rp, pp)):
        assert lib.acav_kmeanspp_seed(*args, None) == -1, args
    assert (out == 7).all() and (rows == 7).all() and (pot == 7).all()


@pytest.mark.parametrize("trials", [1, 'auto'])
def test_blob_seeds_fall_in_16_different_blobs(trials):
    x, ids = blobs()
    T = P.trials_for(16, trials)
    rs = np.random.RandomState(11)
    u = rs.random_sample(1 + 15 * T)
    rows, potential = P.seed(x, 16, T, u)
    assert sorted(ids[rows]) == list(range(16))
    assert (np.diff(potential) < 0).all() and potential[-1] > 0


def test_restated_seeding_edges():
    rs = np.random.RandomState(2)
    x = rs.randn(40, 5).astype(np.float32)
    x[7] = x[3]
    # u = 0: the first row of non-zero weight; u = 1 - 2^-53: the last one
    rows, _ = P.seed(x, 3, 1, np.zeros(3))
    assert rows[0] == 0 and rows[1] == 1 and rows[2] == 2
    rows, _ = P.seed(x, 3, 2, np.full(5, 1 - 2.0 ** -53))
    assert rows[0] == 39 and rows[1] == 38 and rows[2] == 37
    # duplicates are never drawn twice; one centre too many is an error
    y = np.repeat(x[:6], 3, axis=0)
    rows, potential = P.seed(y, 6, 1, rs.random_sample(6))
    assert sorted(rows // 3) == list(range(6)) and potential[-1] == 0
    with pytest.raises(ValueError, match="only 6 distinct"):
        P.seed(y, 7, 1, rs.random_sample(7))
