"""GPU: subset scoring (acav100m_amd/csrc/acav_score.hip) at the sizes where its kernels split their work -- several
table-building workgroups per pair and the cap on them, a prefix that starts inside the id list and spans several of them,
global adds on a wide grid, the EMI's n_ij slices at their cap of 1024 -- against sklearn's scores of
tests/golden/subset_scores_large.npz (tests/golden/gen_subset_scores_large.py).  The fixture holds seeds; the inputs are
rebuilt by tests/_subset_scores_np.large_inputs (checked against the fixture without a GPU in tests/test_capi_host.py).
Every test first asserts, from acav_score_plan, the launch shapes it is about; the rules are those of
tests/test_gpu_subset_scores.py::test_golden_scores."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import _subset_scores_np as R

pytestmark = pytest.mark.gpu

LDS, SLICES, PER, NB, LPC, Z, EMI_PARTS = range(7)  # the slots of acav_score_plan
# case -> (LDS table, table-building workgroups per pair, ids of each, EMI slices) of the call on the whole list
PATHS = {"c7_n20000": (1, 3, 6667, 156), "c143_n20000": (1, 3, 6667, 28), "c300_n20000": (0, 79, 256, 13),
         "c2_n300000": (1, 37, 8109, 1024), "c2_n304097": (1, 38, 8003, 1024), "c32_p45_n400000": (1, 45, 8889, 0)}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "subset_scores_large.npz"))


_inputs = {}


def _case(golden, name):
    """(assign, C, pairs, ids, prefix, measure names) -- rebuilt once from the fixture's seeds and shared, never changed"""
    if name not in _inputs:
        assign, ids = R.large_inputs(*(int(golden[name + "." + k]) for k in ("seed", "V", "D", "C", "n", "repeats")))
        names = [m for m in R.NAMES if m != "adjusted_mutual_info" or int(golden[name + ".emi"])]
        _inputs[name] = (assign, int(golden[name + ".C"]), golden[name + ".pairs"].tolist(), ids, golden[name + ".prefix"].tolist(), names)
    return _inputs[name]


def _scorer(golden, name):
    from acav100m_amd.subset_selection import get_measure
    assign, C_, pairs, _, _, _ = _case(golden, name)
    m = get_measure("batch_mi")(assign, ncentroids=C_, device="cuda:0")
    m.init([tuple(p) for p in pairs], [])
    return m


def _plan(C_, P, n, m, want_emi):
    from acav100m_amd import _lib
    out = (C.c_int64 * 7)()
    _lib.check(_lib.load_library().acav_score_plan(C_, P, n, m, int(want_emi), out))
    return list(out)


def _assert_path(golden, name):
    """the whole list of the case takes the launch shapes the case is there for"""
    _, C_, pairs, ids, _, names = _case(golden, name)
    emi = "adjusted_mutual_info" in names
    plan = _plan(C_, len(pairs), len(ids), len(ids), emi)
    assert (plan[LDS], plan[SLICES], plan[PER], plan[Z]) == PATHS[name], (name, plan)
    assert plan[SLICES] > 1 and plan[EMI_PARTS] == (C_ * plan[Z] if emi else 0)
    return plan


def _same_bits(x, y):
    assert set(x) == set(y)
    for k in x:
        if k == "per_pair":
            for m in x[k]:
                assert np.asarray(x[k][m]).tobytes() == np.asarray(y[k][m]).tobytes(), m
        elif k == "stats":
            assert x[k].tobytes() == y[k].tobytes()
        else:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


_wanted = {}


def _check_against_golden(golden, name, out, rows=None):
    """the rules of test_golden_scores on the prefixes `rows` (default: all) of a result with per_pair and stats: integer stats
    equal the numpy restatement; adjusted_rand / fowlkes_mallows / rand equal sklearn exactly; mutual_info,
    normalized_mutual_info and the entropies within 1e-9 of sklearn (the header's reordering bound, 2^20 terms x 2^-53 x 43 <
    5e-9, covers these tables of <= 9e4 cells); adjusted_mutual_info within max(100 x the restatement's recorded distance from
    sklearn, 1e-13)"""
    assign, C_, pairs, ids, prefix, names = _case(golden, name)
    sk, dev, h = golden[name + ".sk"], golden[name + ".dev"], golden[name + ".h"]
    worst = dict.fromkeys(names, 0.0)
    for at, q in enumerate(range(len(prefix)) if rows is None else rows):
        k = prefix[q]
        for p, (d1, d2) in enumerate(pairs):
            st = np.atleast_2d(out["stats"])[at, p]
            if (name, q, p) not in _wanted:
                _wanted[name, q, p] = R.raw_stats(R.table(assign, ids[:k], d1, d2, C_), with_emi=False)
            want = _wanted[name, q, p]
            for f in ("tp", "fp", "fn", "tn", "n_rows", "n_cols", "n"):
                assert int(st[f]) == want[f], (name, k, p, f)
            assert abs(st["h_row"] - h[q, p, 0]) <= 1e-9 and abs(st["h_col"] - h[q, p, 1]) <= 1e-9
            for mname in names:
                i = R.NAMES.index(mname)
                got = float(np.atleast_2d(out["per_pair"][mname])[at, p])
                d = abs(got - sk[q, p, i])
                worst[mname] = max(worst[mname], d)
                where = "{} prefix {} pair {} {}: {!r} vs sklearn {!r}".format(name, k, p, mname, got, float(sk[q, p, i]))
                if mname in ("adjusted_rand", "fowlkes_mallows", "rand"):
                    assert got == sk[q, p, i], where
                elif mname == "adjusted_mutual_info":
                    assert d <= max(100.0 * dev[q, p, i], 1e-13), where
                else:
                    assert d <= 1e-9, where
        for mname in names:
            col = np.atleast_2d(out["per_pair"][mname])[at]
            assert float(np.atleast_1d(out[mname])[at]) == float(sum(col.tolist()) / len(pairs))
    print(name, "largest distance from sklearn:", " ".join("{}={:.2e}".format(k, v) for k, v in worst.items()),
          "| AMI restatement:", "{:.2e}".format(float(np.nan_to_num(dev[..., 2]).max())),
          "| AMI bound:", "{:.2e}".format(max(100.0 * float(np.nan_to_num(dev[..., 2]).max()), 1e-13)))
    return worst


@pytest.mark.parametrize("name", ["c7_n20000", "c143_n20000", "c300_n20000", "c2_n300000", "c32_p45_n400000"])
def test_large_golden_scores(env, golden, name):
    assign, C_, pairs, ids, prefix, names = _case(golden, name)
    plan = _assert_path(golden, name)
    if name == "c7_n20000":  # the second point of the curve: 15000 ids from 5000 on, in 2 workgroups per pair
        assert prefix == [5000, 20000]
        assert _plan(C_, 2, 5000, 5000, True)[SLICES] == 1 and _plan(C_, 2, 20000, 15000, True)[SLICES:PER + 1] == [2, 7500]
    if name == "c143_n20000":
        assert 4 * C_ * C_ == 81796  # dynamic LDS above 48 KB
    if name == "c2_n300000":
        assert plan[LPC] == 128 and len(np.unique(ids)) < len(ids)
    if name == "c32_p45_n400000":  # ceil(n / 8192) = 49 workgroups, capped to 2048 // 45
        assert len(pairs) == 45 and -(-len(ids) // 8192) == 49 and 2048 // 45 == 45 and "adjusted_mutual_info" not in names
    m = _scorer(golden, name)
    out = m.score_subset(ids, prefixes=prefix, measures=names, per_pair=True, return_stats=True)
    assert np.isnan(out["stats"]["emi"]).all() == ("adjusted_mutual_info" not in names)
    worst = _check_against_golden(golden, name, out)
    if name == "c2_n300000":  # what the floor of the AMI rule is up against: the EMI adds 6e5 terms in another order
        N = R.table(assign, ids, 0, 1, C_)
        de, bound = R.ami_reorder_bound(N, R.raw_stats(N))
        print(name, "AMI: distance from sklearn {:.2e}; reordering bound of the restatement's own terms: EMI {:.2e}, AMI {:.2e}".format(
            worst["adjusted_mutual_info"], de, bound))


def test_large_curve_point_equals_separate_calls(env, golden):
    """the table of the second point is the first point's plus 15000 ids added by 2 workgroups per pair from id 5000 on; the
    separate call builds it from nothing with 3: the same bytes"""
    name = "c7_n20000"
    _, C_, pairs, ids, prefix, _ = _case(golden, name)
    assert _plan(C_, len(pairs), 20000, 15000, True)[SLICES] == 2 and _plan(C_, len(pairs), 20000, 20000, True)[SLICES] == 3
    m = _scorer(golden, name)
    curve = m.score_subset(ids, prefixes=prefix, per_pair=True, return_stats=True)
    for q, k in enumerate(prefix):
        one = m.score_subset(ids[:k], per_pair=True, return_stats=True)
        assert one["stats"].tobytes() == curve["stats"][q].tobytes(), k
        for mname in R.NAMES:
            assert float(one[mname]) == float(curve[mname][q])
            assert one["per_pair"][mname].tobytes() == curve["per_pair"][mname][q].tobytes()
        _check_against_golden(golden, name, one, rows=[q])


@pytest.mark.parametrize("name", ["c7_n20000", "c2_n300000"])
def test_large_bits_do_not_depend_on_run_or_order(env, golden, name):
    _, _, _, ids, _, _ = _case(golden, name)
    assert _assert_path(golden, name)[SLICES] >= 3
    m = _scorer(golden, name)
    first = m.score_subset(ids, per_pair=True, return_stats=True)
    _same_bits(first, m.score_subset(ids, per_pair=True, return_stats=True))
    rs = np.random.RandomState(5)
    _same_bits(first, m.score_subset(rs.permutation(ids), per_pair=True, return_stats=True))
    _same_bits(first, m.score_subset(np.sort(ids)[::-1], per_pair=True, return_stats=True))
    assert np.isfinite(first["stats"]["emi"]).all()
    _check_against_golden(golden, name, first, rows=[len(golden[name + ".prefix"]) - 1])


def test_large_lists_on_a_handle_that_scored_a_short_one(env, golden):
    """one handle: a short list (the ln k / ln k! tables are built for V + 1 = 300001), then the 300000 ids, then 304097 ids
    of the same clips -- more than V + 1, the tables grow under a handle that has used them"""
    short, long_ = "c2_n300000", "c2_n304097"
    _assert_path(golden, short), _assert_path(golden, long_)
    assign, C_, pairs, ids, _, _ = _case(golden, short)
    assign2, _, _, ids2, _, _ = _case(golden, long_)
    assert np.array_equal(assign, assign2) and len(ids2) > assign.shape[0] + 1 >= len(ids)
    m = _scorer(golden, short)
    few = m.score_subset(ids[:50], per_pair=True, return_stats=True)
    assert int(few["stats"]["n"][0]) == 50
    _check_against_golden(golden, short, m.score_subset(ids, per_pair=True, return_stats=True))
    grown = m.score_subset(ids2, per_pair=True, return_stats=True)
    _check_against_golden(golden, long_, grown)
    _same_bits(grown, _scorer(golden, long_).score_subset(ids2, per_pair=True, return_stats=True))  # a handle that starts there
    _same_bits(few, m.score_subset(ids[:50], per_pair=True, return_stats=True))  # the grown tables hold the same values
