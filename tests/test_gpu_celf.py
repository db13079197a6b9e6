"""GPU: the CELF lazy greedy (celf_ratio, acav_mi_run_celf) of the exact measures against the numpy restatement
(tests/_celf_ref.py: S, LOOKUPS and the looked-up clips identical, GAIN and the queue bit for bit) and against the reference's own
runs (tests/golden/celf_*.npz, on their first `agree` picks)."""
import csv
import ctypes as C
import glob as globmod
import itertools
import os
import random

import numpy as np
import pytest

from tests import _celf_ref as CR
from tests.test_gpu_pair_measures import assign_dir  # noqa: F401  (fixture: two assignment shards on disk)

pytestmark = pytest.mark.gpu

MEASURES = ["mi", "mem_mi", "ami", "nmi", "constant", "fm", "rand", "arand"]
RATIOS = [0.3, 1.0]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


def _measure(name, a, c, pairs, cand, **kw):
    from acav100m_amd.subset_selection import get_measure
    m = get_measure(name)(a, ncentroids=c, device="cuda:0", **kw)
    m.init(pairs, [int(i) for i in cand])
    return m


def _correlated(seed, v, dd, c):
    rs = np.random.RandomState(seed)
    comp = rs.randint(0, c, size=v)
    cols = [np.where(rs.rand(v) < 0.5, comp, rs.randint(0, c, size=v)) for _ in range(dd)]
    return np.stack(cols, 1).astype(np.int64)


def _check(m, out, ref, start, cand):
    S, GAIN, _, LOOKUPS = out
    assert S == [int(s) for s in start] + ref["S"]
    assert LOOKUPS == ref["LOOKUPS"]
    assert np.array_equal(np.array(GAIN, np.float64), ref["GAIN"], equal_nan=True)
    tr = m.trace
    assert tr["greedy_picks"] == ref["greedy_picks"]
    cap = m.CELF_TRACE_CAP
    for t, (ids, vals) in enumerate(zip(ref["lookup_ids"], ref["lookup_values"])):
        n = min(len(ids), cap)
        assert tr["lookup_ids"][t][:n].tolist() == ids[:n], f"lazy pick {t}"
        assert (tr["lookup_ids"][t][n:] == -1).all()
        assert np.array_equal(tr["lookup_values"][t][:n], np.array(vals[:n], np.float64), equal_nan=True), f"lazy pick {t}"
    q = tr["queue"]
    left = {int(c): q[i] for i, c in enumerate(cand) if q[i] != -np.inf}
    assert set(left) == set(ref["queue"])
    keys = sorted(left)
    assert np.array_equal(np.array([left[k] for k in keys]), np.array([ref["queue"][k] for k in keys]), equal_nan=True)


def _golden_inputs(g):
    a, c, subset = g["assignments"].astype(np.int64), int(g["C"]), int(g["subset"])
    start = [int(i) for i in np.atleast_1d(g["start"])]
    pairs = [tuple(p) for p in g["pairs"].tolist()]
    cand = [i for i in range(a.shape[0]) if i not in set(start)]
    return a, c, start, subset, pairs, cand


def _goldens(golden_dir):
    return sorted(globmod.glob(os.path.join(golden_dir, "celf_*.npz")))


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("measure", MEASURES)
def test_restatement_on_golden_inputs(env, golden_dir, measure, ratio):
    """every exact measure on the inputs of every CELF golden: S, GAIN (bit for bit), LOOKUPS, the lookup traces and the final
    queue equal the restatement"""
    files = _goldens(golden_dir)
    assert files
    seen = set()
    for f in files:
        g = np.load(f)
        a, c, start, subset, pairs, cand = _golden_inputs(g)
        key = (a.tobytes(), c, tuple(start), subset)
        if key in seen:
            continue
        seen.add(key)
        m = _measure(measure, a, c, pairs, cand)
        out = m.run_greedy(subset, start, record_trace=True, celf_ratio=ratio)
        ref = CR.run_measure(measure, a, pairs, c, cand, start, subset, ratio, trace_cap=m.CELF_TRACE_CAP)
        _check(m, out, ref, start, cand)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("measure", ["mi", "fm"])
def test_free_running_large(env, measure, ratio):
    """V = 20 000, C = 256, D = 3, 300 picks, one measure of each family (MI closed form / pair counting)"""
    v, dd, c, subset = 20000, 3, 256, 302
    a = _correlated(41, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    order = [int(i) for i in np.random.RandomState(5).permutation(v)]
    m = _measure(measure, a, c, pairs, order[1:])
    out = m.run_greedy(subset, order[:1], record_trace=True, celf_ratio=ratio)
    ref = CR.run_measure(measure, a, pairs, c, order[1:], order[:1], subset, ratio, trace_cap=m.CELF_TRACE_CAP)
    assert len(out[0]) == subset - 1
    _check(m, out, ref, order[:1], order[1:])


def test_weighted_mi(env):
    """weight_type weights scale measure 0 in the lazy phase as in the greedy one"""
    v, dd, c, subset = 3000, 4, 24, 120
    a = _correlated(7, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    w = [0.1, 0.25, 0.5, 0.75, 1.0, 1.7]
    order = [int(i) for i in np.random.RandomState(8).permutation(v)]
    for ratio in RATIOS:
        m = _measure("mi", a, c, dict(pairing=pairs, weights=w), order[1:])
        out = m.run_greedy(subset, order[:1], record_trace=True, celf_ratio=ratio)
        ref = CR.run_measure("mi", a, pairs, c, order[1:], order[:1], subset, ratio, weights=w, trace_cap=m.CELF_TRACE_CAP)
        _check(m, out, ref, order[:1], order[1:])
        plain = CR.run_measure("mi", a, pairs, c, order[1:], order[:1], subset, ratio)
        assert not np.array_equal(plain["GAIN"], ref["GAIN"])


@pytest.mark.parametrize("measure", ["mi", "ami", "fm", "arand"])
def test_ratio_zero_is_the_exact_greedy(env, measure):
    """celf_ratio = 0 through acav_mi_run_celf: every returned array equals acav_mi_run_exact on the same handle state, and
    the measure classes return what they returned before (LOOKUPS all 0)"""
    from acav100m_amd import _lib
    v, dd, c, subset = 2000, 3, 12, 80
    a = _correlated(3, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    order = [int(i) for i in np.random.RandomState(4).permutation(v)]
    outs = []
    for entry in ("exact", "celf"):
        m = _measure(measure, a, c, pairs, order[1:])
        m.add_samples(order[:1])
        cand = np.ascontiguousarray(m.candidate_ids, np.int64)
        n = subset - 2
        S, G, K = np.empty(n + 1, np.int64), np.empty(n + 1, np.float64), np.full(n + 1, -7, np.int64)
        nsel = C.c_int64(0)
        if entry == "exact":
            _lib.check(_lib._lib.acav_mi_run_exact(m._h, _lib.ptr(cand), len(cand), 1, subset, _lib.ptr(S), _lib.ptr(G),
                                                   C.byref(nsel), None, None, None))
        else:
            _lib.check(_lib._lib.acav_mi_run_celf(m._h, _lib.ptr(cand), len(cand), 1, subset, 0.0, _lib.ptr(S), _lib.ptr(G),
                                                  _lib.ptr(K), C.byref(nsel), 0, None, None, None))
            assert (K[:n] == 1).all()
        assert nsel.value == n
        outs.append((S[:n].copy(), G[:n].copy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1], equal_nan=True)
    m0, m1 = _measure(measure, a, c, pairs, order[1:]), _measure(measure, a, c, pairs, order[1:])
    r0, r1 = m0.run_greedy(subset, order[:1]), m1.run_greedy(subset, order[:1], celf_ratio=0)
    assert r0[0] == r1[0] and r1[3] == [0] * (len(r1[0]) - 1)
    assert np.array_equal(np.array(r0[1]), np.array(r1[1]), equal_nan=True)
    r2 = _measure(measure, a, c, pairs, order[1:]).run(subset, order[:1], None, 0)
    assert r2[0] == r0[0]


def test_goldens_reference_prefix(env, golden_dir):
    """the reference's own run(..., celf_ratio): S and LOOKUPS identical on the first `agree` picks, its fp32 GAIN within the
    tolerances of the exact measures' goldens"""
    files = _goldens(golden_dir)
    assert files
    for f in files:
        g = np.load(f)
        a, c, start, subset, pairs, cand = _golden_inputs(g)
        measure, ratio, k = str(g["measure"]), float(g["celf_ratio"]), int(g["agree"])
        m = _measure(measure, a, c, pairs, cand)
        if measure not in CR.ADDS_START:
            m.add_samples(start)  # EfficientMI.run of that stage adds the start clips for every measure (efficient.py:249)
        S, GAIN, _, LOOKUPS = m.run_greedy(subset, start, celf_ratio=ratio)
        ns = len(start)
        assert S[:ns] == start and S[ns:ns + k] == g["S"][ns:ns + k].tolist(), f
        assert LOOKUPS[:k] == g["LOOKUPS"][:k].tolist(), f
        gold, got = g["GAIN"][:k], np.array(GAIN[:k])
        assert np.array_equal(np.isnan(got), np.isnan(gold))
        ok = ~np.isnan(gold)
        np.testing.assert_allclose(got[ok], gold[ok], rtol=1e-5, atol=1e-7)


def test_speculation_width_does_not_change_the_result(env, monkeypatch):
    v, dd, c, subset = 6000, 3, 32, 150
    a = _correlated(11, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    order = [int(i) for i in np.random.RandomState(12).permutation(v)]
    for measure in ("mi", "arand"):
        outs = []
        for width in (None, "1", "3", "64"):
            if width is None:
                monkeypatch.delenv("ACAV_CELF_M", raising=False)
            else:
                monkeypatch.setenv("ACAV_CELF_M", width)
            m = _measure(measure, a, c, pairs, order[1:])
            S, GAIN, _, LOOKUPS = m.run_greedy(subset, order[:1], record_trace=True, celf_ratio=0.8)
            outs.append((S, np.array(GAIN), LOOKUPS, m.trace["lookup_ids"].copy(), m.trace["queue"].copy()))
        for o in outs[1:]:
            assert o[0] == outs[0][0] and o[2] == outs[0][2]
            assert np.array_equal(o[1], outs[0][1], equal_nan=True)
            assert np.array_equal(o[3], outs[0][3]) and np.array_equal(o[4], outs[0][4], equal_nan=True)
        if measure == "mi":  # (arand's gain is NaN from a degenerate start on: every pick accepts its first lookup)
            assert max(outs[0][2]) > 1


def test_dense_and_lazy_form_of_a_pick_agree(env, monkeypatch):
    """the dense form of a pick (device-wide sort + max-scan) and the one-workgroup form are the same walk: never dense,
    the default (the one full re-scoring pick dense) and every pick dense give identical outputs, equal to the restatement"""
    v, dd, c, subset = 6000, 3, 32, 150
    a = _correlated(11, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    order = [int(i) for i in np.random.RandomState(12).permutation(v)]
    for measure, ratio in (("mi", 0.8), ("mi", 1.0), ("constant", 0.5), ("fm", 0.7), ("arand", 1.0)):
        ref = CR.run_measure(measure, a, pairs, c, order[1:], order[:1], subset, ratio)
        for mode in ("0", None, "all"):
            if mode is None:
                monkeypatch.delenv("ACAV_CELF_DENSE", raising=False)
            else:
                monkeypatch.setenv("ACAV_CELF_DENSE", mode)
            m = _measure(measure, a, c, pairs, order[1:])
            out = m.run_greedy(subset, order[:1], record_trace=True, celf_ratio=ratio)
            _check(m, out, ref, order[:1], order[1:])
    monkeypatch.delenv("ACAV_CELF_DENSE", raising=False)


@pytest.mark.parametrize("measure,ratio", [("constant", 1.0), ("constant", 0.5), ("mi", 0.5)])
def test_wide_blocks(env, measure, ratio):
    """more than 262 144 candidates: the block keys cover 512 positions each"""
    v, dd, c, subset = 300000, 2, 4, 14
    a = _correlated(21, v, dd, c)
    pairs = [(0, 1)]
    order = [int(i) for i in np.random.RandomState(22).permutation(v)]
    m = _measure(measure, a, c, pairs, order[1:])
    out = m.run_greedy(subset, order[:1], record_trace=True, celf_ratio=ratio)
    ref = CR.run_measure(measure, a, pairs, c, order[1:], order[:1], subset, ratio, trace_cap=m.CELF_TRACE_CAP)
    _check(m, out, ref, order[:1], order[1:])


def test_no_lazy_pick_leaves_an_empty_queue(env):
    v, dd, c = 300, 3, 6
    a = _correlated(1, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    m = _measure("mi", a, c, pairs, range(1, v))
    S, GAIN, _, K = m.run_greedy(4, [0], record_trace=True, celf_ratio=0.1)  # round(2 * 0.9) = 2 greedy picks
    assert K == [1, 1] and m.trace["greedy_picks"] == 2 and len(m.trace["lookup_ids"]) == 0
    assert (m.trace["queue"] == -np.inf).all()


def test_errors_are_loud(env):
    v, dd, c = 300, 3, 6
    a = _correlated(1, v, dd, c)
    pairs = list(itertools.combinations(range(dd), 2))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            _measure("mi", a, c, pairs, range(1, v)).run_greedy(40, [0], celf_ratio=bad)
    with pytest.raises(ValueError):
        _measure("mi", a, c, pairs, range(1, v)).run_greedy(40, [0], celf_ratio=0.5, forced_pos=[0] * 40)


def test_cli_run_celf(env, assign_dir):  # noqa: F811
    from acav100m_amd import shards
    from acav100m_amd.subset_selection.cli import Cli
    from acav100m_amd.subset_selection.pairing import get_cluster_pairing
    root = assign_dir
    glob = os.path.join(root, "clusters", "shard-{000000..000001}.pkl")
    out_csv = os.path.join(root, "celf", "output.csv")
    random.seed(0)
    Cli().run(shards_path=glob, meta_path=os.path.join(root, "videos"), out_path=out_csv, measure_name="fm", celf_ratio=1.0,
              **{"subset.size": 40})
    got = [r[1] for r in csv.reader(open(out_csv))]
    paths = [os.path.join(root, "clusters", "shard-%06d.pkl" % s) for s in range(2)]
    a, ctypes_, _, filenames = shards.load_assignment_shards(paths)
    random.seed(0)
    order = list(range(len(a)))
    random.shuffle(order)
    pairs = [p[:2] for p in get_cluster_pairing(ctypes_, "combination")]
    ref = CR.run_measure("fm", a, pairs, int(a.max()) + 1, order[1:], order[:1], 40, 1.0)
    assert len(got) == 39
    assert got == [filenames[s] for s in sorted(order[:1] + ref["S"])]
    with pytest.raises(ValueError):
        Cli().run(shards_path=glob, meta_path=os.path.join(root, "videos"), out_path=os.path.join(root, "celf_b", "output.csv"),
                  measure_name="batch_mi", celf_ratio=0.5, **{"subset.size": 40})
