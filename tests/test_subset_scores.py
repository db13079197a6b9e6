"""CPU-only checks of subset scoring: the two new symbols, the host-only composer acav_score_compose against sklearn's
golden scores (tests/golden/subset_scores.npz, written by tests/golden/gen_subset_scores.py), the 128-bit adjusted_rand, the
name checks and the csv -> clip mapping of the `evaluate` verb."""
import math
import os
import re

import numpy as np
import pytest

from tests import _subset_scores_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def acav():
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "subset_scores.npz"))


def _ulp_apart(x, y):
    return 0.0 if x == y else abs(x - y) / math.ulp(max(abs(x), abs(y)))


def test_new_symbols_in_header_exports_and_ctypes(acav):
    from acav100m_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acav_hip.h")).read()
    declared = set(re.findall(r"\b(acav_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load_library()
    for name in ("acav_mi_score_subset", "acav_score_compose"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    from acav100m_amd.subset_selection.measures.batch import SCORE_NAMES, SCORE_STATS_DTYPE
    assert SCORE_NAMES == R.NAMES
    for i, name in enumerate(SCORE_NAMES):  # the bit order of the header
        assert re.search(r"#define ACAV_SCORE_%s %d\b" % (name.upper(), i), hdr)
    assert SCORE_STATS_DTYPE.itemsize == 88 and SCORE_STATS_DTYPE.names[:4] == ("mi", "h_row", "h_col", "emi")


def test_compose_matches_every_golden_case(acav, golden):
    """stats recomputed in numpy -> acav_score_compose: adjusted_rand / fowlkes_mallows / rand equal sklearn's values exactly;
    mutual_info is the stat itself; normalized / adjusted_mutual_info are within 1 ulp of the same division done in Python,
    and as close to sklearn as the recorded restatement is (+ that ulp)"""
    from acav100m_amd.subset_selection.measures.batch import compose_scores
    checked = 0
    for name in golden["cases"].tolist():
        assign = golden[str(golden[name + ".assign"])].astype(np.int64)
        C, ids = int(golden[name + ".C"]), golden[name + ".ids"].astype(np.int64)
        for q, k in enumerate(golden[name + ".prefix"].tolist()):
            for p, (d1, d2) in enumerate(golden[name + ".pairs"].tolist()):
                st = R.raw_stats(R.table(assign, ids[:k], d1, d2, C))
                got, want, sk, dev = compose_scores(st), R.compose(st), golden[name + ".sk"][q, p], golden[name + ".dev"][q, p]
                for i, m in enumerate(R.NAMES):
                    where = "{} prefix {} pair {} {}".format(name, k, p, m)
                    if m in ("adjusted_rand", "fowlkes_mallows", "rand"):
                        assert got[m] == sk[i], where
                    elif m == "mutual_info":
                        assert got[m] == st["mi"], where
                        assert abs(got[m] - sk[i]) <= dev[i], where
                    else:
                        assert _ulp_apart(got[m], want[m]) <= 1, where
                        assert abs(got[m] - sk[i]) <= dev[i] + math.ulp(max(abs(sk[i]), 1e-300)), where
                checked += 1
    assert checked >= 24 * 2 + 45


def test_compose_special_cases(acav):
    from acav100m_amd.subset_selection.measures.batch import compose_scores
    base = dict(mi=0.0, h_row=0.0, h_col=0.0, emi=0.0, tp=0, fp=0, fn=0, tn=0, n_rows=1, n_cols=1, n=1)
    s = compose_scores(base)  # n = 1: C(n,2) = 0
    assert (s["adjusted_rand"], s["rand"], s["fowlkes_mallows"]) == (1.0, 1.0, 0.0)
    assert (s["normalized_mutual_info"], s["adjusted_mutual_info"], s["mutual_info"]) == (1.0, 1.0, 0.0)
    s = compose_scores(dict(base, n=4, n_rows=2, n_cols=2, h_row=0.6, h_col=0.6, emi=float("nan"), tp=1, fp=1, fn=1, tn=3))
    assert math.isnan(s["adjusted_mutual_info"]) and s["normalized_mutual_info"] == 0.0  # MI == 0 -> 0; no EMI -> NaN
    s = compose_scores(dict(base, n=4, n_rows=2, n_cols=2, mi=0.5, h_row=0.5, h_col=0.5, emi=0.5, tp=2, tn=4))
    assert s["adjusted_mutual_info"] == 1.0  # 0 / 0 guarded: numerator and denominator both moved to 2^-52
    from acav100m_amd import _lib
    with pytest.raises(ValueError):
        compose_scores(dict(base, n=0))
    with pytest.raises(ValueError):
        compose_scores(dict(base, tp=-1))
    assert _lib._lib.acav_score_compose(None, None) == -1


def test_adjusted_rand_does_not_overflow(acav):
    """n = 2^31 - 2 with TP ~ TN ~ C(n,2) / 2: the products reach 2^121; Python's big integers are the reference"""
    from acav100m_amd.subset_selection.measures.batch import compose_scores
    n = 2 ** 31 - 2
    total = n * (n - 1) // 2
    for fp, fn in ((12345678901, 98765432109), (1, 0), (total // 5, total // 7), (3, 2 ** 40 + 1)):
        tp = (total - fp - fn) // 2 + 17
        tn = total - tp - fp - fn
        assert min(tp, tn) > 2 ** 58 or fp > 2 ** 58
        st = dict(mi=0.1, h_row=1.0, h_col=1.0, emi=0.05, tp=tp, fp=fp, fn=fn, tn=tn, n_rows=5, n_cols=5, n=n)
        got = compose_scores(st)
        want = 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
        assert got["adjusted_rand"] == want
        assert got["rand"] == float(tp + tn) / float(total)
        assert got["fowlkes_mallows"] == math.sqrt(float(tp) / float(tp + fp)) * math.sqrt(float(tp) / float(tp + fn))
    # the sign of a worse-than-chance agreement survives
    st = dict(mi=0.0, h_row=1.0, h_col=1.0, emi=0.0, tp=2 ** 40, fp=2 ** 60, fn=2 ** 60, tn=2 ** 40, n_rows=2, n_cols=2, n=n)
    assert compose_scores(st)["adjusted_rand"] == R.compose(st)["adjusted_rand"] < 0


def test_names_are_checked_before_any_device_call(acav):
    from acav100m_amd import _lib
    from acav100m_amd.subset_selection import get_measure
    from acav100m_amd.subset_selection.evaluate import score_selection
    from acav100m_amd.subset_selection.measures import _REGISTRY
    from acav100m_amd.subset_selection.measures.batch import SCORE_NAMES, score_mask
    touched = _lib.device_touched()
    m = get_measure("batch_mi")(np.zeros((10, 2), np.int64), ncentroids=1, device="cuda:0")  # no init: no handle, no device
    with pytest.raises(ValueError, match="unknown subset score"):
        m.score_subset([0, 1], measures=["mutual_info", "ami"])
    with pytest.raises(ValueError, match="no subset score"):
        m.score_subset([0, 1], measures=[])
    with pytest.raises(ValueError, match="unknown subset score"):
        score_selection(np.zeros((10, 2), np.int64), [("a", "l0"), ("v", "l0")], [0, 1], measures="rand,purity")
    assert _lib.device_touched() == touched
    assert score_mask(None) == (SCORE_NAMES, 63)
    assert score_mask("rand,mutual_info") == (("mutual_info", "rand"), 0b100001)
    # scores of a selection, not measures that select: the registry does not learn them (`rand` was a selection measure before)
    assert set(SCORE_NAMES) & set(_REGISTRY) == {"rand"} and _REGISTRY["rand"].__name__ == "RandScore"
    for cls in set(_REGISTRY.values()):
        if cls.__name__ != "Contrastive":
            assert hasattr(cls, "score_subset")


def test_csv_rows_map_to_clips(tmp_path):
    from acav100m_amd.subset_selection.evaluate import map_selection, read_selection
    shard_names = ["s0", "s0", "s0", "s1", "s1"]
    filenames = ["a.mp4", "b.mp4", "c.mp4", "a.mp4", "d.mp4"]  # the same file name in two shards: two clips
    path = tmp_path / "output.csv"
    path.write_text('s1,a.mp4,vid3,"[0, 10]"\ns0,c.mp4,vid2,"[0, 10]"\ns1,a.mp4,vid3,"[0, 10]"\ns0,a.mp4,vid0,"[0, 10]"\n'
                    's0,c.mp4,vid2,"[0, 10]"\n')
    rows = read_selection(path)
    assert rows == [("s1", "a.mp4"), ("s0", "c.mp4"), ("s1", "a.mp4"), ("s0", "a.mp4"), ("s0", "c.mp4")]
    ids, repeats, unknown = map_selection(rows, shard_names, filenames)
    assert (ids, repeats, unknown) == ([3, 2, 0], 2, [])
    ids, repeats, unknown = map_selection(rows + [("s1", "zzz.mp4"), ("s2", "a.mp4")], shard_names, filenames)
    assert ids == [3, 2, 0] and unknown == [("s1", "zzz.mp4"), ("s2", "a.mp4")]


def test_evaluate_names_the_unknown_clip(tmp_path, monkeypatch):
    """the verb's error for a csv row that matches no clip -- raised after the shards are read, before any device work"""
    from acav100m_amd import _lib
    from acav100m_amd.config import Namespace
    from acav100m_amd.subset_selection import evaluate as E
    csv_path = tmp_path / "output.csv"
    csv_path.write_text("s0,a.mp4,vid0,x\ns9,ghost.mp4,vid1,x\n")
    monkeypatch.setattr("acav100m_amd.subset_selection.run.load_data", lambda *a, **k: ({0: ["p"]}, {}))
    monkeypatch.setattr(E.io, "load_assignment_shards",
                        lambda paths: (np.zeros((2, 2), np.int64), [("a", "l"), ("v", "l")], ["s0", "s0"], ["a.mp4", "b.mp4"]))
    args = Namespace(selection_path=csv_path, verbose=False, data=Namespace(path="x", meta=Namespace(path="y")),
                     computation=Namespace(random_seed=0, device="cuda"), clustering=Namespace(pairing="combination"))
    touched = _lib.device_touched()
    with pytest.raises(ValueError, match=r"shard_name='s9' filename='ghost.mp4'"):
        E.evaluate(args)
    with pytest.raises(ValueError, match="unknown subset score"):
        E.evaluate(Namespace(args, evaluate=Namespace(measures="nmi")))
    assert _lib.device_touched() == touched
