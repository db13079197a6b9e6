"""CPU: the device-free side of the confirmation in a second view -- pair_rows, confirm_pairs and confirm_similarity_counts of
clustering/dedup.py on hand-made pair lists (an empty list, a row all of whose pairs go, the order inside a row), check_confirm's
refusals and check_options without the keys, acav_pairs_cosine_plan on hand-computed sizes with its refusals, the restatement of
tests/_dupconfirm_np.py on a case small enough to do by hand, and the new symbols in the library and the header."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import _dupconfirm_np as F

PLAN_LEN = 6
LDS = 2 * 64 * 36 * 4  # two stages of 64 rows x (32 + 4) floats


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _list():
    """7 rows; row 2: [0, 1], row 4: [1], row 5: [0, 2, 4], row 6: [3]"""
    offsets = np.array([0, 0, 0, 2, 2, 3, 6, 7], np.int64)
    pair_j = np.array([0, 1, 1, 0, 2, 4, 3], np.int64)
    pair_cos = np.array([0.91, 0.92, 0.93, 0.94, 0.95, 0.96, 0.97])
    return offsets, pair_j, pair_cos


def test_pair_rows():
    from acav100m_amd.clustering.dedup import pair_rows
    offsets, pair_j, _cos = _list()
    later, rows, ci, cj = pair_rows(offsets, pair_j)
    assert later.tolist() == [2, 2, 4, 5, 5, 5, 6] and rows.tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert np.array_equal(rows[ci], later) and np.array_equal(rows[cj], pair_j)
    # rows that occur in no pair are left out: 10 rows, the pairs (7, 2) and (9, 7)
    offsets = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2], np.int64)
    later, rows, ci, cj = pair_rows(offsets, np.array([2, 7], np.int64))
    assert later.tolist() == [7, 9] and rows.tolist() == [2, 7, 9] and ci.tolist() == [1, 2] and cj.tolist() == [0, 1]
    assert all(a.dtype == np.int64 for a in (later, rows, ci, cj))
    later, rows, ci, cj = pair_rows(np.zeros(5, np.int64), np.empty(0, np.int64))  # an empty list
    assert len(later) == len(rows) == len(ci) == len(cj) == 0
    with pytest.raises(ValueError):
        pair_rows(offsets, np.array([2], np.int64))


def test_confirm_pairs():
    from acav100m_amd.clustering.dedup import confirm_pairs
    offsets, pair_j, pair_cos = _list()
    keep = np.array([True, False, False, True, False, True, True])  # row 4 loses its only pair, row 5 keeps 0 and 4 in that order
    off, pj, pc = confirm_pairs(offsets, pair_j, pair_cos, keep)
    assert off.tolist() == [0, 0, 0, 1, 1, 1, 3, 4] and pj.tolist() == [0, 0, 4, 3] and pc.tolist() == [0.91, 0.94, 0.96, 0.97]
    off, pj, pc = confirm_pairs(offsets, pair_j, pair_cos, np.ones(7, bool))
    assert np.array_equal(off, offsets) and np.array_equal(pj, pair_j) and np.array_equal(pc, pair_cos)
    off, pj, pc = confirm_pairs(offsets, pair_j, pair_cos, np.zeros(7, bool))
    assert not off.any() and len(off) == 8 and len(pj) == len(pc) == 0
    off, pj, pc = confirm_pairs(np.zeros(4, np.int64), np.empty(0, np.int64), np.empty(0), np.empty(0, bool))  # an empty list
    assert off.tolist() == [0, 0, 0, 0] and len(pj) == len(pc) == 0 and pj.dtype == np.int64 and pc.dtype == np.float64
    with pytest.raises(ValueError):
        confirm_pairs(offsets, pair_j, pair_cos, np.ones(6, bool))


def test_confirm_similarity_counts():
    from acav100m_amd.clustering.dedup import SIMILARITY_GRID, confirm_similarity_counts
    counts = confirm_similarity_counts(np.array([-np.inf, 0.1, 0.5, 0.75, 0.9, 0.95, 0.99, 1.0]))
    assert list(counts) == [repr(g) for g in SIMILARITY_GRID]
    assert list(counts.values()) == [6, 5, 5, 4, 4, 3, 2, 2, 1, 1]
    assert not any(confirm_similarity_counts(np.empty(0)).values())


def test_check_confirm():
    from acav100m_amd.clustering.dedup import check_confirm, check_options
    assert check_confirm({}) == (None, None) and check_confirm(None) == (None, None)
    assert check_confirm({'groups': True, 'keep': 'central'}) == (None, None)
    ok = {'groups': True, 'view': 'a/x', 'confirm_view': 'v/y', 'confirm_threshold': 0.9}
    assert check_confirm(ok) == ('v/y', 0.9)
    assert check_confirm(dict(ok, confirm_threshold=1)) == ('v/y', 1.0)
    assert check_confirm(ok, views=['a/x', 'v/y'], view='a/x') == ('v/y', 0.9)
    for drop in ('confirm_view', 'confirm_threshold'):
        with pytest.raises(ValueError, match="go together"):
            check_confirm({k: v for k, v in ok.items() if k != drop})
    for bad in (0, 0.0, -0.5, 1.5, True, '0.9', float('nan')):
        with pytest.raises(ValueError, match="confirm_threshold must be a number in"):
            check_confirm(dict(ok, confirm_threshold=bad))
    for bad in ('video', 'a/b/c', 7, ''):
        with pytest.raises(ValueError, match="<model_key>/<layer>"):
            check_confirm(dict(ok, confirm_view=bad))
    with pytest.raises(ValueError, match="is dedup.view"):
        check_confirm(dict(ok, confirm_view='a/x'))
    with pytest.raises(ValueError, match="is dedup.view"):  # dedup.view left out and resolved from the cache
        check_confirm({k: v for k, v in ok.items() if k != 'view'}, views=['v/y'], view='v/y')
    with pytest.raises(ValueError, match="not a view of the cache"):
        check_confirm(ok, views=['a/x', 'w/z'], view='a/x')
    for groups in (None, False):
        with pytest.raises(ValueError, match="needs --dedup.groups=True: the confirmed relation is a pair list"):
            check_confirm(dict(ok, groups=groups))
    with pytest.raises(ValueError, match="refused with dedup.against_path"):
        check_confirm(dict(ok, groups=None, against_path='h.pkl', against_meta_path='m'))
    # check_options refuses them before any file is read, and without the keys returns what it returned
    opts = {'threshold': 0.95, 'out_path': 'dups.csv'}
    assert check_options(dict(opts)) == (0.95, None, 'dups.csv', None)
    assert check_options(dict(opts, groups=True, view='a/x'), views=['a/x', 'v/y']) == (0.95, 'a/x', 'dups.csv', None)
    assert check_options(dict(opts, **ok), views=['a/x', 'v/y']) == (0.95, 'a/x', 'dups.csv', None)
    with pytest.raises(ValueError, match="go together"):
        check_options(dict(opts, groups=True, confirm_view='v/y'))
    with pytest.raises(ValueError, match="needs --dedup.groups=True"):
        check_options(dict(opts, confirm_view='v/y', confirm_threshold=0.9))
    with pytest.raises(ValueError, match="not a view of the cache"):
        check_options(dict(opts, **ok), views=['a/x', 'w/z'])
    with pytest.raises(ValueError, match="refused with dedup.against_path"):
        check_options(dict(opts, confirm_view='v/y', confirm_threshold=0.9, against_path='h.pkl', against_meta_path='m'))
    with pytest.raises(ValueError, match="bipartite"):  # the groups mode's own refusal comes first, as before
        check_options(dict(opts, **ok, against_path='h.pkl', against_meta_path='m'))


def _plan(lib, pairs, d=8, cus=256):
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    assert lib.acav_pairs_cosine_plan(pairs, d, cus, out) == 0
    return tuple(out)


def test_pairs_cosine_plan(lib):
    # (pairs per wave, per workgroup, workgroups, rounds, LDS, scratch): a workgroup per 64 pairs up to 8 per compute unit
    assert _plan(lib, 0) == (16, 64, 0, 0, LDS, 16)
    assert _plan(lib, 1) == (16, 64, 1, 1, LDS, 56)
    assert _plan(lib, 16) == (16, 64, 1, 1, LDS, 40 * 16 + 16)
    assert _plan(lib, 17) == (16, 64, 1, 1, LDS, 40 * 17 + 16)
    assert _plan(lib, 64) == (16, 64, 1, 1, LDS, 40 * 64 + 16)
    assert _plan(lib, 65) == (16, 64, 2, 1, LDS, 40 * 65 + 16)
    assert _plan(lib, 2 * 64 * 256 + 1)[2:4] == (2 * 256 + 1, 1)     # past 2 x 64 x cus: still one round
    assert _plan(lib, 8 * 64 * 256)[2:4] == (8 * 256, 1)             # the grid is full
    assert _plan(lib, 8 * 64 * 256 + 1)[2:4] == (8 * 256, 2)         # one pair more: a second round
    assert _plan(lib, 64 * 3 + 5, cus=1)[2:4] == (4, 1) and _plan(lib, 64 * 20 + 5, cus=2)[2:4] == (16, 2)
    assert _plan(lib, 10 ** 12, d=16384)[2:4] == (2048, 7629395)     # ceil(ceil(10^12 / 64) / 2048): the counts are 64-bit
    assert _plan(lib, 100, d=1) == _plan(lib, 100, d=16384)          # the shape does not depend on d


def test_pairs_cosine_plan_refusals(lib):
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    for args in ((-1, 8, 256, out), (10, 0, 256, out), (10, 16385, 256, out), (10, 8, 0, out), (10, 8, 256, None)):
        assert lib.acav_pairs_cosine_plan(*args) == -1, args
    assert tuple(out) == (-7,) * PLAN_LEN


def test_the_host_refusals_of_the_entry_leave_cos_untouched(lib):
    """what is refused before a device is looked for: the sizes and the NULL pointers; pairs = 0 is ACAV_OK without a device"""
    x = np.ones((4, 3), np.float32)
    pi, pj = np.array([0, 1], np.int64), np.array([2, 3], np.int64)
    cos = np.full(2, -5.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for args in ((0, None, 4, 3, p(pi), p(pj), 2, p(cos), None), (0, p(x), 4, 3, p(pi), p(pj), 2, None, None),
                 (0, p(x), 4, 3, None, p(pj), 2, p(cos), None), (0, p(x), 4, 3, p(pi), None, 2, p(cos), None),
                 (0, p(x), 0, 3, p(pi), p(pj), 2, p(cos), None), (0, p(x), 2 ** 31, 3, p(pi), p(pj), 2, p(cos), None),
                 (0, p(x), 4, 0, p(pi), p(pj), 2, p(cos), None), (0, p(x), 4, 16385, p(pi), p(pj), 2, p(cos), None),
                 (0, p(x), 4, 3, p(pi), p(pj), -1, p(cos), None)):
        assert lib.acav_pairs_cosine(*args) == -1, args
    assert lib.acav_pairs_cosine(0, p(x), 4, 3, None, None, 0, p(cos), None) == 0
    assert (cos == -5.0).all()


def test_the_restatement_by_hand():
    xa = np.array([[1, 0], [1, 0], [0, 1], [1, 0], [0, 0]], np.float32)
    xb = np.array([[1, 0], [3, 4], [1, 1], [2, 0], [1, 0]], np.float32)
    assert F.pair_cos(xb, [0, 1, 1, 4], [1, 0, 1, 0]).tolist() == [0.6, 0.6, 1.0, 1.0]
    assert abs(F.pair_cos(xb, [2], [3])[0] - np.sqrt(0.5)) < 1e-15
    assert F.pair_cos(xa, [4, 0, 4], [0, 4, 4]).tolist() == [-np.inf] * 3
    # view A joins 0, 1 and 3 (cosine 1); view B confirms (3, 0) alone at 0.9: cosB(1, 0) = cosB(3, 1) = 0.6
    off, pj, pc, cos_b, margin, margin_b = F.confirmed(xa, xb, np.zeros(5, np.int64), 0.5, 0.9)
    assert off.tolist() == [0, 0, 0, 0, 1, 1] and pj.tolist() == [0] and pc.tolist() == [1.0]
    assert cos_b.tolist() == [0.6, 1.0, 0.6] and margin == 0.5 and abs(margin_b - 0.1) < 1e-15


def test_the_new_symbols_are_in_the_library_and_the_header(lib):
    from acav100m_amd import _lib
    for name in ("acav_pairs_cosine", "acav_pairs_cosine_plan"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert "acav_pairs_cosine" in _lib._FIRST_DEVICE_CALLS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "acav_hip.h")).read()
    assert "int acav_pairs_cosine(int device, const float *x, int64_t n, int d, const int64_t *pair_i" in header
    assert "int acav_pairs_cosine_plan(int64_t pairs, int d, int cus, int64_t *out);" in header
    assert "#define ACAV_PAIRS_COSINE_PLAN_LEN 6" in header
    assert "BYTES" in header[header.index("The cosines of a LIST of pairs"):header.index("int acav_pairs_cosine(")]
