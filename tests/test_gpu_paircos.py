"""GPU: acav_pairs_cosine (clustering/dedup.py: pair_cosines).  Bit for bit the pair_cos of acav_rows_neardup_pairs for the pairs
that entry lists -- the test that pins the chain; against the float64 restatement of tests/_dupconfirm_np.py within the header's
bound for random pairs (i == j, across clusters, repeated rows) over widths below one MFMA step, with tails, past one stage and
pair counts around a wave, a workgroup and one round of the grid; zero rows; purity (a permutation, i and j swapped, a pair alone
and among 1000 others); host, device and unaligned input; both ways the norms are laid out; the refusals with cos untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _dupconfirm_np as F
from tests import _neardup_np as R

pytestmark = pytest.mark.gpu


def _rows(seed, n, d, k, copies=0, interleaved=False):
    """tests/test_gpu_dupgroups.py's generator: its shapes are the ones the bit-for-bit test is stated on"""
    rs = np.random.RandomState(seed)
    x = rs.randn(n, d).astype(np.float32)
    lab = (np.arange(n) % k if interleaved else rs.randint(0, k, n)).astype(np.int64)
    for _ in range(copies):  # a later row becomes a bitwise copy of an earlier one, in its cluster
        s, t = np.sort(rs.choice(n, 2, replace=False))
        x[t], lab[t] = x[s], lab[s]
    return x, lab


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


SHAPES = [(600, 24, 4, True, 12, 0.5), (2000, 70, 6, False, 20, 0.3), (300, 3, 2, False, 4, 0.5)]  # test_gpu_dupgroups.py's first three


@pytest.mark.parametrize("shape", SHAPES, ids=["n{}-d{}-k{}-t{}".format(s[0], s[1], s[2], s[5]) for s in SHAPES])
def test_bit_for_bit_the_pair_cos_of_the_pairs_entry(torch_gpu, shape):
    from acav100m_amd.clustering.dedup import pair_cosines, pair_rows, pairs_earlier
    n, d, k, inter, copies, t = shape
    x, lab = _rows(n + d, n, d, k, copies, inter)
    _best, _partner, offsets, pair_j, pair_cos = pairs_earlier(x, lab, t, k)
    later, rows, ci, cj = pair_rows(offsets, pair_j)
    assert len(pair_j) > 200
    got = pair_cosines(x, later, pair_j)
    assert got.tobytes() == pair_cos.tobytes()
    assert pair_cosines(x, pair_j, later).tobytes() == pair_cos.tobytes()  # i and j swapped
    # the verb's use: only the rows that occur in a pair, re-indexed (the norms by row: R <= 2 P)
    assert pair_cosines(np.ascontiguousarray(x[rows]), ci, cj).tobytes() == pair_cos.tobytes()
    # few pairs of many rows (the norms by pair end: n > 2 P)
    few = np.arange(0, len(pair_j), max(1, len(pair_j) // 40))[:40]
    assert 2 * len(few) < n and pair_cosines(x, later[few], pair_j[few]).tobytes() == pair_cos[few].tobytes()


@functools.lru_cache(maxsize=None)
def _random(d, pairs, n=257):
    """n rows of width d and `pairs` random pairs: every eighth pair i == j, every fifth the pair before it again, the rest any
    two rows; the restated cosines, computed once (never written to)"""
    rs = np.random.RandomState(1000 * d + pairs)
    x = rs.randn(n, d).astype(np.float32)
    pi, pj = rs.randint(0, n, pairs).astype(np.int64), rs.randint(0, n, pairs).astype(np.int64)
    pj[::8] = pi[::8]
    pi[5::5], pj[5::5] = pi[4:-1:5], pj[4:-1:5]
    ref = F.pair_cos(x, pi, pj)
    for a in (x, pi, pj, ref):
        a.setflags(write=False)
    return x, pi, pj, ref


@pytest.mark.parametrize("d", [1, 3, 4, 33, 70, 100])
@pytest.mark.parametrize("pairs", [1, 15, 16, 17, 64 * 3 + 5])
def test_random_pairs_against_the_restatement(torch_gpu, d, pairs):
    from acav100m_amd.clustering.dedup import pair_cosines
    x, pi, pj, ref = _random(d, pairs)
    got = pair_cosines(x, pi, pj)
    err = np.abs(got - ref).max()
    print("d {} pairs {}: largest |cos - restatement| {:.3g}, bound {:.3g}".format(d, pairs, err, R.bound(d)))
    assert err <= R.bound(d)
    same = pi == pj
    assert (np.abs(got[same] - 1.0) <= R.bound(d)).all()


def test_past_one_round_of_the_grid(torch_gpu):
    """d = 8 and 64 x (the workgroups of a full grid) + 7 pairs: every workgroup makes a second round or breaks off, the last
    round is partial"""
    from acav100m_amd import _lib
    from acav100m_amd.clustering.dedup import pair_cosines
    cus = torch_gpu.cuda.get_device_properties(0).multi_processor_count
    out = (C.c_int64 * 6)()
    _lib.check(_lib.load_library().acav_pairs_cosine_plan(10 ** 9, 8, cus, out))
    wgs = int(out[2])
    pairs = 64 * wgs + 7
    _lib.check(_lib.load_library().acav_pairs_cosine_plan(pairs, 8, cus, out))
    assert (int(out[2]), int(out[3])) == (wgs, 2)
    x, pi, pj, ref = _random(8, pairs, n=5000)
    got = pair_cosines(x, pi, pj)
    err = np.abs(got - ref).max()
    print("{} workgroups, {} pairs: largest |cos - restatement| {:.3g}, bound {:.3g}".format(wgs, pairs, err, R.bound(8)))
    assert err <= R.bound(8)


def test_zero_rows_and_bitwise_equal_rows(torch_gpu):
    from acav100m_amd.clustering.dedup import pair_cosines
    rs = np.random.RandomState(3)
    x = rs.randn(40, 37).astype(np.float32)
    x[5] = 0.0
    x[9] = x[2]
    pi = np.array([5, 1, 5, 9, 2, 7, 9], np.int64)
    pj = np.array([1, 5, 5, 2, 9, 7, 9], np.int64)
    got = pair_cosines(x, pi, pj)
    assert (got[:3] == -np.inf).all()
    assert (np.abs(got[3:] - 1.0) <= R.bound(37)).all() and got[3].tobytes() == got[4].tobytes()


def test_purity(torch_gpu):
    from acav100m_amd.clustering.dedup import pair_cosines
    x, pi, pj, _ref = _random(70, 1000)
    got = pair_cosines(x, pi, pj)
    assert pair_cosines(x, pi, pj).tobytes() == got.tobytes()  # the same call, the same bytes
    perm = np.random.RandomState(0).permutation(len(pi))
    assert pair_cosines(x, pi[perm], pj[perm]).tobytes() == got[perm].tobytes()
    assert pair_cosines(x, pj, pi).tobytes() == got.tobytes()
    for e in (0, 17, 63, 64, 999):  # alone in a call: another slot of another wave, the norms by pair end
        assert pair_cosines(x, pi[e:e + 1], pj[e:e + 1]).tobytes() == got[e:e + 1].tobytes()


@pytest.mark.parametrize("d", [24, 70])
def test_host_device_and_unaligned_input(torch_gpu, d):
    from acav100m_amd.clustering.dedup import pair_cosines
    torch = torch_gpu
    x, pi, pj, _ref = _random(d, 64 * 3 + 5)
    got = pair_cosines(x, pi, pj)
    xd, pid, pjd = torch.from_numpy(x).cuda(), torch.from_numpy(pi).cuda(), torch.from_numpy(pj).cuda()
    assert pair_cosines(xd, pid, pjd).tobytes() == got.tobytes()
    assert pair_cosines(xd, pi, pjd).tobytes() == got.tobytes()
    flat = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = xd.reshape(-1)
    off = flat[1:].view(x.shape)  # one float past a 16-byte boundary: the guarded loads
    assert off.data_ptr() % 16 == 4
    assert pair_cosines(off, pid, pjd).tobytes() == got.tobytes()
    # cos on the device
    from acav100m_amd import _lib
    cos = torch.full((len(pi),), -5.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load_library().acav_pairs_cosine(0, _lib.ptr(xd), x.shape[0], d, _lib.ptr(pid), _lib.ptr(pjd), len(pi), _lib.ptr(cos), None))
    assert cos.cpu().numpy().tobytes() == got.tobytes()


def test_duplicate_groups_of_a_kmeans_state_with_a_confirming_view(torch_gpu):
    """KMeans.duplicate_groups(confirm=, confirm_threshold=): the groups of the restated filter.  View B copies view A's planted
    copies for every second pair only, so the confirmation splits groups"""
    from acav100m_amd.clustering import KMeans
    from tests import _dupgroups_np as G
    n, d, k, inter, copies, _t = SHAPES[0]
    xa, _lab = _rows(n + d, n, d, k, copies, inter)
    t, t2 = 0.999999, 0.9  # the bitwise copies alone
    centres = np.random.RandomState(4).randn(k, d).astype(np.float32)
    km = KMeans(None, d, k).to_lloyd(centres).to("cuda:0")
    labels, _ = km.calc_best(xa, need_mean=False)
    labels = labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)
    offsets_a, pair_j_a, _cos, margin = G.pairs(xa, labels, t)
    later = np.repeat(np.arange(n), np.diff(offsets_a))
    xb = np.random.RandomState(5).randn(n, 33).astype(np.float32)
    xb[later[::2]] = xb[pair_j_a[::2]]
    offsets, pair_j, _pc, cos_b, _margin, margin_b = F.confirmed(xa, xb, labels, t, t2)
    assert margin > 4 * R.bound(d) and margin_b > 4 * R.bound(33) and 0 < offsets[-1] < offsets_a[-1]
    want, want_a = G.components(n, offsets, pair_j), G.components(n, offsets_a, pair_j_a)
    assert not np.array_equal(want, want_a)
    root, kept = km.duplicate_groups(xa, t, confirm=xb, confirm_threshold=t2)
    assert np.array_equal(root, want) and np.array_equal(kept, want == np.arange(n))
    root, _kept = km.duplicate_groups(xa, t, labels=labels, confirm=torch_gpu.from_numpy(xb).cuda(), confirm_threshold=t2)
    assert np.array_equal(root, want)
    assert np.array_equal(km.duplicate_groups(xa, t)[0], want_a)  # without the two arguments: what it did
    for bad in (dict(confirm=xb), dict(confirm_threshold=t2), dict(confirm=xb, confirm_threshold=0.0), dict(confirm=xb[:-1], confirm_threshold=t2)):
        with pytest.raises(ValueError, match="confirm"):
            km.duplicate_groups(xa, t, **bad)


def test_refusals_leave_cos_untouched(torch_gpu):
    from acav100m_amd import _lib
    lib = _lib.load_library()
    x, pi, pj, _ref = _random(33, 17)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n, d, pairs = x.shape[0], x.shape[1], len(pi)
    cos = np.full(pairs, -5.0)

    def call(xx=x, ii=pi, jj=pj, nn=n, dd=d, pp=pairs):
        return lib.acav_pairs_cosine(0, p(xx), nn, dd, p(ii), p(jj), pp, p(cos), None)

    for where in (0, 16):
        for value in (n, -1):
            bad = pi.copy()
            bad[where] = value
            assert call(ii=bad) == -1 and "outside [0, {})".format(n) in lib.acav_last_error().decode()
            assert call(jj=bad) == -1
    for value in (np.nan, np.inf, -np.inf):
        bad = x.copy()
        bad[200, 32] = value  # a row no pair has to name
        assert call(xx=bad) == -1 and "1 of the" in lib.acav_last_error().decode() and "not finite" in lib.acav_last_error().decode()
    assert call(dd=0) == -1 and call(pp=-1) == -1 and call(nn=0) == -1
    assert (cos == -5.0).all()
    assert lib.acav_pairs_cosine(0, p(x), n, d, None, None, 0, p(cos), None) == 0 and (cos == -5.0).all()  # pairs = 0: OK
    assert call() == 0 and np.isfinite(cos).all()
