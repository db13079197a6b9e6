"""GPU: acav_rows_crossdup (clustering/dedup.py: nearest_in) against the float64 restatement of tests/_crossdup_np.py: best within
the bound the header states, partner identical -- after the restatement alone has shown that every row's partner is decided
(the gap to the runner-up exceeds four times the bound; bitwise copies of the partner among the held-out rows excepted, they
tie exactly and the lowest position wins).  Shapes past one tile, one column block, one stage of d and both tile heights, with
and without blocking; the purity the header promises (the pool in pieces, one label alone, device and unaligned input, a second
call: the same bytes); the refusals."""
import numpy as np
import pytest

from tests import _crossdup_np as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _rows(n, m, d, k, copies=30):
    """seeded randn rows and randint labels; `copies` pool rows become bitwise copies of held-out rows, with their label"""
    rs = np.random.RandomState(n + m + d)
    x, y = rs.randn(n, d).astype(np.float32), rs.randn(m, d).astype(np.float32)
    lx, ly = rs.randint(0, k, n).astype(np.int64), rs.randint(0, k, m).astype(np.int64)
    planted = rs.choice(n, copies, replace=False)
    source = rs.randint(0, m, copies)
    x[planted], lx[planted] = y[source], ly[source]
    return x, y, lx, ly, planted


def _compare(x, y, lx, ly, got, what):
    """got = (best, partner) of the kernel against the restatement; no row is left out"""
    d = x.shape[1]
    best, partner, second = R.nearest_in(x, y, lx, ly)
    b = R.bound(d)
    has = partner >= 0
    gap = (best[has] - second[has]).min() if has.any() else np.inf
    print("{}: n {} m {} d {}: {} rows with a partner, smallest gap to the runner-up {:.3g}, bound {:.3g}".format(
        what, len(x), len(y), d, int(has.sum()), gap, b))
    assert gap > 4 * b, "the restatement does not decide every partner"
    err = np.abs(got[0][has] - best[has]).max() if has.any() else 0.0
    print("{}: largest |best - restatement| {:.3g}".format(what, err))
    assert got[0].shape == best.shape and got[1].shape == partner.shape
    assert np.array_equal(np.isneginf(got[0]), ~has) and not np.isnan(got[0]).any()
    assert err <= b
    assert np.array_equal(got[1], partner)
    return best, partner


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


SHAPES = [  # (n, m, d, k)
    (600, 150, 24, 1),       # unblocked, ten 64-row tiles, three column blocks
    (2000, 700, 70, 6),      # random labels; d neither a multiple of 4 nor of 32: guarded loads, a zero-filled tail
    (300, 70, 3, 2),         # d below one MFMA step
    (40000, 3000, 8, 133),   # 128-row tiles on 256 compute units, tiles spanning several labels
    (40000, 200, 8, 1),      # 128-row tiles, unblocked
]


@pytest.mark.parametrize("n,m,d,k", SHAPES, ids=["n{}-m{}-d{}-k{}".format(*s) for s in SHAPES])
def test_best_and_partner_match_the_restatement(torch_gpu, n, m, d, k):
    from acav100m_amd.clustering.dedup import nearest_in
    x, y, lx, ly, planted = _rows(n, m, d, k)
    if k == 1:
        lx = ly = None
    got = nearest_in(x, y, lx, ly, k)
    best, _partner = _compare(x, y, lx, ly, got, "host input")
    assert (np.abs(best[planted] - 1.0) <= R.bound(d)).all()
    assert (np.abs(got[0][planted] - 1.0) <= R.bound(d)).all()  # the planted copies come out within the bound of 1
    assert _same(got, nearest_in(x, y, lx, ly, k))  # the same call, the same bytes


def test_small_hand_built_case(torch_gpu):
    from acav100m_amd.clustering.dedup import nearest_in
    rs = np.random.RandomState(11)
    d, k = 12, 5
    x, y = rs.randn(90, d).astype(np.float32), rs.randn(70, d).astype(np.float32)
    lx, ly = rs.randint(0, 4, 90).astype(np.int64), rs.randint(0, 3, 70).astype(np.int64)  # label 3: in x, absent in y; 4: in neither
    ly[[8, 20]] = 1
    y[20] = y[8]                 # two equal held-out rows: the lower one is the partner ...
    x[5], lx[5] = y[20], 1       # ... of a pool row that copies them
    x[40], lx[40] = y[8], 1      # and of a second pool row copying the same held-out row
    x[[7, 33]] = 0.0             # zero rows in x
    y[[3, 50]] = 0.0             # and in y
    got = nearest_in(x, y, lx, ly, k)
    _compare(x, y, lx, ly, got, "hand-built")
    assert got[1][5] == 8 and got[1][40] == 8 and got[0][5] == got[0][40] and abs(got[0][5] - 1.0) <= R.bound(d)
    for z in (7, 33):
        assert got[1][z] == -1 and np.isneginf(got[0][z])
    assert (got[1][lx == 3] == -1).all() and np.isneginf(got[0][lx == 3]).all() and (lx == 3).sum() > 5
    assert not np.isin(got[1], [3, 50]).any()  # a zero row of y is never a partner
    assert (ly[got[1][got[1] >= 0]] == lx[got[1] >= 0]).all()


def test_d_1_every_cosine_is_exactly_plus_or_minus_one(torch_gpu):
    """d = 1: cos = a b / sqrt(fl(a^2 b^2)) with a b and both squares exact, and sqrt(fl(t^2)) = |t| in IEEE arithmetic: every
    cosine is exactly +-1 in the kernel and in numpy alike, every row ties exactly, the lowest held-out row of its sign wins"""
    from acav100m_amd.clustering.dedup import nearest_in
    rs = np.random.RandomState(5)
    x, y = rs.randn(300, 1).astype(np.float32), rs.randn(90, 1).astype(np.float32)
    lx, ly = rs.randint(0, 3, 300).astype(np.int64), rs.randint(0, 3, 90).astype(np.int64)
    best, partner, _ = R.nearest_in(x, y, lx, ly)
    assert set(np.unique(best)) <= {-1.0, 1.0}
    got = nearest_in(x, y, lx, ly, 3)
    assert np.array_equal(got[0], best) and np.array_equal(got[1], partner)


def test_purity_pieces_one_label_device_unaligned_and_torch_labels(torch_gpu):
    torch = torch_gpu
    from acav100m_amd.clustering.dedup import nearest_in
    n, m, d, k = 2000, 700, 70, 6
    x, y, lx, ly, _ = _rows(n, m, d, k)
    want = nearest_in(x, y, lx, ly, k)
    # the pool in three pieces of unequal length, none a multiple of 64
    cuts = [0, 333, 1430, n]
    pieces = [nearest_in(x[a:b], y, lx[a:b], ly, k) for a, b in zip(cuts[:-1], cuts[1:])]
    assert _same((np.concatenate([p[0] for p in pieces]), np.concatenate([p[1] for p in pieces])), want)
    # one label's rows alone, against the held-out rows of that label alone
    for c in (0, 3, 5):
        ix, iy = np.flatnonzero(lx == c), np.flatnonzero(ly == c)
        alone = nearest_in(x[ix], y[iy], np.zeros(len(ix), np.int64), np.zeros(len(iy), np.int64), 1)
        assert alone[0].tobytes() == want[0][ix].tobytes()
        assert np.array_equal(np.where(alone[1] >= 0, iy[np.maximum(alone[1], 0)], -1), want[1][ix])
    # device inputs with torch labels; inputs off 16-byte alignment by one float
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    assert _same(nearest_in(xd, yd, torch.from_numpy(lx).cuda(), torch.from_numpy(ly), k), want)
    assert _same(nearest_in(x, yd, lx, ly, k), want)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
        off = buf[1:].view(*t.shape)
        off.copy_(t)
        assert off.data_ptr() % 16 == 4
        return off

    assert _same(nearest_in(shifted(xd), yd, lx, ly, k), want)
    assert _same(nearest_in(xd, shifted(yd), lx, ly, k), want)
    # d a multiple of 4: the vector loads when aligned, the guarded ones when not
    x4, y4 = np.ascontiguousarray(x[:, :24]), np.ascontiguousarray(y[:, :24])
    want4 = nearest_in(x4, y4, lx, ly, k)
    assert _same(nearest_in(shifted(torch.from_numpy(x4).cuda()), shifted(torch.from_numpy(y4).cuda()), lx, ly, k), want4)
    # the tile height is no part of the answer: 128-row tiles in the full call, 64-row tiles for a piece
    n, m, d, k = 40000, 3000, 8, 133
    x, y, lx, ly, _ = _rows(n, m, d, k)
    full = nearest_in(x, y, lx, ly, k)
    piece = nearest_in(x[1000:9001], y, lx[1000:9001], ly, k)
    assert piece[0].tobytes() == full[0][1000:9001].tobytes() and piece[1].tobytes() == full[1][1000:9001].tobytes()


def test_unblocked_gives_the_bytes_of_all_zero_labels(torch_gpu):
    from acav100m_amd.clustering.dedup import nearest_in
    x, y, _lx, _ly, _ = _rows(600, 150, 24, 1)
    assert _same(nearest_in(x, y), nearest_in(x, y, np.zeros(600, np.int64), np.zeros(150, np.int64), 1))


def test_refusals_leave_the_outputs_untouched(torch_gpu):
    from acav100m_amd import _lib
    from acav100m_amd.clustering.dedup import nearest_in
    lib = _lib.load_library()
    x, y, lx, ly, _ = _rows(200, 90, 8, 3, copies=4)
    best, partner = np.full(200, 7.5), np.full(200, -9, np.int64)
    ARG = dict(x=x, y=y, lx=lx, ly=ly)

    def call(n=200, m=90, d=8, k=3, **kw):
        a = {name: _lib.ptr(kw.get(name, v)) if kw.get(name, v) is not None else None for name, v in ARG.items()}
        return lib.acav_rows_crossdup(0, a['x'], n, a['y'], m, d, a['lx'], a['ly'], k,
                                      _lib.ptr(best) if kw.get('bp', True) else None, _lib.ptr(partner) if kw.get('pp', True) else None, None)

    bad = lx.copy()
    bad[[3, 150]] = [3, -1]
    assert call(lx=bad) == -1 and "2 of the 200 labels of x" in lib.acav_last_error().decode()
    bad = ly.copy()
    bad[[0, 1, 89]] = [3, -5, 2 ** 40]
    assert call(ly=bad) == -1 and "3 of the 90 labels of y" in lib.acav_last_error().decode()
    bad = x.copy()
    bad[7, 2], bad[9, 0], bad[199, 7] = np.nan, np.inf, -np.inf
    assert call(x=bad) == -1
    assert "3 of the 200 x 8 values of x" in lib.acav_last_error().decode() and "not finite" in lib.acav_last_error().decode()
    bad = y.copy()
    bad[89, 7], bad[0, 0] = np.nan, np.inf
    assert call(y=bad) == -1
    assert "2 of the 90 x 8 values of y" in lib.acav_last_error().decode() and "not finite" in lib.acav_last_error().decode()
    for kw in (dict(n=0), dict(n=2 ** 31), dict(m=0), dict(m=2 ** 31), dict(d=0), dict(d=16385), dict(k=0), dict(x=None),
               dict(y=None), dict(bp=False), dict(pp=False), dict(lx=None), dict(ly=None), dict(lx=None, ly=None),
               dict(lx=None, ly=None, k=2)):
        assert call(**kw) == -1, kw
    assert (best == 7.5).all() and (partner == -9).all()
    with pytest.raises(ValueError, match="labels of y are outside"):
        nearest_in(x, y, lx, np.full(90, 3, np.int64), 3)
    with pytest.raises(ValueError, match="go together"):
        nearest_in(x, y, lx, None, 3)
    with pytest.raises(ValueError):
        nearest_in(x, y[:, :7])
    assert call() == 0 and not (best == 7.5).any() and (partner >= 0).all()
    assert call(lx=None, ly=None, k=1) == 0
