"""GPU: acav_rows_probedup (clustering/dedup.py: nearest_earlier / nearest_in with probes) against the float64 restatement of
tests/_probedup_np.py: best and best_each within the bound the header states, partner identical -- after the restatement alone
has shown every partner decided (the gap to the runner-up exceeds four times the bound; bitwise copies of the partner excepted,
they tie exactly and the lowest position wins).  Planted near-duplicates that a cluster border splits: missed without probes,
found with two.  One probe gives the bytes of acav_rows_neardup / acav_rows_crossdup; the purity the header promises; the
refusals."""
import numpy as np
import pytest

from tests import _probedup_np as R

pytestmark = pytest.mark.gpu

SHAPES = [(600, 24, 7, 3), (2000, 70, 12, 4), (300, 3, 5, 2), (40000, 8, 133, 4)]  # (n, d, K, m)
PLANTED = 6
SEED = 1  # at d = 3 the six smallest margins of 150 rows are not small under every seed: under this one every planted pair is the
#           near-duplicate the planted test states (cosine >= 0.996), at every shape
_cache = {}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def planted_case(n, d, K, m):
    """(rows, centres, labels, probes, planted [(source, copy)]): randn rows, centres = K of the rows + 0.25 randn, and PLANTED
    rows of the second half overwritten with near-copies of the rows of the first half that lie nearest a bisector, pushed
    across it: with a, b the two nearest centres of the source s, x_t = x_s + tau (c_b - c_a), tau = margin / ||c_b - c_a||^2
    -- D_b - D_a changes its sign and keeps its size.  Labels and probes are the restatement's, of the final rows."""
    if (n, d, K, m) not in _cache:
        rs = np.random.RandomState(SEED + n + d + K)
        x = rs.randn(n, d).astype(np.float32)
        centres = (x[rs.choice(n, K, replace=False)] + 0.25 * rs.randn(K, d)).astype(np.float32)
        D = R.distances(x[:n // 2], centres)
        order = np.argsort(D, axis=1, kind='stable')
        rows = np.arange(n // 2)
        margin = D[rows, order[:, 1]] - D[rows, order[:, 0]]
        sources = np.argsort(margin, kind='stable')[:PLANTED]
        targets = n // 2 + 7 * np.arange(PLANTED) + 3
        for s, t in zip(sources, targets):
            step = centres[order[s, 1]].astype(np.float64) - centres[order[s, 0]].astype(np.float64)
            x[t] = (x[s].astype(np.float64) + margin[s] / (step @ step) * step).astype(np.float32)
        labels = R.distances(x, centres).argmin(1).astype(np.int64)
        probes = R.probe_centers(x, centres, labels, m)[0]
        _cache[(n, d, K, m)] = (x, centres, labels, probes, list(zip(sources.tolist(), targets.tolist())))
    return _cache[(n, d, K, m)]


def _compare(x, y, probes, ly, before, got, what):
    """got = (best, partner, best_each) of the kernel against the restatement; no row is left out"""
    d = x.shape[1]
    best, partner, second, each = R.nearest(x, y, probes, ly, before)
    b = R.bound(d)
    has = partner >= 0
    gap = (best[has] - second[has]).min() if has.any() else np.inf
    print("{}: n {} my {} d {} m {}: {} rows with a partner, smallest gap to the runner-up {:.3g}, bound {:.3g}".format(
        what, len(x), len(y), d, probes.shape[1], int(has.sum()), gap, b))
    assert gap > 4 * b, "the restatement does not decide every partner"
    assert got[0].shape == best.shape and got[1].shape == partner.shape and got[2].shape == each.shape
    assert np.array_equal(np.isneginf(got[0]), ~has) and not np.isnan(got[0]).any()
    fin = np.isfinite(each)
    assert np.array_equal(np.isneginf(got[2]), ~fin) and not np.isnan(got[2]).any()
    err = np.abs(got[0][has] - best[has]).max() if has.any() else 0.0
    err_each = np.abs(got[2][fin] - each[fin]).max() if fin.any() else 0.0
    print("{}: largest |best - restatement| {:.3g}, |best_each - restatement| {:.3g}".format(what, err, err_each))
    assert err <= b and err_each <= b
    assert np.array_equal(got[1], partner)
    assert np.array_equal(got[0], got[2].max(1))  # best is the largest of best_each, the very value
    return best, partner


def _same(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("n,d,K,m", SHAPES, ids=["n{}-d{}-K{}-m{}".format(*s) for s in SHAPES])
def test_in_set_best_partner_and_best_each_match_the_restatement(torch_gpu, n, d, K, m):
    from acav100m_amd.clustering.dedup import nearest_earlier
    x, _centres, labels, probes, _planted = planted_case(n, d, K, m)
    got = nearest_earlier(x, labels, K, probes=probes, each=True)
    _compare(x, x, probes, labels, np.arange(n), got, "in-set")
    assert _same(got, nearest_earlier(x, labels, K, probes=probes, each=True))  # the same call, the same bytes
    assert _same(got[:2], nearest_earlier(x, labels, K, probes=probes))


@pytest.mark.parametrize("n,d,K,m", SHAPES, ids=["n{}-d{}-K{}-m{}".format(*s) for s in SHAPES])
def test_a_split_pair_is_missed_without_probes_and_found_with_two(torch_gpu, n, d, K, m):
    from acav100m_amd.clustering.dedup import nearest_earlier
    x, _centres, labels, probes, planted = planted_case(n, d, K, m)
    x64 = x.astype(np.float64)
    for s, t in planted:
        cos = (x64[s] @ x64[t]) / np.sqrt((x64[s] @ x64[s]) * (x64[t] @ x64[t]))
        print("planted {} -> {}: labels {} and {}, cosine {:.6f}".format(s, t, labels[s], labels[t], cos))
        assert labels[s] != labels[t] and probes[t, 1] == labels[s] and s < t  # the split itself
        assert cos >= (0.9998 if d >= 8 else 0.996)
    copies, sources = np.array([t for _, t in planted]), np.array([s for s, _ in planted])
    plain = nearest_earlier(x, labels, K)
    assert not (plain[1][copies] == sources).any()       # the in-cluster sweep does not see across the border
    two = nearest_earlier(x, labels, K, probes=probes[:, :2], each=True)
    assert (two[1][copies] == sources).all()             # two probes do
    assert (two[0][copies] >= (0.9998 if d >= 8 else 0.996) - R.bound(d)).all()
    assert (two[2][copies, 1] == two[0][copies]).all() and (two[2][copies, 0] < two[0][copies]).all()
    assert two[2][:, 0].tobytes() == plain[0].tobytes()  # slot 0 is the in-cluster answer


def test_one_probe_gives_the_bytes_of_neardup_and_of_crossdup(torch_gpu):
    from acav100m_amd.clustering.dedup import nearest_earlier, nearest_in
    for n, d, K, m in SHAPES:
        x, _centres, labels, _probes, _planted = planted_case(n, d, K, m)
        got = nearest_earlier(x, labels, K, probes=labels[:, None], each=True)
        assert _same(got[:2], nearest_earlier(x, labels, K)) and got[2][:, 0].tobytes() == got[0].tobytes()
        cut = n // 3
        got = nearest_in(x[cut:], x[:cut], labels[cut:], labels[:cut], K, probes_x=labels[cut:, None])
        assert _same(got, nearest_in(x[cut:], x[:cut], labels[cut:], labels[:cut], K))


def test_against_a_held_out_set_and_the_pool_in_pieces(torch_gpu):
    from acav100m_amd.clustering.dedup import nearest_in
    n, d, K, m = 2000, 70, 12, 4
    x, _centres, labels, probes, _planted = planted_case(n, d, K, m)
    cut = 700
    pool, held, lp, lh, pr = x[cut:], x[:cut], labels[cut:], labels[:cut], probes[cut:]
    want = nearest_in(pool, held, lp, lh, K, probes_x=pr, each=True)
    _compare(pool, held, pr, lh, None, want, "against")
    cuts = [0, 333, 930, len(pool)]  # three pieces of unequal length, none a multiple of 64
    pieces = [nearest_in(pool[a:b], held, lp[a:b], lh, K, probes_x=pr[a:b], each=True) for a, b in zip(cuts[:-1], cuts[1:])]
    assert _same([np.concatenate([p[i] for p in pieces]) for i in range(3)], want)
    # the tile height is no part of the answer: 128-row tiles in the full call, 64-row tiles for a piece
    n, d, K, m = 40000, 8, 133, 4
    x, _centres, labels, probes, _planted = planted_case(n, d, K, m)
    full = nearest_in(x[3000:], x[:3000], None, labels[:3000], K, probes_x=probes[3000:], each=True)
    piece = nearest_in(x[4000:9001], x[:3000], None, labels[:3000], K, probes_x=probes[4000:9001], each=True)
    assert _same(piece, [a[1000:6001] for a in full])


def test_hand_built_ties_zero_rows_missing_slots_and_empty_clusters(torch_gpu):
    from acav100m_amd.clustering.dedup import nearest_earlier, nearest_in
    rs = np.random.RandomState(11)
    n, d, K = 200, 12, 6
    x = rs.randn(n, d).astype(np.float32)
    labels = rs.randint(0, 4, n).astype(np.int64)      # the clusters 4 and 5 hold no row
    probes = np.stack([labels, (labels + 1) % 4, (labels + 2) % 4], 1)
    labels[[10, 30]] = [1, 2]
    x[30] = x[10]                                      # bitwise copies in two clusters ...
    x[150], labels[150] = x[10], 3
    probes[[10, 30, 150]] = [[1, 2, 3], [2, 3, 0], [3, 2, 1]]  # ... both probed by row 150: the lower position wins
    x[[7, 90]] = 0.0                                   # zero rows: no partner, and never one
    probes[20, 1] = -1                                 # a missing slot
    probes[21, 2] = probes[21, 0]                      # a repeated label counts once, at its first slot
    probes[22, 1], probes[23] = 5, [labels[23], 4, 5]  # probed clusters without rows
    probes[24] = -1                                    # a row without probes
    got = nearest_earlier(x, labels, K, probes=probes, each=True)
    _compare(x, x, probes, labels, np.arange(n), got, "hand-built")
    assert got[1][150] == 10 and got[2][150, 1] == got[2][150, 2] == got[0][150] and abs(got[0][150] - 1.0) <= R.bound(d)
    assert got[1][30] != 10                            # row 30 does not probe cluster 1
    for z in (7, 90, 24):
        assert got[1][z] == -1 and np.isneginf(got[0][z]) and np.isneginf(got[2][z]).all()
    assert not np.isin(got[1], [7, 90]).any()
    assert np.isneginf(got[2][20, 1]) and np.isneginf(got[2][21, 2]) and np.isneginf(got[2][22, 1]) and np.isneginf(got[2][23, 1:]).all()
    assert np.isfinite(got[2][21, 0]) and np.isfinite(got[2][23, 0])
    # the same lists against a held-out set: every row of the clusters, whatever its position
    y, ly = x[:120], labels[:120]
    got = nearest_in(x, y, None, ly, K, probes_x=probes, each=True)
    _compare(x, y, probes, ly, None, got, "hand-built, against")
    assert got[1][150] == 10 and got[1][10] == 10 and got[1][30] == 30


def test_purity_device_unaligned_input_and_torch_lists(torch_gpu):
    torch = torch_gpu
    from acav100m_amd.clustering.dedup import nearest_earlier, nearest_in
    n, d, K, m = 2000, 70, 12, 4
    x, _centres, labels, probes, _planted = planted_case(n, d, K, m)
    want = nearest_earlier(x, labels, K, probes=probes, each=True)
    xd = torch.from_numpy(x).cuda()
    assert _same(nearest_earlier(xd, torch.from_numpy(labels).cuda(), K, probes=torch.from_numpy(probes).cuda(), each=True), want)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
        off = buf[1:].view(*t.shape)
        off.copy_(t)
        assert off.data_ptr() % 16 == 4
        return off

    assert _same(nearest_earlier(shifted(xd), labels, K, probes=probes, each=True), want)
    # d a multiple of 4: the vector loads when aligned, the guarded ones when not
    x4 = np.ascontiguousarray(x[:, :24])
    want4 = nearest_earlier(x4, labels, K, probes=probes, each=True)
    assert _same(nearest_earlier(shifted(torch.from_numpy(x4).cuda()), labels, K, probes=probes, each=True), want4)
    held = torch.from_numpy(x4[:700]).cuda()
    want4 = nearest_in(x4[700:], x4[:700], None, labels[:700], K, probes_x=probes[700:], each=True)
    assert _same(nearest_in(torch.from_numpy(x4[700:]).cuda(), shifted(held), None, labels[:700], K, probes_x=probes[700:], each=True), want4)
    # a row's answer does not depend on the other queries: a third of the rows alone, cut at their own positions
    from acav100m_amd import _lib
    lib = _lib.load_library()
    some = np.arange(5, n, 3)
    best, partner, each = np.empty(len(some)), np.empty(len(some), np.int64), np.empty((len(some), m))
    pr, before = np.ascontiguousarray(probes[some]), some.astype(np.int64)
    xs = np.ascontiguousarray(x[some])
    assert lib.acav_rows_probedup(0, _lib.ptr(xs), len(some), _lib.ptr(x), n, d, _lib.ptr(pr), m, _lib.ptr(labels), _lib.ptr(before), K,
                                  _lib.ptr(best), _lib.ptr(partner), _lib.ptr(each), None) == 0
    assert _same((best, partner, each), [a[some] for a in want])


def test_refusals_leave_the_outputs_untouched(torch_gpu):
    from acav100m_amd import _lib
    from acav100m_amd.clustering.dedup import nearest_earlier, nearest_in
    lib = _lib.load_library()
    n, my, d, K, m = 200, 90, 8, 3, 2
    rs = np.random.RandomState(3)
    x, y = rs.randn(n, d).astype(np.float32), rs.randn(my, d).astype(np.float32)
    ly = rs.randint(0, K, my).astype(np.int64)
    pr = np.stack([rs.randint(0, K, n), rs.randint(-1, K, n)], 1).astype(np.int64)
    bf = np.arange(n, dtype=np.int64)
    best, partner, each = np.full(n, 7.5), np.full(n, -9, np.int64), np.full((n, m), 2.5)
    ARG = dict(x=x, y=y, pr=pr, ly=ly, bf=bf, best=best, partner=partner, each=each)

    def call(n=n, my=my, d=d, k=K, m=m, **kw):
        a = {name: _lib.ptr(kw.get(name, v)) for name, v in ARG.items()}
        return lib.acav_rows_probedup(0, a['x'], n, a['y'], my, d, a['pr'], m, a['ly'], a['bf'], k, a['best'], a['partner'], a['each'], None)

    bad = pr.copy()
    bad[[3, 150], [0, 1]] = [K, -2]
    assert call(pr=bad) == -1 and "2 of the 200 x 2 probes" in lib.acav_last_error().decode()
    bad = ly.copy()
    bad[[0, 1, 89]] = [K, -5, 2 ** 40]
    assert call(ly=bad) == -1 and "3 of the 90 labels of y" in lib.acav_last_error().decode()
    bad = x.copy()
    bad[7, 2], bad[9, 0], bad[199, 7] = np.nan, np.inf, -np.inf
    assert call(x=bad) == -1 and "3 of the 200 x 8 values of x" in lib.acav_last_error().decode()
    bad = y.copy()
    bad[89, 7], bad[0, 0] = np.nan, np.inf
    assert call(y=bad) == -1 and "2 of the 90 x 8 values of y" in lib.acav_last_error().decode()
    for kw in (dict(n=0), dict(n=2 ** 31), dict(my=0), dict(my=2 ** 31), dict(d=0), dict(d=16385), dict(k=0), dict(m=0), dict(m=17),
               dict(n=2 ** 30, m=2), dict(x=None), dict(y=None), dict(pr=None), dict(ly=None), dict(best=None), dict(partner=None)):
        assert call(**kw) == -1, kw
    assert (best == 7.5).all() and (partner == -9).all() and (each == 2.5).all()
    with pytest.raises(ValueError, match="probes of x are outside"):
        nearest_in(x, y, None, ly, K, probes_x=np.full((n, 2), K, np.int64))
    with pytest.raises(ValueError, match="need labels_y"):
        nearest_in(x, y, probes_x=pr)
    with pytest.raises(ValueError, match="probe lists"):
        nearest_earlier(x, np.zeros(n, np.int64), K, probes=pr[:50])
    with pytest.raises(ValueError, match="each=True needs"):
        nearest_earlier(x, np.zeros(n, np.int64), K, each=True)
    assert call() == 0 and not (best == 7.5).any() and not (each == 2.5).any()
    assert call(bf=None, each=None) == 0
