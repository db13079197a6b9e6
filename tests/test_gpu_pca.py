"""GPU: acav_rows_scatter / acav_rows_project (acav100m_amd/csrc/acav_pca.hip) through clustering.pca against the float64
restatement (tests/_pca_np.py): the sums within the any-order dot-product bound, the projection within the fp32 one, and the
same bits from host, device and unaligned input and from every way of cutting the rows into segments and calls."""
import ctypes as C

import numpy as np
import pytest

from tests import _pca_np as R

pytestmark = pytest.mark.gpu

U53, U24 = 2.0 ** -53, 2.0 ** -24


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import acav100m_amd
    lib = acav100m_amd.load_library()
    cus = C.c_int(0)
    assert lib.acav_device_info(0, None, 0, C.byref(cus), None) == 0
    return lib, cus.value


def _past_the_grid(gpu):
    """one slice -- and one row -- more than a round of launches holds at d = 64"""
    lib, cus = gpu
    out = (C.c_int64 * 7)()
    assert lib.acav_rows_scatter_plan(2 ** 30, 64, cus, out) == 0
    slice_rows, pairs, per_round, grid = int(out[0]), int(out[2]), int(out[3]), int(out[4])
    assert pairs == 1 and grid == per_round * pairs
    return slice_rows * (per_round + 1) + 1


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _shift_of(x):
    """any finite fp32 shift will do for the contract; the run's is the mean of the first rows"""
    return x[:100].astype(np.float64).mean(0).astype(np.float32)


def _sums(x, shift, prefix=None, into=None):
    """(sum f64 [d], scatter f64 [d, d]) as numpy after one update of fresh (or the given) accumulators"""
    from acav100m_amd.clustering import ScatterMoments
    sm = into if into is not None else ScatterMoments(x.shape[1], shift, "cuda:0")
    sm.update(x, prefix)
    return sm.sum.cpu().numpy(), sm.scatter.cpu().numpy()


# the smallest shapes at which each path can go wrong: two rows; n on either side of a stage with d below two blocks; d % 4 != 0
# (the guarded path) below one block; 36 blocks a side with one slice; a slice and a few rows with tails in both directions
SHAPES = [(2, 3), (63, 88), (257, 88), (1000, 7), (300, 2304), (1030, 1408)]


def _check_scatter(x, x_dev):
    n, d = x.shape
    shift = _shift_of(x)
    want_s, want_g, abs_g, abs_s = R.shifted_sums(x, shift)
    got_s, got_g = _sums(x_dev, shift)
    bound = 2 * (n + 2) * U53
    err_g = np.abs(got_g - want_g)
    err_s = np.abs(got_s - want_s)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("n {} d {}: scatter error / bound {:.3g}, sum error / bound {:.3g}".format(
            n, d, np.nanmax(np.where(abs_g > 0, err_g / (bound * abs_g), 0.0)), np.nanmax(np.where(abs_s > 0, err_s / (bound * abs_s), 0.0))))
    assert (err_g <= bound * abs_g).all()
    assert (err_s <= bound * abs_s).all()
    assert _same_bits(got_g, np.ascontiguousarray(got_g.T))  # symmetric to the bit
    # host pointer == device pointer == a second call
    for again in (x, x_dev):
        s2, g2 = _sums(again, shift)
        assert _same_bits(s2, got_s) and _same_bits(g2, got_g)
    return shift, got_s, got_g


@pytest.mark.parametrize("n,d", SHAPES, ids=["{}x{}".format(*s) for s in SHAPES])
def test_scatter(gpu, n, d):
    import torch
    x = R.recipe(n, d, seed=7 * n + d)
    _check_scatter(x, torch.from_numpy(x).cuda())


def test_scatter_past_the_grid(gpu):
    import torch
    n = _past_the_grid(gpu)
    x = R.recipe(n, 64, seed=5)
    _check_scatter(x, torch.from_numpy(x).cuda())


def test_scatter_unaligned_rows(gpu):
    """(1000, 8) at a 4-byte offset into a larger buffer: the guarded and the 16-byte path give the same bits"""
    import torch
    x = R.recipe(1000, 8, seed=11)
    buf = torch.zeros(1000 * 8 + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    x_dev = buf[1:].view(1000, 8)
    assert x_dev.data_ptr() % 16 == 4 and x_dev.is_contiguous()
    shift, s, g = _check_scatter(x, torch.from_numpy(x).cuda())
    s2, g2 = _sums(x_dev, shift)
    assert _same_bits(s2, s) and _same_bits(g2, g)


@pytest.mark.parametrize("n,d", [(1000, 7), (1030, 1408), (3000, 88)], ids=["1000x7", "1030x1408", "3000x88"])
def test_scatter_segments_and_calls(gpu, n, d):
    """the accumulators of the same shards, bit for bit: one call with the prefix [0, 100, 100, 613, n], the same shards as two
    and as four calls into the same accumulators, and the same segments inside a larger call started from equal accumulators"""
    import torch
    from acav100m_amd.clustering import ScatterMoments
    x = R.recipe(n, d, seed=n + 13 * d)
    xt = torch.from_numpy(x).cuda()
    shift = _shift_of(x)
    prefix = [0, 100, 100, 613, n]
    one_s, one_g = _sums(xt, shift, prefix)
    two = ScatterMoments(d, shift, "cuda:0")
    _sums(xt[:100], shift, [0, 100], into=two)
    s2, g2 = _sums(x[100:], shift, [0, 0, 513, n - 100], into=two)  # (the second call from the host)
    assert _same_bits(s2, one_s) and _same_bits(g2, one_g) and two.n == n
    four = ScatterMoments(d, shift, "cuda:0")
    for lo, hi in zip(prefix[:-1], prefix[1:]):
        s4, g4 = _sums(xt[lo:hi], shift, None, into=four)
    assert _same_bits(s4, one_s) and _same_bits(g4, one_g)
    # an empty segment changes nothing, wherever it stands
    s5, g5 = _sums(xt, shift, [0, 0, 100, 613, 613, n, n])
    assert _same_bits(s5, one_s) and _same_bits(g5, one_g)
    # inside a larger call: other rows before and after, from equal accumulators
    other = R.recipe(377, d, seed=99)
    big = torch.from_numpy(np.concatenate([other[:300], x, other[300:]])).cuda()
    a = ScatterMoments(d, shift, "cuda:0")
    sa, ga = _sums(big, shift, [0, 300] + [300 + p for p in prefix[1:]] + [300 + n + 77], into=a)
    b = ScatterMoments(d, shift, "cuda:0")
    _sums(other[:300], shift, None, into=b)
    _sums(xt, shift, prefix, into=b)
    sb, gb = _sums(other[300:], shift, None, into=b)
    assert _same_bits(sa, sb) and _same_bits(ga, gb) and a.n == b.n == n + 377
    # finish(): the mean and the centred scatter matrix of the restatement
    n_, mean, S = two.finish()
    want = R.fit(x, 1)
    assert n_ == n and np.abs(mean - want["mean64"]).max() <= 1e-12 * max(1.0, np.abs(want["mean64"]).max())
    assert np.abs(S - want["S"]).max() <= 1e-9 * np.abs(want["S"]).max()


PS = [1, 16, 37, 256]


def _comps(p, d, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(p, d) / np.sqrt(d)).astype(np.float32), rs.uniform(-5, 5, d).astype(np.float32)


def _check_project(x, x_dev, p):
    from acav100m_amd.clustering import project
    n, d = x.shape
    comps, mean = _comps(p, d, seed=p + d)
    mean[:] = mean + x[:50].astype(np.float64).mean(0).astype(np.float32)  # near the data's, like a fitted one
    keep = x.copy()
    y = project(x_dev, mean, comps)
    assert y.is_cuda and tuple(y.shape) == (n, p) and y.is_contiguous()
    got = y.cpu().numpy()
    want, mag = R.project64(x, mean, comps)
    bound = 1.01 * (d + 2) * U24 * mag + d * 2.0 ** -126
    err = np.abs(got.astype(np.float64) - want)
    print("n {} d {} p {}: error / bound {:.3g}".format(n, d, p, float((err / bound).max())))
    assert (err <= bound).all()
    assert _same_bits(x_dev.cpu().numpy(), keep)  # x is left untouched
    assert _same_bits(project(x, mean, comps).cpu().numpy(), got)  # host input == device input
    for a, b in ((0, 1), (1, min(n, 18)), (n // 3, n // 3 + min(65, n - n // 3)), (max(0, n - 5), n)):
        assert _same_bits(project(x_dev[a:b], mean, comps).cpu().numpy(), got[a:b]), (a, b)
    return mean, comps, got


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n,d", SHAPES, ids=["{}x{}".format(*s) for s in SHAPES])
def test_project(gpu, n, d, p):
    import torch
    x = R.recipe(n, d, seed=3 * n + d)
    _check_project(x, torch.from_numpy(x).cuda(), p)


def test_project_past_the_grid(gpu):
    import torch
    n = _past_the_grid(gpu)
    x = R.recipe(n, 64, seed=6)
    _check_project(x, torch.from_numpy(x).cuda(), 37)


@pytest.mark.parametrize("p", [16, 37])
def test_project_unaligned_rows(gpu, p):
    import torch
    from acav100m_amd.clustering import project
    x = R.recipe(1000, 8, seed=12)
    buf = torch.zeros(1000 * 8 + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    x_dev = buf[1:].view(1000, 8)
    assert x_dev.data_ptr() % 16 == 4
    mean, comps, got = _check_project(x, torch.from_numpy(x).cuda(), p)
    assert _same_bits(project(x_dev, mean, comps).cpu().numpy(), got)
    assert float(buf[0]) == 0.0


@pytest.mark.parametrize("n,d,p", [(257, 88, 16), (1030, 1408, 37)], ids=["257x88->16", "1030x1408->37"])
def test_fit_transform_against_the_restatement(gpu, n, d, p):
    """explained_variance_ by Weyl's inequality, the leading components by the Davis-Kahan bound, both from the scatter bound:
    dS_ij <= (2 (n + 2) + 4) 2^-53 ((|E|^T |E|)_ij + 2 a_i a_j / N), a = sum_rows |E| (the scatter sum's bound plus that of
    sum sum^T / N and the subtraction), and 16 d 2^-53 lambda_1 for the two eigh calls; |d lambda| <= ||dS||_F / (N - 1) + that,
    |d comp| <= that / gap + 2^-24 (the rounding to fp32), the gap taken from the restatement's own spectrum"""
    import torch
    from acav100m_amd.clustering import PCA, project
    x = R.recipe(n, d, seed=n + d + p)
    want = R.fit(x, p)
    pca = PCA(p)
    y = pca.fit_transform(x)
    assert isinstance(y, np.ndarray) and y.shape == (n, p) and y.dtype == np.float32
    assert pca.components_.dtype == np.float32 and pca.components_.shape == (p, d) and pca.mean_.dtype == np.float32
    _, _, abs_g, abs_s = R.shifted_sums(x, pca.shift_)
    dS = (2 * (n + 2) + 4) * U53 * (abs_g + 2 * np.outer(abs_s, abs_s) / n)
    w = want["spectrum"]
    dcov = np.sqrt((dS ** 2).sum()) / (n - 1) + 16 * d * U53 * w[0]
    dl = np.abs(pca.explained_variance_ - want["explained_variance"])
    lead = min(8, p)
    print("n {} d {} p {}: |d lambda| / bound {:.3g}, relative bound of the leading ones {:.3g}".format(
        n, d, p, float((dl / dcov).max()), float(dcov / w[lead - 1])))
    assert (dl <= dcov).all()
    assert abs(pca.total_variance_ - want["total_variance"]) <= d * dcov
    assert np.allclose(pca.explained_variance_ratio_, pca.explained_variance_ / pca.total_variance_, rtol=1e-15, atol=0)
    assert np.abs(pca.mean_.astype(np.float64) - want["mean64"]).max() <= U24 * np.abs(want["mean64"]).max() * 1.01
    for k in range(lead):
        gap = min(w[k - 1] - w[k] if k else np.inf, w[k] - w[k + 1])
        dc = np.abs(pca.components_[k].astype(np.float64) - want["components64"][k]).max()
        assert dc <= dcov / gap + U24, (k, dc, dcov / gap)
    # fit_transform is transform of the fitted rows; numpy in, numpy out; a tensor in, a device tensor out
    assert _same_bits(y, project(x, pca.mean_, pca.components_).cpu().numpy())
    xt = torch.from_numpy(x).cuda()
    pt = PCA(p)
    yt = pt.fit_transform(xt)
    assert yt.is_cuda and _same_bits(yt.cpu().numpy(), y) and _same_bits(pt.components_, pca.components_)
    with pytest.raises(ValueError, match="N <= p"):
        PCA(p).fit(x[:p])


def test_pca_features_picks_the_smallest_width(gpu):
    from acav100m_amd.clustering import PCA, pca_feature, pca_features
    feats = {"a": R.recipe(300, 20, seed=1), "b": R.recipe(300, 12, seed=2)}
    out = pca_features(feats)
    assert out["a"].shape == (300, 12) and out["b"].shape == (300, 12)
    assert _same_bits(out["a"], PCA(12).fit_transform(feats["a"])) and _same_bits(out["b"], pca_feature(feats["b"], 12))
    assert pca_features(feats, 5)["a"].shape == (300, 5)
