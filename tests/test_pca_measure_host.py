"""CPU: the host side of the PCA selection measures (pca, pca_ip, pca_cs, pca_l1, pca_l2) -- the registry, the refusals of the
CLI before any shard is read, the defaults, the numpy restatement (tests/_pca_measure_np.py) against float64 and against torch's
cosine_similarity, the launch plan of acav_pair_scores and the argument checks of acav_pair_scores / acav_rank_desc, none of
which needs a device."""
import ctypes as C

import numpy as np
import pytest

from tests import _pca_measure_np as R

NAMES = {'pca': 'inner_product', 'pca_ip': 'inner_product', 'pca_cs': 'cosine_similarity', 'pca_l1': 'euclidean_diff_l1',
         'pca_l2': 'euclidean_diff_l2'}


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


# ------------------------------------------------------------------------------------------------ registry and refusals
def test_registry_names_resolve_to_pcaoptim_with_their_distance():
    from acav100m_amd.subset_selection.measures import get_measure
    from acav100m_amd.subset_selection.measures.pca import DISTANCE_CODES, DISTANCES, PCAOptim
    assert DISTANCES == NAMES
    assert DISTANCE_CODES == {'inner_product': 0, 'cosine_similarity': 1, 'euclidean_diff_l1': 2, 'euclidean_diff_l2': 3}
    for name, kind in NAMES.items():
        cls = get_measure(name)
        assert issubclass(cls, PCAOptim) and cls.measure_type == kind, name
        assert get_measure(name.upper()) is cls
    for name in ('pca_l3', 'pcacs', 'pca_'):
        with pytest.raises(AssertionError, match="no measure named"):
            get_measure(name)


def _args(**over):
    from acav100m_amd.config import SUBSET_DEFAULTS, merge
    return merge(SUBSET_DEFAULTS, over)


@pytest.mark.parametrize("name", sorted(NAMES))
def test_cli_refuses_what_a_pca_measure_cannot_take_before_any_shard_is_read(name, tmp_path):
    from acav100m_amd.subset_selection.cli import run
    nowhere = {"data.path": str(tmp_path / "nowhere" / "shard-{000000..000003}.pkl"), "data.output.path": str(tmp_path / "o.csv"),
               "measure_name": name}  # the shards do not exist: reading one would fail differently (or select nothing)
    with pytest.raises(ValueError, match="weight_type.*ignore pair weights"):
        run(_args(**{"clustering.weight_type": "linear"}, **nowhere))
    with pytest.raises(ValueError, match="celf_ratio.*no lazy variant"):
        run(_args(celf_ratio=0.5, **nowhere))
    with pytest.raises(ValueError, match="concurrent_chunks.*no lockstep form"):
        run(_args(**{"computation.concurrent_chunks": 2}, chunk_size=1, **nowhere))
    with pytest.raises(ValueError, match="concurrent_chunks.*no lockstep form"):
        run(_args(**{"computation.concurrent_chunks": 2}, **nowhere))
    with pytest.raises(ValueError, match="pca.dim"):
        run(_args(**{"pca.dim": 0}, **nowhere))
    assert not (tmp_path / "o.csv").exists()


def test_defaults():
    from acav100m_amd.config import SUBSET_DEFAULTS
    assert SUBSET_DEFAULTS['pca'] == {'dim': None, 'whiten': True}
    # every default from before the pca measures
    rest = {k: v for k, v in SUBSET_DEFAULTS.items() if k != 'pca'}
    assert rest == {
        'data': {'path': 'data', 'output': {'path': 'output.csv'}, 'meta': {'path': None}},
        'computation': {'random_seed': 0, 'num_workers': 40, 'use_gpu': True, 'num_gpus': None, 'dist_backend': 'nccl',
                        'dist_init_method': 'tcp://localhost:9967', 'use_distributed': True, 'load_async': False,
                        'concurrent_chunks': 1},
        'subset': {'ratio': 0.2, 'size': None},
        'clustering': {'pairing': 'combination', 'weight_type': None},
        'batch': {'batch_size': 20, 'selection_size': 4, 'keep_unselected': True},
        'contrastive': {'num_epochs': 3, 'num_warmup_steps': 1, 'base_lr': 2e-4, 'train_batch_size': 128, 'test_batch_size': 128,
                        'cached_epoch': None, 'train_from_cached': False},
        'measure_name': 'batch_mi', 'celf_ratio': 0, 'shuffle_candidates': True, 'chunk_size': None, 'save_cache_as_csvs': True,
        'log_every': 1000, 'log_times': 10, 'verbose': True, 'debug': False,
    }


def test_existing_measures_keep_their_checks():
    from acav100m_amd.subset_selection.run import lockstep_supported
    from acav100m_amd.subset_selection.run_greedy import check_celf_ratio, check_weight_type
    for name in ('mi', 'mem_mi', 'batch_mi'):
        check_weight_type(name, 'linear')
    for name in ('mi', 'mem_mi', 'ami', 'nmi', 'fm', 'rand', 'arand'):
        assert check_celf_ratio(name, 0.5) == 0.5
        lockstep_supported(name)
    lockstep_supported('batch_mi')
    for name in ('batch_mi', 'contrastive'):
        with pytest.raises(ValueError):
            check_celf_ratio(name, 0.5)
    with pytest.raises(ValueError):
        lockstep_supported('contrastive')


def test_pcaoptim_has_no_cpu_path():
    pytest.importorskip("torch")
    from acav100m_amd._lib import AcavError
    from acav100m_amd.subset_selection.measures.pca import PCAOptim
    with pytest.raises(AcavError, match="no CPU path"):
        PCAOptim([np.zeros((4, 2), np.float32)] * 2, device="cpu")
    with pytest.raises(ValueError, match="measure_type"):
        PCAOptim([np.zeros((4, 2), np.float32)] * 2, measure_type='manhattan', device="cpu")


# ------------------------------------------------------------------------------------------------ the restatement
def _views(seed, V, p, D, scale=1.0):
    rs = np.random.RandomState(seed)
    return [(scale * rs.randn(V, p)).astype(np.float32) for _ in range(D)]


# roundings on top of the p of a chain and the P of the pair sum (P - 1 additions, one division), from the operation order:
#   inner_product      term = fl(a b): 1, then p - 1 additions (0 + t is exact): p in all                          -> c = 0
#   euclidean_diff_l1  term = |fl(a - b)|: 1 (|.| and the final negation are exact), then p - 1 additions           -> c = 0
#   euclidean_diff_l2  e = fl(a - b): 1, fl(e e): e twice and the product, 3, then p - 1 additions: p + 2           -> c = 2
#   cosine_similarity  see test_restatement_cosine_against_float64
C_EXTRA = {'inner_product': 0, 'euclidean_diff_l1': 0, 'euclidean_diff_l2': 2}


@pytest.mark.parametrize("kind", sorted(C_EXTRA))
@pytest.mark.parametrize("V,p,D", [(40, 1, 2), (33, 7, 3), (20, 67, 10)])
def test_restatement_against_float64(kind, V, p, D):
    """|score32 - score64| <= gamma_(p + P + c) (sum_pairs sum_j |term_j|) / P with gamma_m = m u / (1 - m u), u = 2^-24: every
    term of a chain carries its own roundings (c + 1 of them, table above) and at most p - 1 of the chain's additions; a distance
    then goes through at most P - 1 additions of the pair sum and the division by float(P).  All factors (1 + delta) on one
    term: p + c + P of them at most."""
    views = _views(V + p, V, p, D)
    for pairs in (R.combination(D), R.bipartite(D), [(0, 0), (D - 1, 0)]):
        got = R.scores32(views, pairs, kind)
        want, mass = R.scores64(views, pairs, kind)
        assert got.dtype == np.float32
        bound = R.gamma(p + len(pairs) + C_EXTRA[kind]) * mass
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), (kind, pairs[:2], np.abs(got - want).max())


@pytest.mark.parametrize("V,p,D", [(40, 1, 2), (33, 7, 3), (20, 67, 10)])
def test_restatement_cosine_against_float64(V, p, D):
    """dot: |dot32 - dot| <= gamma_p sum |a_j b_j| (as the inner product).  Norms: s32 = sum a_j^2 (1 + theta_p) (positive terms),
    n32 = fl(sqrt(s32)) = |a| (1 + theta_p)^(1/2) (1 + delta): relative error <= gamma_p / 2 + u <= gamma_(p/2 + 1); the maximum
    with eps is exact; fl(na nb): gamma_(p + 3); the division: one more.  d32 = dot32 / (na nb)(1 + theta_(p + 4)), so
    |d32 - d| <= gamma_p mass + |d| gamma_(p + 4)(1 + ...) <= gamma_(2 p + 4) mass with mass = sum |a_j b_j| / (|a| |b|) >= |d|;
    the pair sum and the division by P add P.  Second-order terms are O(p^2 u^2) < 2 u here: gamma_(2 p + P + 6) mass."""
    views = _views(7 * V + p, V, p, D)
    for pairs in (R.combination(D), R.bipartite(D), [(0, 0), (D - 1, 0)]):
        got = R.scores32(views, pairs, 'cosine_similarity')
        want, mass = R.scores64(views, pairs, 'cosine_similarity')
        bound = R.gamma(2 * p + len(pairs) + 6) * mass
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), np.abs(got - want).max()
        assert (np.abs(got) <= 1 + 1e-6).all()


def test_restatement_cosine_against_torch():
    """torch.nn.functional.cosine_similarity on the CPU agrees with the eps-form x.y / (max(|x|, eps) max(|y|, eps)) within the
    bound above for rows of ordinary size (norms in [0.1, 10]); near zero norm the two historical torch forms differ (the
    older one clamps the PRODUCT of the norms), so those rows are held to the eps-form alone."""
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(5)
    V, p = 200, 24
    a, b = rs.randn(V, p), rs.randn(V, p)
    a *= (rs.uniform(0.1, 10, V) / np.linalg.norm(a, axis=1))[:, None]
    b *= (rs.uniform(0.1, 10, V) / np.linalg.norm(b, axis=1))[:, None]
    a, b = a.astype(np.float32), b.astype(np.float32)
    got = R.distance32(a, b, 'cosine_similarity')
    ref = torch.nn.functional.cosine_similarity(torch.from_numpy(a), torch.from_numpy(b), dim=1, eps=1e-8).numpy()
    want, mass = R.distance64(a, b, 'cosine_similarity')
    bound = R.gamma(2 * p + 6) * mass
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= 2 * bound).all()  # torch's own fp32 sum: the same bound
    # near-zero norms: the eps-form only
    z = np.zeros((3, p), np.float32)
    tiny = np.full((3, p), 1e-12, np.float32)
    assert R.distance32(z, b[:3], 'cosine_similarity').tobytes() == np.zeros(3, np.float32).tobytes()
    assert R.distance32(z, z, 'cosine_similarity').tobytes() == np.zeros(3, np.float32).tobytes()
    t = R.distance32(tiny, b[:3], 'cosine_similarity')
    n_b = np.linalg.norm(b[:3].astype(np.float64), axis=1)
    want_t = (tiny.astype(np.float64) * b[:3]).sum(1) / (1e-8 * n_b)  # |tiny| = 4.9e-12 < eps: the clamp is what divides
    assert np.allclose(t, want_t, rtol=1e-5, atol=0)


def test_restatement_ranking_and_gain():
    s = np.array([1.0, -0.0, 3.0, 0.0, 3.0, -2.0, 0.0, -0.0], np.float32)
    assert list(R.rank_desc(s, 8)) == [2, 4, 0, 1, 3, 6, 7, 5]
    assert list(R.rank_desc(s, 0)) == [] and list(R.rank_desc(s, 1)) == [2]
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError):
            R.rank_desc(np.array([0.0, bad], np.float32), 1)
    assert R.gain(s, [2, 4, 0, 1]) == [3.0, 6.0, 4.0, 1.0]  # the PREVIOUS score is added, not a running total
    # one pair of identical rows: -0.0 under l1 / l2
    x = _views(0, 5, 3, 1)[0]
    for kind in ('euclidean_diff_l1', 'euclidean_diff_l2'):
        got = R.scores32([x, x], [(0, 1)], kind)
        assert got.tobytes() == np.full(5, -0.0, np.float32).tobytes()


# ------------------------------------------------------------------------------------------------ plan
def _plan(lib, n, p, D, P, cus):
    out = (C.c_int64 * 9)(*([-7] * 9))
    assert lib.acav_pair_scores_plan(n, p, D, P, cus, out) == 0, (n, p, D, P, cus)
    return tuple(out)


def _lds(D):
    chunk = 32 if D <= 10 else 16 if D <= 19 else 8 if D <= 32 else 4  # the widest whose D x 32 padded rows fit 48 KB
    stride = 8 if chunk == 4 else chunk + 4
    assert chunk == 4 or 4 * D * 32 * stride <= 48 << 10
    assert chunk == 32 or 4 * D * 32 * (2 * chunk + 4) > 48 << 10
    return chunk, 4 * (max(D * 32 * stride, 32 * 65) + 32 * D)


def test_pair_scores_plan_table(lib):
    # (n, p, D, P, cus) -> (tile rows, chunk, tiles, workgroups, LDS, scratch, workgroups per CU, passes, passes for the cosine)
    R_, cus = 32, 256
    for n, tiles, grid in [(0, 0, 0), (1, 1, 1), (R_ - 1, 1, 1), (R_, 1, 1), (R_ + 1, 2, 2), (3 * R_ + 1, 4, 4),
                           (768 * R_ - R_, 767, 767), (768 * R_, 768, 768), (768 * R_ + 1, 769, 768),  # 3 per CU: the grid is full
                           (10 ** 6, 31250, 768), (2 ** 37 - 1, 2 ** 32, 768)]:
        assert _plan(lib, n, 64, 10, 45, cus) == (32, 32, tiles, grid, 47360, 8 * 10 + 8 * 45, 3, 1, 1), n
    base = _plan(lib, 1000, 32, 10, 45, cus)
    for p in (1, 3, 31, 32, 33, 69, 16384):  # the plan does not depend on p: the chunk is a function of D alone
        assert _plan(lib, 1000, p, 10, 45, cus) == base
    # LDS of a workgroup against the 160 KB of a compute unit: where a wider D costs a CU a resident workgroup (the grid is
    # capped at 4 per CU), and where a narrower chunk wins it back
    for D, chunk, lds, per_cu in [(1, 32, 8448, 4), (2, 32, 9472, 4), (8, 32, 37888, 4), (9, 32, 42624, 3), (10, 32, 47360, 3),
                                  (11, 16, 29568, 4), (15, 16, 40320, 4), (16, 16, 43008, 3), (19, 16, 51072, 3),
                                  (20, 8, 33280, 4), (24, 8, 39936, 4), (25, 8, 41600, 3), (32, 8, 53248, 3),
                                  (33, 4, 38016, 4), (35, 4, 40320, 4), (36, 4, 41472, 3), (47, 4, 54144, 3), (48, 4, 55296, 2),
                                  (64, 4, 73728, 2)]:
        assert _lds(D) == (chunk, lds), D
        assert per_cu == min(4, (160 << 10) // lds)
        got = _plan(lib, 10 ** 6, 64, D, 1, cus)
        assert (got[1], got[4], got[6], got[3]) == (chunk, lds, per_cu, cus * per_cu), D
    # passes: 64 chains per clip and pass; the cosine adds one norm chain per view
    for D, P, passes, passes_cos in [(10, 45, 1, 1), (10, 54, 1, 1), (10, 55, 1, 2), (10, 64, 1, 2), (10, 65, 2, 2),
                                     (64, 1, 1, 2), (2, 4096, 64, 65), (64, 4096, 64, 65), (63, 4096 - 63, 64, 64)]:
        got = _plan(lib, 100, 8, D, P, 8)
        assert got[7:] == (passes, passes_cos) and got[5] == 8 * D + 8 * P, (D, P)
    out = (C.c_int64 * 9)()
    for args in ((-1, 64, 10, 45, 256), (2 ** 37, 64, 10, 45, 256), (100, 0, 10, 45, 256), (100, 16385, 10, 45, 256),
                 (100, 64, 0, 45, 256), (100, 64, 65, 45, 256), (100, 64, 10, 0, 256), (100, 64, 10, 4097, 256),
                 (100, 64, 10, 45, 0)):
        assert lib.acav_pair_scores_plan(*args, out) == -1, args
    assert lib.acav_pair_scores_plan(100, 64, 10, 45, 256, None) == -1


# ------------------------------------------------------------------------------------------------ EINVAL without a device
def test_pair_scores_refuses_bad_arguments_without_a_device(lib):
    y = [np.ones((6, 4), np.float32) for _ in range(3)]
    table = (C.c_void_p * 3)(*[a.ctypes.data for a in y])
    tp = C.cast(table, C.c_void_p)
    pairs = np.array([[0, 1], [1, 2], [2, 2]], np.int32)
    pp = pairs.ctypes.data_as(C.c_void_p)
    scores = np.full(6, 7.0, np.float32)
    sp = scores.ctypes.data_as(C.c_void_p)
    ok = (tp, 3, 6, 4, pp, 3, 0, sp)

    def call(**over):
        names = ("views", "nviews", "n", "p", "pairs", "npairs", "distance", "scores")
        args = dict(zip(names, ok))
        args.update(over)
        return lib.acav_pair_scores(0, *[args[k] for k in names], None)
    for over in (dict(views=None), dict(pairs=None), dict(scores=None), dict(n=-1), dict(n=2 ** 37), dict(p=0), dict(p=16385),
                 dict(nviews=0), dict(nviews=65), dict(npairs=0), dict(npairs=4097), dict(distance=-1), dict(distance=4)):
        assert call(**over) == -1, over
    for bad in ([[0, 3]], [[-1, 0]], [[0, 1], [3, 0]]):
        b = np.array(bad, np.int32)
        assert call(pairs=b.ctypes.data_as(C.c_void_p), npairs=len(b)) == -1, bad
    nulls = (C.c_void_p * 3)(y[0].ctypes.data, None, y[2].ctypes.data)
    assert call(views=C.cast(nulls, C.c_void_p)) == -1  # a NULL view
    assert call() == -1                                  # host views / host scores: the rows are read on the device
    # no clips: a no-op, whatever the view pointers are, and no device is needed for that
    assert call(n=0, scores=None, views=C.cast(nulls, C.c_void_p)) == 0
    assert call(n=0, distance=9) == -1
    assert (scores == 7.0).all()


def test_rank_desc_refuses_bad_arguments_without_a_device(lib):
    scores = np.arange(5, dtype=np.float32)
    ids, top = np.full(5, -7, np.int64), np.full(5, 7.0, np.float32)
    sp, ip, tp = (a.ctypes.data_as(C.c_void_p) for a in (scores, ids, top))
    for args in ((sp, 5, -1, ip, tp), (sp, 5, 6, ip, tp), (sp, -1, 0, ip, tp), (sp, 2 ** 32, 1, ip, tp), (None, 5, 1, ip, tp),
                 (sp, 5, 1, None, tp), (sp, 5, 1, ip, None), (sp, 5, 5, ip, tp), (sp, 5, 0, None, None)):  # the last two: host pointers
        assert lib.acav_rank_desc(0, *args, None) == -1, args
    assert lib.acav_rank_desc(0, None, 0, 0, None, None, None) == 0  # nothing to rank: a no-op
    assert (ids == -7).all() and (top == 7.0).all()
