"""CPU-only checks of the product's host side: the C-ABI library loads and exports every symbol
include/acav_hip.h declares, the host MT19937 stream equals torch's (golden), the mirror classes
keep the reference's surface, nothing in the product imports the oracle, the launch plans of the two evaluate kernels
(acav_kmeans_quality_plan, acav_score_plan) and the large scoring fixture against the numpy restatement."""
import ast
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def acav():
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


def test_header_symbols_exported(acav):
    from acav100m_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acav_hip.h")).read()
    declared = set(re.findall(r"\b(acav_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 35
    lib = _lib.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/acav_hip.h but not exported"
    assert declared - {"acav_last_error"} == set(_lib.SIGNATURES), "ctypes table and header drifted"
    assert lib.acav_version() >= 100


# (n, K, cus) -> (row tiles, grid, dynamic LDS bytes, workgroups per CU), read off acav_kmeans_quality as it stood before the
# plan function: tiles = ceil(n / 64); LDS = 8 (6 K + 64 * 34 + 8 * 64) + 4 * 64 * 36 + 4 * 64 = 48 K + 30976 bytes;
# per_cu = max(1, min(4, 163840 // LDS)); grid = min(tiles, cus * per_cu)
QUALITY_PLANS = [
    ((0, 1, 256), (0, 0, 31024, 4)), ((1, 1, 256), (1, 1, 31024, 4)), ((64, 1, 256), (1, 1, 31024, 4)),
    ((65, 1, 256), (2, 2, 31024, 4)), ((65536, 1, 256), (1024, 1024, 31024, 4)), ((65537, 1, 256), (1025, 1024, 31024, 4)),
    ((0, 64, 256), (0, 0, 34048, 4)), ((1, 64, 256), (1, 1, 34048, 4)), ((64, 64, 256), (1, 1, 34048, 4)),
    ((65, 64, 256), (2, 2, 34048, 4)), ((65536, 64, 256), (1024, 1024, 34048, 4)), ((65537, 64, 256), (1025, 1024, 34048, 4)),
    ((0, 1024, 256), (0, 0, 80128, 2)), ((1, 1024, 256), (1, 1, 80128, 2)), ((64, 1024, 256), (1, 1, 80128, 2)),
    ((65, 1024, 256), (2, 2, 80128, 2)), ((32768, 1024, 256), (512, 512, 80128, 2)), ((32769, 1024, 256), (513, 512, 80128, 2)),
    ((0, 2048, 256), (0, 0, 129280, 1)), ((1, 2048, 256), (1, 1, 129280, 1)), ((64, 2048, 256), (1, 1, 129280, 1)),
    ((65, 2048, 256), (2, 2, 129280, 1)), ((16384, 2048, 256), (256, 256, 129280, 1)), ((16385, 2048, 256), (257, 256, 129280, 1)),
    # the K at which a CU holds one workgroup fewer: 163840 / 40960 = 4, / 54592 = 3.001, / 81904 = 2.0004
    ((10 ** 6, 208, 256), (15625, 1024, 40960, 4)), ((10 ** 6, 209, 256), (15625, 768, 41008, 3)),
    ((10 ** 6, 492, 256), (15625, 768, 54592, 3)), ((10 ** 6, 493, 256), (15625, 512, 54640, 2)),
    ((10 ** 6, 1061, 256), (15625, 512, 81904, 2)), ((10 ** 6, 1062, 256), (15625, 256, 81952, 1)),
    # the shapes of tests/_kmeans_quality_np.large_shapes on 256 and on 8 compute units
    ((131137, 5, 256), (2050, 1024, 31216, 4)), ((131137, 70, 256), (2050, 1024, 34336, 4)), ((32833, 2048, 256), (514, 256, 129280, 1)),
    ((4161, 5, 8), (66, 32, 31216, 4)), ((1089, 2048, 8), (18, 8, 129280, 1)),
    ((2 ** 37 - 1, 1, 256), (2 ** 31, 1024, 31024, 4)),
]


@pytest.mark.parametrize("args,want", QUALITY_PLANS, ids=["n{}-k{}-cus{}".format(*a) for a, _ in QUALITY_PLANS])
def test_quality_plan_table(acav, args, want):
    lib = acav.load_library()
    out = (C.c_int64 * 4)(-7, -7, -7, -7)
    assert lib.acav_kmeans_quality_plan(*args, out) == 0
    assert tuple(out) == want


def test_quality_plan_refuses_bad_sizes(acav):
    lib = acav.load_library()
    out = (C.c_int64 * 4)()
    for args in ((-1, 8, 256), (2 ** 37, 8, 256), (100, 0, 256), (100, 2049, 256), (100, 8, 0)):
        assert lib.acav_kmeans_quality_plan(*args, out) == -1, args
    assert lib.acav_kmeans_quality_plan(100, 8, 256, None) == -1


# (C, P, n, m, want_emi) -> (LDS table, table-building workgroups per pair, ids of each, cell workgroups per pair, EMI lanes per
# column, EMI slices Z, EMI partials per pair), read off score_subset_run as it stood before the plan function:
# nb = ceil(C^2 / 4096); LDS table when 4 C^2 <= 81920 (C <= 143), then slices = min(ceil(m / 8192), max(1, 2048 // P)) and
# per = ceil(m / slices), else slices = ceil(m / 256) of 256 ids; lpc = max(16, 256 // 2^floor(log2 C));
# Z = max(1, min(8192 // (P C), n // (2 lpc), 1024)); partials = C Z
SCORE_PLANS = [
    # the cases of tests/golden/subset_scores_large.npz
    ((7, 2, 20000, 20000, 1), (1, 3, 6667, 1, 64, 156, 1092)), ((7, 2, 5000, 5000, 1), (1, 1, 5000, 1, 64, 39, 273)),
    ((7, 2, 20000, 15000, 1), (1, 2, 7500, 1, 64, 156, 1092)),
    ((143, 2, 20000, 20000, 1), (1, 3, 6667, 5, 16, 28, 4004)), ((144, 2, 20000, 20000, 1), (0, 79, 256, 6, 16, 28, 4032)),
    ((300, 2, 20000, 20000, 1), (0, 79, 256, 22, 16, 13, 3900)),
    ((2, 1, 300000, 300000, 1), (1, 37, 8109, 1, 128, 1024, 2048)), ((2, 1, 304097, 304097, 1), (1, 38, 8003, 1, 128, 1024, 2048)),
    ((32, 45, 400000, 400000, 0), (1, 45, 8889, 1, 0, 0, 0)), ((32, 45, 400000, 400000, 1), (1, 45, 8889, 1, 16, 5, 160)),
    # m at one workgroup's share and one past it
    ((2, 1, 8192, 8192, 1), (1, 1, 8192, 1, 128, 32, 64)), ((2, 1, 8193, 8193, 1), (1, 2, 4097, 1, 128, 32, 64)),
    ((2, 1, 20000, 8193, 0), (1, 2, 4097, 1, 0, 0, 0)),
    # the cap on the workgroups per pair: 2048 // P, at least 1
    ((2, 1024, 400000, 400000, 0), (1, 2, 200000, 1, 0, 0, 0)), ((2, 2048, 400000, 400000, 0), (1, 1, 400000, 1, 0, 0, 0)),
    ((2, 2049, 400000, 400000, 1), (1, 1, 400000, 1, 128, 1, 2)),
    ((1, 1, 2 ** 31 - 1, 2 ** 31 - 1, 1), (1, 2048, 1048576, 1, 256, 1024, 1024)),
    # C: one label, the lanes-per-column steps, the last LDS table and the first global one, Z down to 1
    ((1, 1, 1, 1, 1), (1, 1, 1, 1, 256, 1, 1)), ((3, 1, 1000, 1000, 1), (1, 1, 1000, 1, 128, 3, 9)),
    ((15, 1, 1000, 1000, 1), (1, 1, 1000, 1, 32, 15, 225)), ((16, 1, 1000, 1000, 1), (1, 1, 1000, 1, 16, 31, 496)),
    ((64, 2, 2500, 2500, 1), (1, 1, 2500, 1, 16, 64, 4096)),
    ((143, 45, 1000, 1000, 1), (1, 1, 1000, 5, 16, 1, 143)), ((144, 45, 1000, 1000, 1), (0, 4, 256, 6, 16, 1, 144)),
    ((300, 45, 1000, 1000, 1), (0, 4, 256, 22, 16, 1, 300)),
    # Z reaches its cap at n = 1024 * 2 lpc
    ((2, 1, 262143, 262143, 1), (1, 32, 8192, 1, 128, 1023, 2046)), ((2, 1, 262144, 262144, 1), (1, 32, 8192, 1, 128, 1024, 2048)),
]


@pytest.mark.parametrize("args,want", SCORE_PLANS, ids=["c{}-p{}-n{}-m{}-emi{}".format(*a) for a, _ in SCORE_PLANS])
def test_score_plan_table(acav, args, want):
    lib = acav.load_library()
    out = (C.c_int64 * 7)(*([-7] * 7))
    assert lib.acav_score_plan(*args, out) == 0
    assert tuple(out) == want


def test_score_plan_refuses_bad_sizes(acav):
    lib = acav.load_library()
    out = (C.c_int64 * 7)()
    for args in ((0, 1, 10, 10, 1), (32769, 1, 10, 10, 1), (2, 0, 10, 10, 1), (2, 65536, 10, 10, 1), (2, 1, 0, 0, 1),
                 (2, 1, 2 ** 31, 10, 1), (2, 1, 10, 0, 1), (2, 1, 10, 11, 1)):
        assert lib.acav_score_plan(*args, out) == -1, args
    assert lib.acav_score_plan(2, 1, 10, 10, 1, None) == -1


def test_large_scoring_fixture_is_what_the_restatement_gives(golden_dir):
    """tests/golden/subset_scores_large.npz holds seeds, not arrays: the inputs rebuilt from them give, through the numpy
    restatement, exactly the recorded distances from sklearn -- the fixture is checked without a GPU and without sklearn"""
    from tests import _subset_scores_np as R
    g = np.load(os.path.join(golden_dir, "subset_scores_large.npz"))
    names = g["cases"].tolist()
    assert names == ["c7_n20000", "c143_n20000", "c300_n20000", "c2_n300000", "c2_n304097", "c32_p45_n400000"]
    checked = 0
    for name in names:
        C_, with_emi = int(g[name + ".C"]), bool(g[name + ".emi"])
        assign, ids = R.large_inputs(*(int(g[name + "." + k]) for k in ("seed", "V", "D", "C", "n", "repeats")))
        assert assign.max() == C_ - 1 and len(ids) == int(g[name + ".n"]) == g[name + ".prefix"][-1]
        assert (len(np.unique(ids)) < len(ids)) == bool(g[name + ".repeats"])
        sk, dev = g[name + ".sk"], g[name + ".dev"]
        assert np.isnan(sk[..., 2]).all() == (not with_emi) and np.isfinite(np.delete(sk, 2, -1)).all()
        for q, k in enumerate(g[name + ".prefix"].tolist()):
            for p, (d1, d2) in enumerate(g[name + ".pairs"].tolist()):
                ours = R.compose(R.raw_stats(R.table(assign, ids[:k], d1, d2, C_), with_emi=with_emi))
                got = np.array([abs(ours[m] - s) for m, s in zip(R.NAMES, sk[q, p])])
                assert np.array_equal(got, dev[q, p], equal_nan=True), (name, k, p, got, dev[q, p])
                assert not dev[q, p, 3:].any()  # adjusted_rand, fowlkes_mallows, rand: integers and one division
                checked += 1
    assert checked == 4 + 2 + 2 + 1 + 1 + 45 and float(np.nanmax(g["c300_n20000.dev"])) < 1e-10


def test_trim_device_cache_is_callable_without_a_gpu(acav):
    import acav100m_amd
    assert acav100m_amd.trim_device_cache() >= 0  # nothing parked in a process that never allocated


def test_no_gpu_is_a_loud_error(acav):
    from acav100m_amd.clustering import KMeans
    if acav.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(acav.AcavError, match="no HIP device"):
        KMeans(None, 8, 4).to("cuda")
    from acav100m_amd.subset_selection import get_measure
    m = get_measure("batch_mi")(np.zeros((10, 2), np.int64), ncentroids=1, batch_size=2, selection_size=1,
                                device="cuda")
    with pytest.raises(acav.AcavError, match="no HIP device"):
        m.init([(0, 1)], list(range(1, 10)))


def test_product_rng_equals_torch_stream(acav, golden_dir):
    g = np.load(os.path.join(golden_dir, "rng.npz"))
    for s in (0, 1, 1234):
        r = acav.Generator(s)
        assert np.array_equal(r.rand(7, 5), g[f"s{s}_rand_7x5"])
        assert np.array_equal(r.randperm(10), g[f"s{s}_perm10"])
        assert np.array_equal(r.randperm(1000), g[f"s{s}_perm1000"])
        assert np.array_equal(r.randperm(100003)[:2000], g[f"s{s}_perm100003_head"])
        assert np.array_equal(r.rand(3), g[f"s{s}_rand_after"])


def test_product_rng_live_against_torch(acav):
    import torch
    torch.manual_seed(77)
    r = acav.Generator(77)
    assert np.array_equal(r.rand(33, 3), torch.rand(33, 3).numpy())
    assert np.array_equal(r.randperm(5001), torch.randperm(5001).numpy())
    # default generator == an unseeded torch process (default seed 67280421310721)
    assert torch.initial_seed() == 77
    g2 = acav.Generator()
    torch.manual_seed(67280421310721)
    assert np.array_equal(g2.rand(5), torch.rand(5).numpy())


def test_warmup_best_matches_reference_formula(acav):
    import torch
    torch.manual_seed(5)
    dist = torch.rand(24, 32)
    v, i = dist.min(axis=0)
    best, mean = acav.Generator(5).warmup_best(24, 32)
    assert np.array_equal(best, i.numpy())
    assert abs(mean - v.mean().item()) < 1e-6


def test_kmeans_surface_and_checkpoint_roundtrip(acav, golden_dir):
    """constructor / attributes / get_attrs / load of sgd_clustering.py:18-57 without a GPU"""
    import pickle
    from acav100m_amd.clustering import KMeans
    import torch
    acav.manual_seed(0)
    km = KMeans(None, 8, 16)
    torch.manual_seed(0)
    assert np.array_equal(km.centers.numpy(), (torch.rand(16, 8) * 1e-5).numpy())  # sgd_clustering.py:24
    assert km.count == 0 and km.fallback == 0 and km.lr == 1e-2 and km.initial_rounds == 10
    assert km.reinit == (.7, 5.0) and km.sequential is False and not km.is_distributed
    km.count = 320
    km.counts = np.arange(16, dtype=np.float32)
    dt = km.get_attrs()
    assert set(dt) == {'args', 'count', 'lr', 'initial_rounds', 'reinit', 'fallback', 'sequential', 'centers',
                       'counts'}
    km2 = KMeans.load(dt)
    assert km2.count == 320 and np.array_equal(km2.counts.numpy(), np.arange(16, dtype=np.float32))
    km3 = pickle.loads(pickle.dumps(km))
    assert np.array_equal(km3.centers.numpy(), km.centers.numpy()) and km3.count == 320
    for name in ("to", "initialize", "add", "calc_best", "get_attrs", "load_from_saves", "load"):
        assert callable(getattr(KMeans, name))


def test_run_greedy_host_logic(acav, monkeypatch):
    """_run_greedy (run_greedy.py:9-54): C = max+1, subset = round(ratio*V), B/k clamps, python shuffle,
    start index removed from the candidates -- checked with a recording stand-in measure."""
    import random
    import importlib
    rg = importlib.import_module("acav100m_amd.subset_selection.run_greedy")
    seen = {}

    class Rec:
        def __init__(self, assignments, **kw):
            seen.update(kw, V=assignments.shape[0])

        def init(self, pairs, candidates):
            seen.update(pairs=pairs, candidates=list(candidates))

        def run_greedy(self, subset_size, start_indices, target, **kw):
            seen.update(subset=subset_size, start=list(start_indices))
            return list(range(subset_size)), [0.0] * subset_size, [], []

    monkeypatch.setattr(rg, "get_measure", lambda name: Rec)

    class NS:
        def __init__(self, **kw):
            self.__dict__.update(kw)
    args = NS(batch=NS(batch_size=20, selection_size=4, keep_unselected=True), computation=NS(device="cuda"),
              log_every=1, log_times=None, node_rank=None, parent_pid=None)
    a = np.zeros((15, 3), np.int64)
    a[4, 1] = 6
    random.seed(3)
    rg._run_greedy(args, a, [("a", "l0"), ("a", "l1"), ("v", "l0")], None, 0.2, "batch_mi", "combination", True)
    random.seed(3)
    expect = list(range(15))
    random.shuffle(expect)
    assert seen["ncentroids"] == 7 and seen["subset"] == 3 and seen["batch_size"] == 14
    assert seen["selection_size"] == 4 and seen["start"] == expect[:1] and seen["candidates"] == expect[1:]
    assert seen["pairs"] == [(0, 1), (0, 2), (1, 2)]
    rows = rg.run_greedy(args, a, ["s"] * 15, [f"f{i}" for i in range(15)], [("a", "l0"), ("a", "l1"), ("v", "l0")],
                         None, 0.2, "batch_mi")
    assert [r["filename"] for r in rows] == ["f0", "f1", "f2"]  # sorted(S) (run_greedy.py:72)


def test_product_never_imports_the_oracle():
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "acav100m_amd")):
        for f in files:
            if not f.endswith(".py"):
                continue
            tree = ast.parse(open(os.path.join(dirpath, f)).read())
            for node in ast.walk(tree):
                names = []
                if isinstance(node, ast.Import):
                    names = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    names = [node.module or ""]
                bad += [(f, n) for n in names if n.split(".")[0] == "oracle"]
    assert not bad, bad
    # the native side neither includes nor loads anything from oracle/ (comments may cite it as the spec)
    for f in os.listdir(os.path.join(ROOT, "acav100m_amd", "csrc")):
        src = open(os.path.join(ROOT, "acav100m_amd", "csrc", f)).read()
        assert "libacav_oracle" not in src and "orc_" not in src, f
        assert not re.search(r'#include\s*[<"][^>"]*oracle', src), f


def test_rng_jump_equals_sequential_draws(acav):
    """GF(2) jump-ahead of the MT19937 stream (acav_mtjump.hip: characteristic polynomial by Berlekamp-Massey,
    t^J mod phi, XOR-combination of windows) == drawing the words one by one.  The GPU generator lanes hop over each
    other's blocks with the same polynomials."""
    for seed, pre, n in [(0, 0, 1), (0, 0, 624), (0, 0, 625), (1, 100, 5000), (2, 7, 300_007), (3, 624, 19937 * 3 + 11)]:
        a, b = acav.Generator(seed), acav.Generator(seed)
        for _ in range(pre):
            a.u32(), b.u32()
        a.jump(n)
        for _ in range(n):
            b.u32()
        (ma, ia), (mb, ib) = a.get_state(), b.get_state()
        assert ia == ib and np.array_equal(ma, mb), (seed, pre, n)
        assert [a.u32() for _ in range(700)] == [b.u32() for _ in range(700)]
    # composition: two half jumps == one jump, far beyond anything one would draw sequentially
    a, b = acav.Generator(9), acav.Generator(9)
    n = 624 * 4096 * 31 + 12345
    a.jump(n)
    b.jump(n // 3).jump(n - n // 3)
    assert a.get_state()[1] == b.get_state()[1] and np.array_equal(a.get_state()[0], b.get_state()[0])


def test_python_shuffle_in_library_equals_random_shuffle(acav):
    """run_greedy.py:38-41 shuffles the candidates with Python's generator; acav_rng_py_shuffle reproduces
    random.shuffle(list(range(n))) and leaves `random` in the state the interpreter's own loop would."""
    import random
    from acav100m_amd.rng import python_shuffled_range
    for seed, n in [(0, 1), (0, 2), (0, 10), (1, 1000), (5, 100003), (7, 65536)]:
        random.seed(seed)
        want = list(range(n))
        random.shuffle(want)
        after = [random.random(), random.getrandbits(40)]
        random.seed(seed)
        got = python_shuffled_range(n)
        assert got.tolist() == want, (seed, n)
        assert [random.random(), random.getrandbits(40)] == after, "generator state after the shuffle"


def test_contrastive_rank_rows_short_batches(acav):
    """a batch with fewer rows than ranks (the tail batch of drop_last=False) must not raise on a SUBSET of the
    ranks in front of a collective.  Training drops it on every rank alike (decided from the offsets), inference scores an
    empty slice on the ranks past its end."""
    from acav100m_amd.subset_selection.measures.contrastive import Contrastive
    off = [0, 128, 129]  # a 128-row batch and a 1-row tail, 2 ranks
    per_rank = [Contrastive.rank_rows(off, r, 2) for r in range(2)]
    assert [o.tolist() for _, o in per_rank] == [[0, 64], [0, 64]]          # same number of batches on both ranks
    assert per_rank[0][0].tolist() == list(range(0, 128, 2)) and per_rank[1][0].tolist() == list(range(1, 128, 2))
    inf = [Contrastive.rank_rows(off, r, 2, training=False) for r in range(2)]
    assert inf[0][0].tolist() == list(range(0, 128, 2)) + [128] and inf[0][1].tolist() == [0, 64, 65]
    assert inf[1][0].tolist() == list(range(1, 128, 2)) and inf[1][1].tolist() == [0, 64, 64]
    assert sorted(inf[0][0].tolist() + inf[1][0].tolist()) == list(range(129))  # every row scored exactly once
