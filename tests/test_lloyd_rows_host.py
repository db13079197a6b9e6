"""CPU: the host side of Lloyd k-means with the rows partitioned over several GPUs (clustering.algorithm=lloyd with
clustering.multi_gpu=rows; acav100m_amd/parallel/lloyd_rows.py): which combinations of options are accepted, the pure row
locator, the replay of the per-shard column moments in global shard order, and the three exchanges under gloo with two CPU
processes.  Every comparison is bit for bit."""
import os
import socket

import numpy as np
import pytest


def _args(**over):
    from acav100m_amd.config import CLUSTERING_DEFAULTS, merge
    return merge(CLUSTERING_DEFAULTS, over)


# (options, world size, refused: None or words of the message)
MATRIX = [
    ({"clustering.algorithm": "lloyd", "clustering.multi_gpu": "rows"}, 2, None),
    ({"clustering.algorithm": "lloyd", "clustering.multi_gpu": "rows"}, 1, None),
    ({"clustering.algorithm": "lloyd", "clustering.multi_gpu": "striped"}, 2, ("striped", "clustering.multi_gpu=rows")),
    ({"clustering.algorithm": "lloyd", "clustering.multi_gpu": "reference"}, 2, ("reference", "clustering.multi_gpu=rows")),
    ({"clustering.algorithm": "lloyd", "clustering.multi_gpu": "rows", "clustering.pca_dim": 8}, 2, ("clustering.pca_dim", "scatter matrices")),
    ({"clustering.multi_gpu": "rows", "clustering.pca_dim": 8}, 2, ("clustering.pca_dim", "scatter matrices")),
    ({"clustering.multi_gpu": "rows", "clustering.whiten": True}, 2, ("clustering.whiten", "column moments")),
    ({"clustering.multi_gpu": "striped", "clustering.whiten": True}, 2, ("clustering.whiten", "column moments")),
    ({"clustering.algorithm": "lloyd", "clustering.multi_gpu": "rows", "clustering.whiten": True}, 2, None),
    ({"clustering.algorithm": "lloyd", "clustering.multi_gpu": "rows", "clustering.whiten": True, "clustering.init": "kmeans++"}, 4, None),
    ({"clustering.algorithm": "lloyd", "clustering.multi_gpu": "striped", "clustering.whiten": True}, 2, ("clustering.whiten", "column moments")),
    ({"clustering.algorithm": "lloyd"}, 8, None),                                                          # views: unchanged
    ({"clustering.algorithm": "lloyd", "clustering.whiten": True, "clustering.pca_dim": 8}, 8, None),
    ({"clustering.whiten": True, "clustering.pca_dim": 8}, 8, None),
    ({"clustering.multi_gpu": "rows"}, 2, None),                                                           # the SGD modes: unchanged
    ({"clustering.multi_gpu": "reference"}, 2, None),
]


@pytest.mark.parametrize("over,world,refused", MATRIX)
def test_mode_matrix(over, world, refused):
    from acav100m_amd.clustering.run_clustering import check_options
    args = _args(**over)
    if refused is None:
        check_options(args, world)
        return
    with pytest.raises(ValueError) as err:
        check_options(args, world)
    for word in refused:
        assert word in str(err.value), (word, str(err.value))


COUNTS = [3, 0, 5, 1, 4]


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_every_row_has_one_owner_and_local_numbers_run_in_shard_order(world):
    from acav100m_amd.parallel.lloyd_rows import locate_rows
    n = sum(COUNTS)
    pos, owner, local = locate_rows(np.arange(n), COUNTS, world)
    assert pos.tolist() == list(range(n)) and owner.dtype == local.dtype == np.int64
    # brute force: the global numbers of every rank's rows, its shards in list order
    first = np.concatenate([[0], np.cumsum(COUNTS)])
    held = {r: np.concatenate([np.arange(first[i], first[i + 1]) for i in range(r, len(COUNTS), world)] + [np.zeros(0, int)])
            for r in range(world)}
    assert sorted(np.concatenate(list(held.values())).tolist()) == list(range(n))  # the partition itself
    for r in range(world):
        mine = np.flatnonzero(owner == r)
        assert mine.tolist() == sorted(held[r].tolist())                            # exactly one owner per row
        assert local[mine].tolist() == list(range(len(mine)))                       # 0 .. n_r - 1 in its shard order
        assert np.array_equal(held[r][local[mine]], mine)


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_locating_a_permutation_agrees_with_concatenation(world):
    import torch
    from acav100m_amd.parallel.lloyd_rows import locate_rows
    n, d = sum(COUNTS), 3
    rs = np.random.RandomState(world)
    shards = [rs.randn(c, d).astype(np.float32) for c in COUNTS]
    everything = np.concatenate(shards)                                              # the one-GPU run's rows
    local_rows = {r: np.concatenate([shards[i] for i in range(r, len(COUNTS), world)] + [np.zeros((0, d), np.float32)])
                  for r in range(world)}
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).numpy()
    for picks in (perm, np.sort(perm[:7]), perm[:1], perm[:0]):
        pos, owner, local = locate_rows(picks, COUNTS, world)
        got = np.zeros((len(picks), d), np.float32)
        for r in range(world):                                                       # every rank fills the positions it owns
            mine = owner == r
            got[pos[mine]] = local_rows[r][local[mine]]
        assert got.tobytes() == everything[picks].tobytes()
    with pytest.raises(ValueError):
        locate_rows([n], COUNTS, world)


def _moments(x):
    x = x.astype(np.float64)
    mean = x.mean(axis=0)
    return len(x), mean, ((x - mean) ** 2).sum(axis=0)


def test_moments_replayed_in_global_shard_order_are_the_single_sequence():
    from acav100m_amd.clustering.whiten import ColumnMoments
    from acav100m_amd.parallel.lloyd_rows import replay_moments
    d, order_matters = 7, False
    for seed, counts in enumerate(([3, 0, 5, 1, 4], [40, 7, 0, 13, 1, 29, 2], [5, 5, 5, 5])):
        rs = np.random.RandomState(seed)
        shards = [(rs.randn(c, d) * 10 ** rs.uniform(-2, 2, d) + rs.randn(d)).astype(np.float32) for c in counts]
        single = ColumnMoments(d, device=None)
        table = np.zeros((len(counts), 2, d))
        for i, x in enumerate(shards):
            if len(x):
                n, mean, m2 = _moments(x)
                single.add_segment(n, mean, m2)
                table[i] = mean, m2
        for w in (1, 2, 3):
            # dealt rank::w, every rank keeps its own shards' entries of a zero-filled table; their union is the table
            parts = []
            for r in range(w):
                part = np.zeros_like(table)
                part[r::w] = table[r::w]
                parts.append(part)
            merged = np.sum([p.view(np.int64) for p in parts], axis=0).view(np.float64)
            assert merged.tobytes() == table.tobytes()
            cm = replay_moments(d, counts, merged)
            assert cm.n == single.n and cm.mean.tobytes() == single.mean.tobytes() and cm.M2.tobytes() == single.M2.tobytes()
            assert cm.std().tobytes() == single.std().tobytes()
            # rank-major order -- every rank's shards first merged among themselves -- is another sequence of Chan merges
            major = ColumnMoments(d, device=None)
            for r in range(w):
                for i in range(r, len(counts), w):
                    if counts[i]:
                        major.add_segment(counts[i], table[i, 0], table[i, 1])
            if w > 1 and (major.mean.tobytes() != single.mean.tobytes() or major.M2.tobytes() != single.M2.tobytes()):
                order_matters = True
    assert order_matters  # the order is not a formality: these inputs tell the two apart


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _exchange_worker(rank, world, port, tmp):
    import datetime
    import sys
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from acav100m_amd.parallel import lloyd_rows as R
        # the per-shard counts: rank r states the shards r::world
        counts = R.exchange_counts({i: COUNTS[i] for i in range(rank, len(COUNTS), world)}, len(COUNTS))
        # the picked rows, bit for bit: -0.0, a subnormal, the largest fp32, and float64 moments
        rows = np.array([[-0.0, 1e-45, 3.4028235e38], [1.5, -0.0, -1e-40], [0.0, -2.5, 7.0], [-0.0, -0.0, -0.0]], np.float32)
        _pos, owner, _loc = R.locate_rows([0, 3, 8, 12], COUNTS, world)
        mine = np.zeros_like(rows)
        mine[owner == rank] = rows[owner == rank]
        got = R.exchange_bits(mine)
        m64 = np.array([[-0.0, 5e-324], [1 / 3, -1e300]], np.float64)
        part = np.zeros_like(m64)
        part[rank::world] = m64[rank::world]
        got64 = R.exchange_bits(part)
        # the int64 tables
        rs = np.random.RandomState(10 + rank)
        sums = rs.randint(-2 ** 61, 2 ** 61, size=(6, 5)).astype(np.int64) // world
        cnts = rs.randint(0, 2 ** 40, size=6).astype(np.int64)
        ts, tc = torch.from_numpy(sums.copy()), torch.from_numpy(cnts.copy())
        R.allreduce_tables(ts, tc)
        changed = R.allreduce_sum([rank + 1, 0, 2 ** 40])
        top = R.allreduce_max([0.5 + rank, float("inf") if rank == 1 else 2.0, 0.0])
        np.savez(os.path.join(tmp, "rank%d.npz" % rank), counts=counts, got=got, got64=got64, sums=sums, cnts=cnts, ts=ts.numpy(),
                 tc=tc.numpy(), changed=np.array(changed), top=np.array(top), rows=rows, m64=m64)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_exchanges_under_gloo_two_processes(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.spawn(_exchange_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=False)
    try:
        import time
        deadline = time.monotonic() + 120
        while not ctx.join(timeout=5):  # (raises when a child failed)
            assert time.monotonic() < deadline, "the two workers did not finish in 120 s"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    r0, r1 = (np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world))
    for r in (r0, r1):
        assert r["counts"].tolist() == COUNTS                                        # both ranks agree on every shard
        assert r["got"].tobytes() == r["rows"].tobytes()                             # -0.0 and the subnormal arrive unchanged
        assert np.signbit(r["got"][0, 0]) and r["got"][0, 1] == np.float32(1e-45) != 0
        assert r["got64"].tobytes() == r["m64"].tobytes()
        assert np.array_equal(r["ts"], r0["sums"] + r1["sums"]) and np.array_equal(r["tc"], r0["cnts"] + r1["cnts"])
        assert r["changed"].tolist() == [3, 0, 2 ** 41]
        assert r["top"].tolist() == [1.5, float("inf"), 0.0]
