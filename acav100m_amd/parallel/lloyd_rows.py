"""Lloyd k-means with the rows PARTITIONED over the ranks (clustering.algorithm=lloyd, clustering.multi_gpu=rows): rank r holds
the shards paths[r::world], and the run produces the files of the one-GPU run.  What crosses the ranks:

  row numbering   the one-GPU run numbers its rows shard by shard in list order.  The ranks exchange their per-shard row counts
                  once (exchange_counts); locate_rows -- pure -- then says which rank owns a global row and where it sits there
  picked rows     the K initial rows, or the k-means++ sample: every rank fills the positions it owns of a zero-filled array, and
                  the array is summed as INTEGERS (exchange_bits): every position has one owner, so the sum is that owner's bits
                  -- a float sum would turn -0.0 into +0.0
  magnitude       the largest |x| per view, MAX (allreduce_max): the fixed-point shift is the one-GPU run's
  tables          [sums || counts] int64 per view and iteration, SUM (allreduce_tables): integer sums do not depend on who added
                  what, so the reduced tables are the one-GPU run's bit for bit; and the changed-label counts, SUM
  moments         clustering.whiten: the per-shard float64 (n, mean, M2), exchanged as bits and replayed in GLOBAL shard order
                  (replay_moments): the one-GPU run's sequence of Chan merges

Collectives go through torch.distributed on kmeans_dp._collective_device(): RCCL on the GPUs, gloo when several ranks share one
GPU.  Every rank issues the same sequence of collectives whatever its own rows look like: each helper here is exactly one
collective, called unconditionally by the driver (run_clustering._train_clusters_lloyd)."""
import numpy as np


def locate_rows(rows, shard_counts, world_size):
    """Pure: global row numbers `rows` (any order) -> (position in `rows`, owning rank, local row number), three int64 arrays of
    len(rows).  shard_counts: rows of every shard in list order (empty shards allowed); shard i belongs to rank i % world_size,
    whose local numbering runs over ITS shards in list order."""
    rows = np.asarray(rows, np.int64).reshape(-1)
    counts = np.asarray(shard_counts, np.int64).reshape(-1)
    w = int(world_size)
    if w < 1 or (counts < 0).any():
        raise ValueError("world_size = {} and shard counts {}: need a world of at least 1 and counts >= 0".format(w, counts.tolist()))
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)  # global first row of every shard, and the total
    if len(rows) and (rows.min() < 0 or rows.max() >= start[-1]):
        raise ValueError("a row number lies outside [0, {})".format(int(start[-1])))
    local_start = np.zeros(len(counts), np.int64)  # first LOCAL row of every shard on its owner
    for r in range(w):
        mine = counts[r::w]
        local_start[r::w] = np.concatenate([[0], np.cumsum(mine)[:-1]]) if len(mine) else mine
    # side='right': among shards that start at the same row (empty ones before it) the last, non-empty one
    shard = np.searchsorted(start, rows, side='right') - 1
    return np.arange(len(rows), dtype=np.int64), (shard % w).astype(np.int64), local_start[shard] + (rows - start[shard])


def replay_moments(d, counts, moments):
    """Pure: per-shard column moments in GLOBAL shard order -> whiten.ColumnMoments after one add_segment per non-empty shard, in
    that order -- the one-GPU run's sequence of Chan merges.  counts [S] rows per shard, moments [S, 2, d] float64 (mean, M2)."""
    from ..clustering.whiten import ColumnMoments
    cm = ColumnMoments(d, device=None)
    for n, m in zip(np.asarray(counts, np.int64), np.asarray(moments, np.float64)):
        if n > 0:  # an empty shard is no segment (run_clustering._shard_prefix skips it)
            cm.add_segment(int(n), m[0], m[1])
    return cm


def _device():
    from .kmeans_dp import _collective_device
    return _collective_device()


def exchange_counts(mine, n_shards):
    """{global shard index: rows} of this rank's shards -> int64 [n_shards] of every rank's, by one SUM of zero-filled arrays"""
    import torch
    import torch.distributed as dist
    t = torch.zeros(int(n_shards), dtype=torch.int64)
    for i, n in mine.items():
        t[int(i)] = int(n)
    t = t.to(_device())
    dist.all_reduce(t)
    return t.cpu().numpy()


def exchange_bits(a):
    """numpy array (float32 / float64 / any 4- or 8-byte type) that is zero wherever another rank owns the position -> the array
    with every owner's BITS in place, on every rank: one SUM over its integer view (x + 0 + ... + 0 in integers is x; in floats
    -0.0 would come back as +0.0)"""
    import torch
    import torch.distributed as dist
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize not in (4, 8):
        raise ValueError("exchange_bits takes 4- or 8-byte elements, not {}".format(a.dtype))
    ints = a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()
    t = torch.from_numpy(ints).to(_device())
    dist.all_reduce(t)
    return t.cpu().numpy().view(a.dtype).reshape(a.shape)


def allreduce_max(values):
    """list of python floats -> their MAX over the ranks (float64; inf and NaN travel as they are)"""
    import torch
    import torch.distributed as dist
    t = torch.tensor([float(v) for v in values] + [0.0], dtype=torch.float64).to(_device())  # (never an empty collective)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return [float(v) for v in t.cpu()[:-1]]


def allreduce_tables(sums, counts):
    """sums int64 [K, d] and counts int64 [K] (torch tensors, updated in place) <- their SUM over the ranks: one all-reduce of
    [sums || counts].  On the tensors' own device when that is the collective device (RCCL), through the host otherwise (gloo)."""
    import torch
    import torch.distributed as dist
    flat = torch.cat([sums.reshape(-1), counts.reshape(-1)])
    dev = _device()
    moved = flat if flat.device == dev else flat.to(dev)
    dist.all_reduce(moved)
    flat = moved if moved.device == sums.device else moved.to(sums.device)
    sums.copy_(flat[:sums.numel()].view_as(sums))
    counts.copy_(flat[sums.numel():])
    return sums, counts


def allreduce_sum(values):
    """list of python ints -> their SUM over the ranks (int64)"""
    import torch
    import torch.distributed as dist
    t = torch.tensor([int(v) for v in values] + [0], dtype=torch.int64).to(_device())  # (never an empty collective)
    dist.all_reduce(t)
    return [int(v) for v in t.cpu()[:-1]]
