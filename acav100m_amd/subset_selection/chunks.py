"""Chunked mode's plan and cache files, shared by the three chunk drivers (run.run_chunks, run_pca.run_chunks_pca,
run_contrastive.run_chunks_contrastive): the reference's get_chunks / split_chunks / run_chunks preamble (chunk.py:21-53,
utils.split_chunks) and its per-chunk cache (chunk.py:125-131).  Imports none of the drivers."""
import copy
import math
import os
from collections import namedtuple
from pathlib import Path

from .. import shards as io
from ..parallel import world

# chunks: [(number, [shard paths])] of the run; mine: this rank's block of them; subset_size: per chunk; parent_pid: plan_chunks'
ChunkPlan = namedtuple('ChunkPlan', 'chunks num_chunks gpus rank mine subset_size parent_pid')


def shard_paths(args):
    """the shard files of data.path that exist, sorted"""
    return [p for p in sorted(io.brace_expand(args.data.path)) if Path(p).is_file()]


def resolve_parent_pid(args):
    """chunk.py:22: one name for all processes of a run -- the explicit value, else the launcher's, else this process's"""
    args.parent_pid = str(args.parent_pid or os.environ.get('ACAV_PARENT_PID') or os.getpid())
    return args.parent_pid


def chunk_plan(paths, chunk_size, rank, world, subset_size):
    """Pure: chunks of `chunk_size` paths; rank r of gpus = max(1, min(world, num_chunks)) takes the r-th contiguous block
    of ceil(num_chunks / gpus) chunks (ranks past gpus: none); an integer subset size is split evenly over ALL chunks."""
    chunks = list(enumerate(io.chunked(paths, int(chunk_size))))
    num_chunks = len(chunks)
    gpus = max(1, min(world, num_chunks))
    per = math.ceil(num_chunks / gpus)
    mine = chunks[rank * per:(rank + 1) * per] if rank < gpus else []
    if isinstance(subset_size, int):
        subset_size = math.ceil(subset_size / num_chunks)
    return ChunkPlan(chunks, num_chunks, gpus, rank, mine, subset_size, None)


def plan_chunks(args, announce_excess=False):
    """-> (plan of THIS process's rank, chunk_args): `args` gets its parent_pid; chunk_args is a copy of it with the per-chunk
    subset.size and node_rank = rank."""
    pid = resolve_parent_pid(args)
    rank, w = world()
    plan = chunk_plan(shard_paths(args), args.chunk_size, rank, w, args.subset.size)._replace(parent_pid=pid)
    if announce_excess and w > plan.num_chunks:
        print("num_gpus ({}) exceeds num_chunks ({})".format(w, plan.num_chunks))
        print("thresholding num_gpus to be equal to num_chunks")
    chunk_args = copy.deepcopy(args)
    chunk_args.subset.size = plan.subset_size
    chunk_args.node_rank = rank
    print("running {} chunks in {} gpus".format(plan.num_chunks, plan.gpus))
    return plan, chunk_args


def cache_name(plan, i):
    """the cache of the i-th chunk of this rank's block (not the chunk's number: the reducers group by pid and rank)"""
    return "cache_{}_{}_{}".format(plan.parent_pid, plan.rank, i)


def save_chunk(args, plan, i, res, metas):
    """chunk.py:125-131: the chunk's selection as caches/{name}_output.csv, or -- save_cache_as_csvs=False -- as the
    pickle caches/{name}.pkl = {'res', 'metas'} that `cli.py reduce_pkls` turns into the csv later"""
    name = cache_name(plan, i)
    cache_dir = Path(args.data.output.path).parent / 'caches'
    if args.save_cache_as_csvs or args.save_cache_as_csvs is None:
        out_path, _ = io.append_output_csv(res, metas, cache_dir / Path(args.data.output.path).name, name + '_')
        return out_path
    cache_dir.mkdir(parents=True, exist_ok=True)
    out_path = cache_dir / (name + '.pkl')
    io.dump_pickle({'res': res, 'metas': metas}, out_path)
    return out_path
