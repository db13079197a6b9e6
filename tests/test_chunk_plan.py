"""CPU: the host side of chunked selection that the three chunk drivers share (subset_selection/chunks.py) -- which chunks a
rank takes, the per-chunk subset size, the run's parent_pid, the cache file of a chunk in both formats -- and the one
pre-flight check of `cli.run`, which refuses before any shard is looked for."""
import math
import os

import pytest

from acav100m_amd.config import SUBSET_DEFAULTS, merge
from acav100m_amd.subset_selection import chunks

WORLDS = (1, 2, 3, 5, 8)


def _args(**over):
    return merge(SUBSET_DEFAULTS, over)


# ------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("npaths", [9, 10])
@pytest.mark.parametrize("world", WORLDS)
def test_blocks_cover_every_chunk_once_in_order(npaths, world):
    paths = ["shard-%06d.pkl" % i for i in range(npaths)]
    plans = [chunks.chunk_plan(paths, 2, rank, world, None) for rank in range(world)]
    gpus = max(1, min(world, 5))
    per = math.ceil(5 / gpus)
    for rank, plan in enumerate(plans):
        assert (plan.num_chunks, plan.gpus, plan.rank) == (5, gpus, rank)
        assert [num for num, _ in plan.chunks] == list(range(5))
        assert [p for _, chunk in plan.chunks for p in chunk] == paths
        assert [len(chunk) for _, chunk in plan.chunks] == [2, 2, 2, 2, npaths - 8]  # only the last chunk may be short
        if rank >= gpus:
            assert plan.mine == []
    assert [c for plan in plans for c in plan.mine] == plans[0].chunks
    sizes = [len(plan.mine) for plan in plans if plan.mine]
    assert all(n == per for n in sizes[:-1]) and 1 <= sizes[-1] <= per


def test_subset_size_is_split_over_all_chunks():
    paths = ["shard-%06d.pkl" % i for i in range(10)]
    for rank in range(2):
        assert chunks.chunk_plan(paths, 2, rank, 2, 81).subset_size == 17
        assert chunks.chunk_plan(paths, 2, rank, 2, None).subset_size is None


@pytest.fixture
def shards(tmp_path):
    for i in range(10):
        (tmp_path / ("shard-%06d.pkl" % i)).write_bytes(b"")
    return str(tmp_path / "shard-{000000..000011}.pkl")  # two of the names do not exist


def test_shard_paths_lists_the_existing_files_sorted(shards):
    got = chunks.shard_paths(_args(**{"data.path": shards}))
    assert [os.path.basename(str(p)) for p in got] == ["shard-%06d.pkl" % i for i in range(10)]


def test_plan_chunks_leaves_the_callers_args_alone(shards, monkeypatch, capsys):
    monkeypatch.setattr(chunks, "world", lambda: (1, 2))
    args = _args(**{"data.path": shards, "subset.size": 81}, chunk_size=2, parent_pid=4242)
    plan, chunk_args = chunks.plan_chunks(args)
    assert capsys.readouterr().out == "running 5 chunks in 2 gpus\n"
    assert (args.subset.size, args.node_rank, args.parent_pid) == (81, None, "4242")
    assert (chunk_args.subset.size, chunk_args.node_rank, chunk_args.parent_pid) == (17, 1, "4242")
    assert [num for num, _ in plan.mine] == [3, 4]
    # the index within the block names the file, not the chunk's number
    assert [chunks.cache_name(plan, i) for i in range(len(plan.mine))] == ["cache_4242_1_0", "cache_4242_1_1"]
    args = _args(**{"data.path": shards}, chunk_size=2)
    assert chunks.plan_chunks(args)[1].subset.size is None


def test_excess_ranks_are_announced_before_the_banner_only_when_asked(shards, monkeypatch, capsys):
    monkeypatch.setattr(chunks, "world", lambda: (6, 8))
    banner = "running 5 chunks in 5 gpus\n"
    plan, _ = chunks.plan_chunks(_args(**{"data.path": shards}, chunk_size=2))
    assert plan.mine == [] and capsys.readouterr().out == banner
    chunks.plan_chunks(_args(**{"data.path": shards}, chunk_size=2), announce_excess=True)
    assert capsys.readouterr().out == ("num_gpus (8) exceeds num_chunks (5)\nthresholding num_gpus to be equal to num_chunks\n"
                                       + banner)


def test_parent_pid_explicit_then_environment_then_own(monkeypatch):
    monkeypatch.setenv("ACAV_PARENT_PID", "777")
    assert chunks.resolve_parent_pid(_args(parent_pid=4242)) == "4242"
    args = _args()
    assert chunks.resolve_parent_pid(args) == "777" and args.parent_pid == "777"
    monkeypatch.delenv("ACAV_PARENT_PID")
    assert chunks.resolve_parent_pid(_args()) == str(os.getpid())


# ------------------------------------------------------------------------------------------------------ the cache files
def test_csv_and_pkl_caches_reduce_to_the_same_output(tmp_path):
    from acav100m_amd.subset_selection.run import merge_all_csvs, reduce_all_pkls
    plan = chunks.chunk_plan(["a", "b", "c", "d"], 2, 0, 1, None)._replace(parent_pid="55")
    rows = [[{"filename": "clip_a.mp4", "shard_name": "shard-000000"}, {"filename": "clip_b.mp4", "shard_name": "shard-000001"}],
            [{"filename": "clip_c.mp4", "shard_name": "shard-000002"}, {"filename": "clip_d.mp4", "shard_name": "shard-000002"}]]
    metas = [{"shard-000000": {"clip_a": {"filename": "clip_a.mp4", "id": "vid_a", "segment": [10, 20]}}},  # clip_b has none
             {"shard-000002": {"clip_c": {"filename": "clip_c.mp4", "id": "vid_c", "segment": [0.5, 10.5]},
                               "clip_d": {"filename": "clip_d.mp4", "id": "vid,d", "segment": [30, 40]}}}]
    outs = {}
    for as_csv, suffix in ((True, "_output.csv"), (False, ".pkl")):
        args = _args(**{"data.output.path": str(tmp_path / suffix.strip("._") / "output.csv")}, save_cache_as_csvs=as_csv)
        written = [chunks.save_chunk(args, plan, i, rows[i], metas[i]) for i in range(2)]
        assert [p.name for p in written] == ["cache_55_0_%d%s" % (i, suffix) for i in range(2)]
        caches = args.data.output.path.parent / "caches"
        assert sorted(p.name for p in caches.iterdir()) == [p.name for p in written]
        assert (merge_all_csvs if as_csv else reduce_all_pkls)(args) == 4
        outs[as_csv] = args.data.output.path.read_bytes()
    assert outs[True] == outs[False]
    assert outs[True].splitlines()[:2] == [b'shard-000000,clip_a.mp4,vid_a,"[10, 20]"', b'shard-000001,clip_b.mp4,-1,"[-1.0, -1.0]"']


# ------------------------------------------------------------------------------------------------- the pre-flight check
REFUSED = [
    ({"celf_ratio": 0.5, "measure_name": "batch_mi"}, "celf_ratio.*no lazy variant"),
    ({"clustering.weight_type": "linear_1", "measure_name": "ami"}, "weight_type.*ignore pair weights"),
    ({"computation.concurrent_chunks": 2, "measure_name": "contrastive", "chunk_size": 2}, "concurrent_chunks.*no lockstep form"),
    ({"computation.concurrent_chunks": 2, "measure_name": "pca_l2"}, "concurrent_chunks.*no lockstep form"),
    ({"pca.dim": 0, "measure_name": "pca"}, "pca.dim"),
]


@pytest.mark.parametrize("over,message", REFUSED, ids=[o["measure_name"] for o, _ in REFUSED])
def test_a_refused_run_looks_for_no_shard(over, message, tmp_path):
    from acav100m_amd.subset_selection import cli
    glob = str(tmp_path / "nowhere" / "shard-{000000..000003}.pkl")  # no such directory
    out = tmp_path / "out" / "output.csv"
    with pytest.raises(ValueError, match=message):
        cli.run(_args(**{"data.path": glob, "data.output.path": str(out)}, **over))
    with pytest.raises(ValueError, match=message):
        cli.Cli().run(shards_path=glob, out_path=str(out), **over)
    assert not out.exists() and not (out.parent / "caches").exists() and not (tmp_path / "nowhere").exists()
