"""GPU: `clustering.cli cluster --clustering.algorithm=lloyd --clustering.multi_gpu=rows --computation.num_gpus=2` on the
synthetic shards of tests/golden/synth.py (the data of tests/test_gpu_lloyd_cli.py: 256 rows per shard, the ten real view
widths, K = 32, 4 iterations, ACAV_SEED=0): two workers on the one GPU (gloo), each holding its own shards, write the files
of the one-process run -- every cache_epoch_* state and every label, bit for bit: the sums are integers, and every rank moves the
centres from the same reduced tables.  Plus a one-rank RCCL group with the partitioned path forced: the collectives on the device."""
import os
import pickle
import re
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, ITERS = 32, 4
LLOYD = ["--clustering.algorithm=lloyd", "--clustering.epochs=%d" % ITERS, "--clustering.ncentroids=%d" % K, "--computation.num_workers=0"]
ROWS = ["--computation.num_gpus=2", "--clustering.multi_gpu=rows"]


def _cli(argv, env=None, ok=True):
    full = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        full.pop(k, None)
    full.update({"ACAV_SEED": "0"}, **(env or {}))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full["PYTHONPATH"] = root + os.pathsep + full.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "acav100m_amd.clustering.cli", "cluster"] + argv, env=full, capture_output=True,
                       text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def _state(path):
    """{(model key, layer): what a cache file says of the view}"""
    import torch
    saved = torch.load(path, map_location="cpu", weights_only=False)
    out = {}
    for mk, per in saved.items():
        if not isinstance(per, dict):
            continue
        for layer, dt in per.items():
            std = dt.get("whiten_std")
            out[mk, layer] = (np.asarray(dt["centers"], np.float32).tobytes(), np.asarray(dt["counts"], np.float32).tobytes(),
                              int(dt["count"]), dt.get("algorithm"), None if std is None else np.asarray(std).tobytes())
    return out


def _is_shard(f):
    return f.endswith(".pkl") and not f.startswith("cache_epoch_")


def _labels(path):
    rows = pickle.load(open(path, "rb"))
    return [(r["filename"], sorted((kind, layer, int(lab)) for kind in ("audio", "video")
                                   for layer, lab in r[kind + "_assignments"][0]["array"].items())) for r in rows]


def _same_files(one, two, whitened=False):
    """every cache_epoch_* state and every assignment shard of run `two` is run `one`'s"""
    names = lambda d: sorted(f for f in os.listdir(d) if f.startswith("cache_epoch_") or _is_shard(f))  # noqa: E731
    assert names(one) == names(two) and any(f.startswith("cache_epoch_") for f in names(one)) and any(_is_shard(f) for f in names(one))
    for f in names(one):
        a, b = os.path.join(one, f), os.path.join(two, f)
        if f.startswith("cache_epoch_"):
            sa, sb = _state(a), _state(b)
            assert len(sa) == 10 and sa.keys() == sb.keys()
            for v in sa:
                assert sa[v] == sb[v], (f, v)
                assert sa[v][3] == "lloyd" and (sa[v][4] is not None) == whitened
        else:
            la = _labels(a)
            assert la == _labels(b) and len(la) > 0, f


@pytest.fixture(scope="module")
def data(tmp_path_factory, golden_dir):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, golden_dir)
    import synth
    made = {}

    def shards(n):
        if n not in made:
            root = str(tmp_path_factory.mktemp("acav_lloyd_rows_%d" % n))
            glob = synth.write_feature_shards(root, n_shards=n, rows=256, seed=0)
            made[n] = (root, ["--feature_path=" + glob, "--meta_path=" + os.path.join(root, "videos")])
        return made[n]
    shards.row_bytes = 4 * (sum(synth.AUDIO_DIMS) + sum(synth.VIDEO_DIMS))
    return shards


def _pair(data, n_shards, name, more):
    """the one-process run and the two-worker run with the same options -> (dir one, dir two, log one, log two)"""
    root, common = data(n_shards)
    one, two = os.path.join(root, name + "_one"), os.path.join(root, name + "_two")
    log1 = _cli(common + LLOYD + more + ["--out_path=" + one, "--computation.num_gpus=1"])
    log2 = _cli(common + LLOYD + more + ROWS + ["--out_path=" + two], {"ACAV_DIST_BACKEND": "gloo"})
    assert log2.count("done") == 2 and "clustering.multi_gpu=rows: the rows are partitioned over 2 ranks" in log2
    return one, two, log1, log2


@pytest.fixture(scope="module")
def plain(data):
    return _pair(data, 4, "plain", [])


def test_two_workers_write_the_one_process_files(plain):
    one, two, _log1, log2 = plain
    _same_files(one, two)
    assert len([f for f in os.listdir(two) if f.startswith("cache_epoch_")]) == ITERS
    assert "rank 0 holds 512 of 1024 rows in 2 of 4 shards" in log2 and "rank 1 holds 512 of 1024 rows in 2 of 4 shards" in log2


def test_three_shards_two_and_one(data):
    one, two, _log1, log2 = _pair(data, 3, "three", [])
    _same_files(one, two)
    assert "rank 0 holds 512 of 768 rows in 2 of 3 shards" in log2 and "rank 1 holds 256 of 768 rows in 1 of 3 shards" in log2


def test_kmeanspp_sample_spans_both_ranks(data):
    one, two, log1, log2 = _pair(data, 4, "plus", ["--clustering.init=kmeans++", "--clustering.init_sample=96", "--clustering.init_trials=2"])
    _same_files(one, two)
    potentials = lambda log: sorted(set(re.findall(r"lloyd (\S+): k-means\+\+ seeds from a sample of 96 rows, 2 trials per pick: "  # noqa: E731
                                                   r"potential (\d+) -> (\d+)", log)))
    assert len(potentials(log1)) == 10 and potentials(log1) == potentials(log2)


def test_whitening_merges_the_moments_in_shard_order(data):
    one, two, _log1, _log2 = _pair(data, 4, "white", ["--clustering.whiten=True"])
    _same_files(one, two, whitened=True)


def test_every_rank_streams_several_row_groups(data):
    # six shards: a rank's three do not fit 2.5 shards' worth and stream one by one (a group takes half the budget)
    budget = int(2.5 * 256 * data.row_bytes)
    one, two, log1, log2 = _pair(data, 6, "groups", ["--data.resident_bytes=%d" % budget])
    _same_files(one, two)
    assert log2.count("streaming 3 shards in 3 groups") == 2 and "streaming 6 shards in 6 groups" in log1


def test_cached_epoch_and_resume(data, plain):
    root, common = data(4)
    one, two = plain[:2]
    shard_files = sorted(f for f in os.listdir(two) if _is_shard(f))
    assert len(shard_files) == 4
    copies = {}
    for name, src in (("one", one), ("two", two)):
        for what in ("assign", "resume"):
            dst = copies[name, what] = os.path.join(root, "copy_%s_%s" % (name, what))
            shutil.copytree(src, dst)
            for f in shard_files:
                os.remove(os.path.join(dst, f))
    last = ["--clustering.cached_epoch=%d" % (ITERS - 1)]
    # the two-worker run's caches label the rows as the run itself did, on two workers
    _cli(common + LLOYD + ROWS + last + ["--out_path=" + copies["two", "assign"]], {"ACAV_DIST_BACKEND": "gloo"})
    for f in shard_files:
        assert _labels(os.path.join(copies["two", "assign"], "epoch_%d_" % (ITERS - 1) + f)) == _labels(os.path.join(two, f)), f
    # one more iteration from the cache: two workers continue as one process does
    more = ["--clustering.algorithm=lloyd", "--clustering.ncentroids=%d" % K, "--clustering.epochs=1", "--clustering.resume_training=True",
            "--computation.num_workers=0"] + last
    _cli(common + more + ["--out_path=" + copies["one", "resume"], "--computation.num_gpus=1"])
    _cli(common + more + ROWS + ["--out_path=" + copies["two", "resume"]], {"ACAV_DIST_BACKEND": "gloo"})
    _same_files(copies["one", "resume"], copies["two", "resume"])
    # (a resumed run numbers its first iteration cached_epoch: the file it wrote is cache_epoch_3 again, one iteration further)
    name, = [f for f in os.listdir(two) if f.startswith("cache_epoch_%d_" % (ITERS - 1))]
    before, after = _state(os.path.join(two, name)), _state(os.path.join(copies["two", "resume"], name))
    assert all(after[v][2] == before[v][2] + 1024 for v in before)


def test_pca_with_partitioned_rows_fails_before_anything_is_written(data):
    root, common = data(4)
    out = os.path.join(root, "pca_rows")
    log = _cli(common + LLOYD + ROWS + ["--clustering.pca_dim=8", "--out_path=" + out], {"ACAV_DIST_BACKEND": "gloo"}, ok=False)
    assert "clustering.pca_dim with clustering.multi_gpu=rows on 2 GPUs" in log and "scatter matrices" in log
    assert not os.path.isdir(out) or not [f for f in os.listdir(out) if f.startswith("cache_epoch_") or _is_shard(f)]


def test_one_rank_rccl_group_runs_the_collectives_on_the_device(data, plain, monkeypatch):
    """the partitioned path forced in a group of one rank whose backend is RCCL: every collective of the run -- the int64 SUMs of
    the counts, the picked rows' bits and the tables, the float64 MAX -- runs on the GPU, and the files are the plain run's"""
    import functools
    import torch
    import torch.distributed as dist
    import acav100m_amd
    from acav100m_amd.clustering import run_clustering as rc
    from acav100m_amd.clustering.cli import Cli
    root, common = data(4)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    seen = []
    real = dist.all_reduce

    def recording(t, *a, **kw):
        seen.append((t.device.type, t.dtype, kw.get("op", a[0] if a else dist.ReduceOp.SUM)))
        return real(t, *a, **kw)
    monkeypatch.setattr(rc, "_train_clusters_lloyd", functools.partial(rc._train_clusters_lloyd, force_partitioned=True))
    out = os.path.join(root, "rccl_one_rank")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        monkeypatch.setattr(dist, "all_reduce", recording)
        acav100m_amd.manual_seed(0)
        saved = Cli().cluster(out_path=out, feature_path=common[0].split("=", 1)[1], meta_path=common[1].split("=", 1)[1],
                              **{"clustering.algorithm": "lloyd", "clustering.epochs": ITERS, "clustering.ncentroids": K,
                                 "computation.num_workers": 0})
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(dist, "all_reduce", real)
        dist.destroy_process_group()
    assert len(saved) == 4
    _same_files(plain[0], out)
    assert seen and all(dev == "cuda" for dev, _dt, _op in seen)
    assert any(dt == torch.int64 and op == dist.ReduceOp.SUM for _dev, dt, op in seen)
    assert any(dt == torch.float64 and op == dist.ReduceOp.MAX for _dev, dt, op in seen)
    assert any(dt == torch.int32 for _dev, dt, _op in seen)  # the picked fp32 rows, as bits
