"""GPU: `clustering.cli cluster --clustering.algorithm=lloyd --clustering.spherical=True --clustering.multi_gpu=rows
--computation.num_gpus=2` on the synthetic shards of tests/golden/synth.py, set up exactly as tests/test_gpu_lloyd_rows_cli.py:
two workers on the one GPU (gloo), each holding its own shards, write the files of the one-process run bit for bit -- the row
normalisation is a function of one row, and every rank renormalises its own copy of the identical centres -- once with
clustering.whiten=True in front of it."""
import os

import numpy as np
import pytest

from tests.test_gpu_lloyd_rows_cli import ITERS, LLOYD, ROWS, _cli, _is_shard, _labels, _state, data  # noqa: F401  (data: the fixture)

pytestmark = pytest.mark.gpu


def _flags(path):
    """{(model key, layer): (normalize, spherical, squared norms of the centres)} of a cache file"""
    import torch
    saved = torch.load(path, map_location="cpu", weights_only=False)
    return {(mk, layer): (dt.get("normalize"), dt.get("spherical"), (np.asarray(dt["centers"], np.float64) ** 2).sum(1))
            for mk, per in saved.items() if isinstance(per, dict) for layer, dt in per.items()}


@pytest.mark.parametrize("whiten", [False, True])
def test_two_workers_write_the_one_process_files(data, whiten):
    root, common = data(4)
    more = ["--clustering.spherical=True"] + (["--clustering.whiten=True"] if whiten else [])
    name = "sph_white" if whiten else "sph"
    one, two = os.path.join(root, name + "_one"), os.path.join(root, name + "_two")
    _cli(common + LLOYD + more + ["--out_path=" + one, "--computation.num_gpus=1"])
    log2 = _cli(common + LLOYD + more + ROWS + ["--out_path=" + two], {"ACAV_DIST_BACKEND": "gloo"})
    assert log2.count("done") == 2 and "clustering.multi_gpu=rows: the rows are partitioned over 2 ranks" in log2
    names = lambda d: sorted(f for f in os.listdir(d) if f.startswith("cache_epoch_") or _is_shard(f))  # noqa: E731
    assert names(one) == names(two) and len([f for f in names(one) if f.startswith("cache_epoch_")]) == ITERS
    assert len([f for f in names(one) if _is_shard(f)]) == 4
    for f in names(one):
        a, b = os.path.join(one, f), os.path.join(two, f)
        if not f.startswith("cache_epoch_"):
            la = _labels(a)
            assert la == _labels(b) and len(la) > 0, f
            continue
        sa, sb = _state(a), _state(b)
        assert len(sa) == 10 and sa.keys() == sb.keys()
        for v in sa:
            assert sa[v] == sb[v], (f, v)  # centres, counts, count, algorithm and the std, bit for bit
            assert sa[v][3] == "lloyd" and (sa[v][4] is not None) == whiten
        for fl in (_flags(a), _flags(b)):
            for v, (normalize, spherical, n2) in fl.items():
                assert normalize is True and spherical is True and (np.abs(n2 - 1.0) <= 6e-7).all(), (f, v)
