"""bench.py --dump-outputs without a GPU: which arrays are written, in which dtypes, and the fixed, seeded row sample that
keeps the dump of the largest workload (cfg5's per-GPU slice: 12.5M rows, 2.5M selected clips) under 64 MB."""
import os

import numpy as np
import torch

import bench


class _KM:
    def __init__(self, k, d):
        self.k, self.d = k, d

    def state_arrays(self):
        rs = np.random.RandomState(self.d)
        return rs.randn(self.k, self.d).astype(np.float32), np.full(self.k, 3.0, np.float32), 12345, 0


def _dump(out, n, dims, k, selected):
    rs = np.random.RandomState(0)
    last = {"kms": [_KM(k, d) for d in dims], "S": [int(i) for i in rs.permutation(n)[:selected]],
            "GAIN": rs.rand(selected)}
    labels = [torch.from_numpy(rs.randint(0, k, n).astype(np.int64)) for _ in dims]
    bench.dump_outputs(str(out), last, labels)
    return last, labels


def test_dump_whole_arrays_at_the_default_shape(tmp_path):
    last, labels = _dump(tmp_path, 200_000, (64, 32), 16, 40_000)
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(["centers_v0.npy", "centers_v1.npy", "counts_v0.npy", "counts_v1.npy", "count_v0.npy",
                            "count_v1.npy", "labels.npy", "selected.npy", "gains.npy"])
    got = {n[:-4]: np.load(tmp_path / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["labels"], np.stack([lab.numpy() for lab in labels], 1).astype(np.float32))
    assert np.array_equal(got["selected"].astype(np.int64), last["S"])
    assert got["gains"].dtype == np.float64 and np.array_equal(got["gains"], last["GAIN"])
    assert np.array_equal(got["centers_v1"], last["kms"][1].state_arrays()[0])
    assert list(got["count_v0"]) == [12345.0, 0.0]


def test_dump_samples_large_arrays_the_same_way_every_time(tmp_path):
    n, sel = 3_000_000, 2_200_000
    _, labels = _dump(tmp_path / "a", n, (8, 8), 4, sel)
    _dump(tmp_path / "b", n, (8, 8), 4, sel)
    total = 0
    for name in sorted(os.listdir(tmp_path / "a")):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert np.array_equal(a, b), name
        assert a.size <= bench.DUMP_MAX_VALUES, name
        total += os.path.getsize(tmp_path / "a" / name)
    rows = np.load(tmp_path / "a" / "labels_rows.npy").astype(np.int64)
    assert len(rows) == bench.DUMP_MAX_VALUES // 2 and np.all(np.diff(rows) > 0)
    want = np.stack([lab.numpy() for lab in labels], 1)[rows]
    assert np.array_equal(np.load(tmp_path / "a" / "labels.npy"), want)
    assert os.path.exists(tmp_path / "a" / "selected_rows.npy") and os.path.exists(tmp_path / "a" / "gains_rows.npy")
    assert total < 64e6
