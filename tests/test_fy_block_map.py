"""The workgroup placement of k_fy_tile_multi / k_fy_resolve_multi (fy_block_map in acav100m_amd/csrc/acav_mi.hip), through
the exported queries acav_fy_block_grid / acav_fy_block_map: no device.  A 3-D grid of nx x ny x gz workgroups is launched as
one row in which all workgroups of a (y, z) item share b % 8 (the XCD they land on)."""
import ctypes as C
import itertools

import pytest

GRIDS = list(itertools.product((1, 5, 489), (1, 3, 10), (1, 7, 8, 9, 16)))


@pytest.fixture(scope="module")
def lib():
    from acav100m_amd import _lib
    return _lib.load_library()


def _row(lib, nx, ny, gz):
    n = C.c_int64(0)
    assert lib.acav_fy_block_grid(nx, ny, gz, C.byref(n)) == 0
    x, y, z = C.c_int(0), C.c_int(0), C.c_int(0)
    out = []
    for b in range(n.value):
        assert lib.acav_fy_block_map(b, nx, ny, gz, C.byref(x), C.byref(y), C.byref(z)) == 0
        out.append((x.value, y.value, z.value))
    return out


@pytest.mark.parametrize("nx,ny,gz", GRIDS)
def test_block_map(lib, nx, ny, gz):
    row = _row(lib, nx, ny, gz)
    items = ny * gz
    work = [(b, q) for b, q in enumerate(row) if q != (-1, -1, -1)]
    # every workgroup of the 3-D grid exactly once, and nothing outside it
    assert sorted(q for _, q in work) == sorted(itertools.product(range(nx), range(ny), range(gz)))
    if items < 8:  # the old order: x fastest, then y, then z; no padding
        assert len(row) == nx * items
        assert row == [(b % nx, (b // nx) % ny, b // (nx * ny)) for b in range(len(row))]
        return
    # padding: only what rounds every class up to the same number of items
    per_class = -(-items // 8)
    assert len(row) == 8 * nx * per_class
    assert len(row) - len(work) == nx * (8 * per_class - items)
    # the workgroups of an item share b % 8
    cls = {}
    for b, (x, y, z) in work:
        assert cls.setdefault((y, z), b % 8) == b % 8
    # the items are dealt evenly over the eight classes
    counts = [sum(1 for c in cls.values() if c == r) for r in range(8)]
    assert sum(counts) == items and max(counts) - min(counts) <= 1
    # within a class: item after item, each item's nx workgroups in one run with x ascending, and the padding (if any) last
    for r in range(8):
        mine = row[r::8]
        assert len(mine) == nx * per_class
        seen = []
        for s in range(per_class):
            run = mine[s * nx:(s + 1) * nx]
            if run[0] == (-1, -1, -1):
                assert s == per_class - 1 and all(q == (-1, -1, -1) for q in run)
                continue
            assert [q[0] for q in run] == list(range(nx)) and len({q[1:] for q in run}) == 1
            seen.append(run[0][1:])
        assert len(set(seen)) == len(seen) == counts[r]


def test_block_map_arguments(lib):
    n = C.c_int64(0)
    x, y, z = C.c_int(0), C.c_int(0), C.c_int(0)
    assert lib.acav_fy_block_grid(0, 1, 1, C.byref(n)) == -1
    assert lib.acav_fy_block_grid(1, 1, 1, None) == -1
    assert lib.acav_fy_block_grid(5, 3, 16, C.byref(n)) == 0 and n.value == 8 * 5 * 6
    assert lib.acav_fy_block_map(n.value, 5, 3, 16, C.byref(x), C.byref(y), C.byref(z)) == -1
    assert lib.acav_fy_block_map(-1, 5, 3, 16, C.byref(x), C.byref(y), C.byref(z)) == -1
    assert lib.acav_fy_block_map(0, 5, 3, 16, None, C.byref(y), C.byref(z)) == -1
    # a row beyond 2^31 - 1 workgroups cannot be launched: the loop falls back to the 3-D grid, the query refuses
    assert lib.acav_fy_block_grid(1 << 24, 64, 16, C.byref(n)) == 0 and n.value == 8 * (1 << 24) * 128
    assert lib.acav_fy_block_map(0, 1 << 24, 64, 16, C.byref(x), C.byref(y), C.byref(z)) == -1
