"""The workgroup placement of k_fy_gather_select_multi (gs_block_map in acav100m_amd/csrc/acav_mi.hip), through the exported
queries acav_gs_block_grid / acav_gs_block_map: no device.  Workgroup 0 is the selection; of the workgroups b >= 1 only those
whose b % 8 (the XCD they land on) lies in {(rot + j) % 8 : j < n_xcd} gather, numbered densely in ascending b; the others are
padding.  n_xcd = 8 is the grid without a subset: g = b - 1, no padding."""
import ctypes as C

import pytest

SELECT, GATHER, NONE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from acav100m_amd import _lib
    return _lib.load_library()


def _row(lib, gather_blocks, n, rot):
    nb = C.c_int64(0)
    assert lib.acav_gs_block_grid(gather_blocks, n, rot, C.byref(nb)) == 0
    role, g = C.c_int(0), C.c_int64(0)
    out = []
    for b in range(nb.value):
        assert lib.acav_gs_block_map(b, n, rot, C.byref(role), C.byref(g)) == 0
        out.append((role.value, g.value))
    return out


@pytest.mark.parametrize("n", [1, 2, 4, 8])
@pytest.mark.parametrize("rot", range(8))
def test_block_map(lib, n, rot):
    classes = {(rot + j) % 8 for j in range(n)}
    for gather_blocks in range(1, 41):
        row = _row(lib, gather_blocks, n, rot)
        assert row[0] == (SELECT, -1)
        seen = []
        for b, (role, g) in enumerate(row[1:], start=1):
            assert role in (GATHER, NONE)
            assert (role == GATHER) == (b % 8 in classes), (b, role)
            if role == GATHER:
                seen.append(g)
            else:
                assert g == -1
        assert seen == list(range(gather_blocks))  # each index once, ascending in b
        assert row[-1][0] == (GATHER if gather_blocks else SELECT)  # no padding behind the last working workgroup
        # the padded grid, counted independently: the selection, and the shortest row whose classes hold gather_blocks workgroups
        b, left = 0, gather_blocks
        while left:
            b += 1
            left -= b % 8 in classes
        assert len(row) == b + 1
        if n == 8:
            assert len(row) == gather_blocks + 1 and all(g == b - 1 for b, (_, g) in enumerate(row) if b)


def test_no_gather_blocks_is_the_selection_alone(lib):
    for n in (1, 2, 4, 8):
        for rot in range(8):
            assert _row(lib, 0, n, rot) == [(SELECT, -1)]


def test_large_rows(lib):
    """the product's grid at 10^6 candidates (977 gather workgroups) and one near the 2^31 limit of a launch"""
    nb, role, g = C.c_int64(0), C.c_int(0), C.c_int64(0)
    for n, rot in ((2, 6), (4, 7), (1, 0), (8, 3)):
        assert lib.acav_gs_block_grid(977, n, rot, C.byref(nb)) == 0
        assert 977 * 8 // n - 8 <= nb.value <= 977 * 8 // n + 8
        assert lib.acav_gs_block_map(nb.value - 1, n, rot, C.byref(role), C.byref(g)) == 0 and (role.value, g.value) == (GATHER, 976)
    assert lib.acav_gs_block_grid(1 << 27, 1, 0, C.byref(nb)) == 0 and nb.value == 8 * ((1 << 27) - 1) + 8 + 1
    assert lib.acav_gs_block_map(nb.value - 1, 1, 0, C.byref(role), C.byref(g)) == 0 and (role.value, g.value) == (GATHER, (1 << 27) - 1)


def test_bad_arguments(lib):
    nb, role, g = C.c_int64(0), C.c_int(0), C.c_int64(0)
    for n in (0, 3, 5, 16, -1):
        assert lib.acav_gs_block_grid(10, n, 0, C.byref(nb)) == -1
        assert lib.acav_gs_block_map(1, n, 0, C.byref(role), C.byref(g)) == -1
    for rot in (-1, 8):
        assert lib.acav_gs_block_grid(10, 4, rot, C.byref(nb)) == -1
        assert lib.acav_gs_block_map(1, 4, rot, C.byref(role), C.byref(g)) == -1
    assert lib.acav_gs_block_grid(-1, 4, 0, C.byref(nb)) == -1
    assert lib.acav_gs_block_grid(10, 4, 0, None) == -1
    assert lib.acav_gs_block_map(-1, 4, 0, C.byref(role), C.byref(g)) == -1
    assert lib.acav_gs_block_map(1, 4, 0, None, C.byref(g)) == -1
    assert lib.acav_gs_block_map(1, 4, 0, C.byref(role), None) == -1
