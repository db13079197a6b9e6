"""Which kernels a sweep of acav_kmeans_assign launches (assign_pick_plan, acav_kmeans_form.h), without a GPU:
acav_kmeans_assign_plan answers for a shape, the CU count and the environment switches.  The expected rows of
tests/golden/assign_plans.json were recorded from the selection code this function replaced (the block of nested
ternaries inside acav_kmeans_assign, copied into a host-only program and fed the table's inputs)."""
import ctypes as C
import json
import os
import random

import pytest

SWITCHES = ("ACAV_ASSIGN_EXACT_ONLY", "ACAV_FILTER_PAD", "ACAV_ASSIGN_CAND", "ACAV_ASSIGN_EMIT", "ACAV_CAND_PAIR_CAP",
            "ACAV_FILTER_NT", "ACAV_FILTER_GS", "ACAV_FILTER_NW", "ACAV_FILTER_SCHED")
LEN = 27  # ACAV_ASSIGN_PLAN_LEN; the slots (include/acav_hip.h):
(ERROR, PATH, GRID, FD, RAGGED, NGROUPS, GS, NW, NT, XS, SCHED, DCR, EMIT, EMIT_PASS, CAND, UND_LIST, PAIR_CAP, FILTER_ID, EMIT_ID,
 FGRID, FBLOCK, FSMEM, EGRID, EBLOCK, ESMEM, RGRID, CGRID) = range(LEN)
GUARDED, FAST, FILTER = range(3)


def kernel_id(nt, nw, gs, dcr, sched, emit, xs):
    return int("%d%d%d%d%d%d%d" % (nt, nw, gs, dcr, sched, emit, xs))


# the instantiations of k_assign_f16_rw the library holds: (NW, GS, DCR, SCHED, EMIT) x {NT, default policy, scaled rows}
FAMILIES = ((8, 1, 3, 2, 0), (8, 0, 3, 2, 0), (4, 1, 2, 0, 0), (4, 0, 2, 2, 0), (4, 0, 2, 0, 2), (4, 0, 2, 0, 0), (4, 0, 2, 0, 1))
KERNEL_IDS = {kernel_id(nt, nw, gs, dcr, sched, emit, xs)
              for nw, gs, dcr, sched, emit in FAMILIES for nt, xs in ((1, 0), (0, 0), (1, 1))}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assign_plans.json")) as _f:
    ROWS = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _plan(lib, monkeypatch, d, k, n, aligned=1, need_mean=0, rows_scaled=0, cus=256, env=None):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        assert name in SWITCHES
        monkeypatch.setenv(name, value)
    out = (C.c_int * LEN)(*([-7] * LEN))
    assert lib.acav_kmeans_assign_plan(d, k, n, aligned, need_mean, rows_scaled, cus, out) == 0
    return list(out)


def test_table_covers_the_kernels_and_the_paths():
    assert 50 <= len(ROWS) <= 80 and len({r["name"] for r in ROWS}) == len(ROWS)
    assert len(KERNEL_IDS) == 21
    assert {i for r in ROWS for i in (r["out"][FILTER_ID], r["out"][EMIT_ID]) if i > 0} == KERNEL_IDS
    assert {r["out"][PATH] for r in ROWS if not r["out"][ERROR]} == {GUARDED, FAST, FILTER}
    assert {r["out"][ERROR] for r in ROWS} == {0, 1}
    for name in SWITCHES:
        assert len({r["env"][name] for r in ROWS if name in r["env"]}) >= 2, name


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_assign_plan_matches_recorded_choice(lib, monkeypatch, row):
    got = _plan(lib, monkeypatch, row["d"], row["k"], row["n"], row["aligned"], row["need_mean"], row["rows_scaled"], row["cus"], row["env"])
    assert got == row["out"]


@pytest.mark.parametrize("k,n,env", [(200, 10 ** 6, {"ACAV_FILTER_NW": "8"}), (200, 10 ** 6, {"ACAV_FILTER_SCHED": "2"}),
                                     (256, 10 ** 6, {"ACAV_FILTER_SCHED": "2"}), (200, 10 ** 6, {"ACAV_ASSIGN_EMIT": "0"}),
                                     (1024, 10 ** 6, {"ACAV_ASSIGN_EMIT": "0"}), (200, 10 ** 6, {"ACAV_ASSIGN_CAND": "0"}),
                                     (1024, 10 ** 6, {"ACAV_ASSIGN_CAND": "0"}), (200, 2 ** 27, {}), (1024, 2 ** 27, {})])
def test_switches_that_silently_drop_the_candidate_path(lib, monkeypatch, k, n, env):
    """No emission in place, no emission pass, no k_assign_cand: every undecided row goes to the f32 list and the full exact sweep."""
    out = _plan(lib, monkeypatch, 1024, k, n, env=env)
    assert out[PATH] == FILTER
    assert out[EMIT] == 0 and out[EMIT_PASS] == 0 and out[EMIT_ID] == -1 and out[UND_LIST] == 0 and out[CGRID] == 0
    assert out[FILTER_ID] % 100 // 10 == 0  # the lean kernel
    assert _plan(lib, monkeypatch, 1024, k, 10 ** 6)[UND_LIST] == 1  # the same shape takes the candidate path without the switch


def test_invariants_over_generated_shapes(lib, monkeypatch):
    rng = random.Random(13)
    widths, ns = list(range(32, 2305, 8)), (128, 1000, 10 ** 6, 2 ** 27)
    shapes = {(rng.choice(widths), rng.randint(2, 1024), rng.choice(ns)) for _ in range(4000)}
    shapes |= {(d, k, n) for d in (32, 256, 264, 288, 1024, 2304) for k in (2, 256, 257, 1024) for n in ns}
    paths = set()
    for d, k, n in sorted(shapes):
        out = _plan(lib, monkeypatch, d, k, n)
        assert out[ERROR] == 0 and out[PATH] == FILTER, (d, k, n, out)
        assert out[FSMEM] <= 160 * 1024 and out[ESMEM] <= 160 * 1024
        assert out[NW] in (4, 8) and out[DCR] == (3 if out[NW] == 8 else 2) and out[FBLOCK] == 64 * out[NW]
        assert not out[XS] or out[NT]
        assert out[FILTER_ID] in KERNEL_IDS and out[FILTER_ID] == kernel_id(*(out[i] for i in (NT, NW, GS, DCR, SCHED, EMIT, XS)))
        assert (out[EMIT_ID] in KERNEL_IDS and out[EMIT_ID] // 10 ** 5 % 10 == 4) if out[EMIT_PASS] else out[EMIT_ID] == -1
        paths.add((out[GS], out[NW], out[EMIT], out[EMIT_PASS], out[UND_LIST]))
    assert paths == {(0, 4, 2, 0, 1), (1, 4, 0, 1, 1), (1, 8, 0, 1, 1), (0, 4, 0, 0, 0), (1, 4, 0, 0, 0), (1, 8, 0, 0, 0)}  # the last three: n = 2^27


def test_bad_arguments_are_errors(lib):
    out = (C.c_int * LEN)()
    assert lib.acav_kmeans_assign_plan(0, 256, 1000, 1, 0, 0, 256, out) == -1
    assert lib.acav_kmeans_assign_plan(1024, 0, 1000, 1, 0, 0, 256, out) == -1
    assert lib.acav_kmeans_assign_plan(1024, 256, 0, 1, 0, 0, 256, out) == -1
    assert lib.acav_kmeans_assign_plan(1024, 256, 1000, 1, 0, 0, 0, out) == -1
    assert lib.acav_kmeans_assign_plan(16384, 2 ** 17, 1000, 1, 0, 0, 256, out) == -1  # k * d beyond acav_kmeans_create's limit
    assert lib.acav_kmeans_assign_plan(1024, 256, 1000, 1, 0, 0, 256, None) == -1
