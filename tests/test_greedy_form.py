"""What a batch-MI greedy call launches (greedy_pick_form, greedy_group_grids, mt_pick_lanes: acav_mi_form.h), without a GPU:
acav_mi_greedy_form answers for a shape and the environment switches.  The expected rows of tests/golden/greedy_forms.json were
recorded from the code these functions replaced (run_greedy_tiled, FyPlan::build, MtStream::plan and the entry points' own
tiled / legacy choice), not from the functions themselves.  The layouts of form / group / generator: include/acav_hip.h."""
import ctypes as C
import json
import os

import pytest

SWITCHES = ("ACAV_FY_LEGACY", "ACAV_FY_PACK", "ACAV_FY_XCD_AFFINE", "ACAV_GS_XCDS", "ACAV_GS_XCD_ROT", "ACAV_GS_XCD_MIN_L",
            "ACAV_FY_PART_DIRECT", "ACAV_FY_CAP", "ACAV_FY_TILES_MIN", "ACAV_FY_ECAP", "ACAV_MI_SHARE_GEN", "ACAV_MI_QUEUE_PROBE",
            "ACAV_MI_TIMING")
TILED, LEGACY, REFUSED = range(3)
BAD_XCDS, SHORT_LIST, LDS = 1, 2, 3
# form[...]: the fields the coverage test reads
PATH, REFUSAL, WIDE, ITERS_MAX, LMAX, MODE, PACK, STAGED, NTMAX, PROBE, CONSTS, PER_CHUNK = 0, 2, 6, 8, 9, 10, 12, 13, 16, 21, 24, 32

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "greedy_forms.json")) as _f:
    _GOLDEN = json.load(_f)
ROWS, GENERATOR = _GOLDEN["form"], _GOLDEN["generator"]


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _i64(values):
    return (C.c_int64 * len(values))(*values)


def _form(lib, monkeypatch, row):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in row["env"].items():
        assert name in SWITCHES
        monkeypatch.setenv(name, value)
    n = len(row["L"])
    group_size = ROWS[0]["form"][CONSTS]
    form, group, h = _i64([-7] * (PER_CHUNK + 2 * n)), _i64([-7] * (20 + 4 * group_size)), C.c_uint64(7)
    rc = lib.acav_mi_greedy_form(n, _i64(row["L"]), _i64(row["subset"]), row["B"], row["k"], row["keep"], row["max_iters"], row["P"],
                                 row["D"], row["weighted"], form, row["g0"], row["before"], group if row["g0"] >= 0 else None,
                                 C.byref(h), None, None)
    assert rc == 0
    return list(form), list(group) if row["g0"] >= 0 else [], h.value


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_greedy_form_matches_recorded_plan(lib, monkeypatch, row):
    form, group, h = _form(lib, monkeypatch, row)
    assert form == row["form"]
    assert group == row["group"]
    assert h == row["hash"]


@pytest.mark.parametrize("row", GENERATOR, ids=[r["name"] for r in GENERATOR])
def test_generator_lanes_match_recorded_plan(lib, row):
    L, form, out = _i64([600]), _i64([0] * (PER_CHUNK + 2)), _i64([-7] * 8)
    assert lib.acav_mi_greedy_form(1, L, _i64([120]), 20, 4, 1, -1, 3, 3, 0, form, -1, 0, None, None, _i64(row["in"]), out) == 0
    assert list(out) == row["out"]


def test_table_covers_the_edges():
    assert len({r["name"] for r in ROWS}) == len(ROWS) and len({r["name"] for r in GENERATOR}) == len(GENERATOR)
    group_size, depth, pack_max, tiled_max, maxb, phibp, fastbp, fastkp = ROWS[0]["form"][CONSTS:CONSTS + 8]
    assert all(r["form"][CONSTS:CONSTS + 8] == ROWS[0]["form"][CONSTS:CONSTS + 8] for r in ROWS)
    plain = [r for r in ROWS if not r["env"]]
    single = {(r["L"][0], r["B"]): r for r in plain if len(r["L"]) == 1}
    # list lengths: below, at and above a batch; the edges of the queue probe, the gather subset, the packed buckets, the tile table
    lengths = {L for (L, B) in single if B == 20}
    assert {1, 19, 20, 600, 8192, 8193, 100000, 249999, 250000, 799999, 800000, 1000000, pack_max, pack_max + 1, tiled_max,
            tiled_max + 1} <= lengths
    assert [single[(L, 20)]["form"][REFUSAL] for L in (1, 19, 20)] == [SHORT_LIST, SHORT_LIST, 0]
    assert [single[(L, 20)]["form"][PROBE] for L in (249999, 250000)] == [0, 1]
    assert [single[(L, 20)]["form"][PACK] for L in (pack_max, pack_max + 1)] == [1, 0]
    assert [single[(L, 20)]["form"][PATH] for L in (tiled_max, tiled_max + 1)] == [TILED, LEGACY]
    assert {r["form"][STAGED] for r in plain if r["form"][PATH] == TILED} == {0, 1}
    # batch and selection sizes, keep_unselected, max_iters
    for B in (20, maxb, maxb + 1, 256, 1024):
        for k in (1, B // 5, B):
            assert {r["keep"] for r in plain if (r["B"], r["k"]) == (B, k)} == {0, 1}, (B, k)
    assert {r["form"][WIDE] for r in plain if r["B"] in (maxb, maxb + 1)} == {0, 1}
    assert {-1, 0, 3} <= {r["max_iters"] for r in ROWS}
    # B P around SEL_PHIBP and SEL_FASTBP, k P around SEL_FASTKP; the wide batch whose LDS is refused and its neighbour
    bp, kp = {r["B"] * r["P"] for r in plain}, {r["k"] * r["P"] for r in plain if r["B"] * r["P"] <= fastbp}
    assert {phibp, fastbp} <= bp and any(phibp < v < fastbp for v in bp) and any(v > fastbp for v in bp)
    assert fastkp in kp and any(v > fastkp for v in kp)
    assert {r["form"][MODE] for r in plain if r["form"][PATH] == TILED} == {0, 1, 3}
    lds = sorted((r["D"], r["form"][REFUSAL]) for r in plain if (r["B"], r["k"], r["P"]) == (1024, 8, 8) and r["name"].startswith("wide_lds"))
    assert len(lds) == 2 and lds[1] == (lds[0][0] + 1, LDS) and lds[0][1] == 0
    assert {r["form"][REFUSAL] for r in ROWS} == {0, BAD_XCDS, SHORT_LIST, LDS} and {r["weighted"] for r in ROWS} == {0, 1}
    assert any(r["env"].get("ACAV_GS_XCDS") == "3" and r["form"][REFUSAL] == BAD_XCDS for r in ROWS)
    # chunks: unequal lists and subsets; the longest list, the most iterations and chunk 0 are three different chunks
    assert {1, 8, 125} <= {len(r["L"]) for r in ROWS}
    for n in (8, 125):
        r = next(r for r in plain if len(r["L"]) == n and r["form"][PATH] == TILED)
        iters = r["form"][PER_CHUNK:PER_CHUNK + n]
        assert len(set(r["L"])) > 1 and len(set(r["subset"])) > 1 and len(set(iters)) > 1
        assert len({0, r["L"].index(max(r["L"])), iters.index(max(iters))}) == 3
    # groups: the first, a middle and the last, ragged group of three launches; the rotation over the first ten launches, on and off
    for n in (1, 8, 125):
        starts = {}
        for r in ROWS:
            if len(r["L"]) == n and r["g0"] >= 0:
                starts.setdefault((tuple(r["L"]), tuple(sorted(r["env"].items()))), []).append((r["g0"], r["group"][0], r["form"][ITERS_MAX]))
        assert any(len(s) >= 3 and min(s)[0] == 0 and max(s)[0] + max(s)[1] == max(s)[2] and max(s)[1] < group_size for s in starts.values()), n
    rot = {r["env"].get("ACAV_GS_XCD_ROT"): [r["group"][20 + 4 * q + 3] for q in range(10)]
           for r in ROWS if r["g0"] == 0 and r["L"] == [1000000] and set(r["env"]) <= {"ACAV_GS_XCD_ROT"}}
    assert rot["0"] == [0] * 10 and rot["1"] == rot[None] == [4 * q % 8 for q in range(10)]
    # every switch at a value of its own
    assert {name for r in ROWS for name in r["env"]} == set(SWITCHES)
    # the generator: nothing to generate, one lane block, 2 .. 32 lanes, the enlarged lane block, forced lane blocks
    gen = {r["name"]: r for r in GENERATOR}
    assert any(r["out"][4] == 0 for r in GENERATOR) and any(r["out"][4] == 1 and r["out"][2] == 1 for r in GENERATOR)
    assert {2, 4, 8, 16, 32} <= {r["out"][2] for r in GENERATOR if not r["in"][3]}
    assert gen["enlarged"]["out"][1] > gen["not_enlarged"]["out"][1] and gen["enlarged"]["out"][7] == gen["not_enlarged"]["out"][7] == 1
    assert any(r["in"][3] and r["out"][1:3] == r["in"][3:5] for r in GENERATOR)


def test_bad_arguments_are_errors(lib):
    L, S, form, group, out = _i64([600]), _i64([120]), _i64([0] * (PER_CHUNK + 2)), _i64([0] * 84), _i64([0] * 8)

    def call(n=1, L=L, S=S, B=20, k=4, P=3, D=3, form=form, g0=-1, before=0, group=None, mt_in=None, mt_out=None):
        return lib.acav_mi_greedy_form(n, L, S, B, k, 1, -1, P, D, 0, form, g0, before, group, None, mt_in, mt_out)
    assert call() == 0
    assert call(n=0) == -1 and call(L=None) == -1 and call(S=None) == -1 and call(form=None) == -1
    assert call(B=0) == -1 and call(B=1025) == -1 and call(k=0) == -1 and call(k=21) == -1 and call(P=0) == -1 and call(D=0) == -1
    assert call(B=1024, P=9) == -1  # B P beyond the selection's limit
    assert call(L=_i64([0])) == -1 and call(S=_i64([-1])) == -1
    assert call(g0=0, group=group) == 0 and call(g0=16, group=group) == 0
    assert call(g0=8, group=group) == -1 and call(g0=32, group=group) == -1 and call(g0=0, before=-1, group=group) == -1  # 30 iterations
    assert call(mt_in=_i64([1000, 0, 100, 0, 0])) == -1 and call(mt_out=out) == -1
    assert call(mt_in=_i64([1000, 0, 100, 0, 0]), mt_out=out) == 0
    for bad in ([-1, 0, 100, 0, 0], [1000, 625, 100, 0, 0], [1000, 0, -1, 0, 0], [1000, 0, 100, 625, 1], [1000, 0, 100, 624, 3], [1000, 0, 100, 0, 2]):
        assert call(mt_in=_i64(bad), mt_out=out) == -1, bad


def test_a_group_of_a_legacy_or_refused_form_is_an_error(lib, monkeypatch):
    L, S, form, group = _i64([600]), _i64([120]), _i64([0] * (PER_CHUNK + 2)), _i64([0] * 84)
    monkeypatch.setenv("ACAV_FY_LEGACY", "1")
    assert lib.acav_mi_greedy_form(1, L, S, 20, 4, 1, -1, 3, 3, 0, form, 0, 0, group, None, None, None) == -1
    monkeypatch.delenv("ACAV_FY_LEGACY")
    monkeypatch.setenv("ACAV_GS_XCDS", "3")
    assert lib.acav_mi_greedy_form(1, L, S, 20, 4, 1, -1, 3, 3, 0, form, 0, 0, group, None, None, None) == -1
    assert form[PATH] == REFUSED and form[REFUSAL] == BAD_XCDS
