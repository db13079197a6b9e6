"""Which persistent kernel an epoch of acav_kmeans_train runs on (train_pick_form, acav_kmeans_form.h), without a GPU:
acav_kmeans_train_form answers for a shape, a device's limits and the environment switches.  The expected rows of
tests/golden/train_forms.json were recorded from the selection code this function replaced."""
import ctypes as C
import json
import os

import pytest

SWITCHES = ("ACAV_NO_PERSISTENT", "ACAV_FORCE_WIDE", "ACAV_TALL", "ACAV_WIDE_NCP", "ACAV_WIDE_NRP", "ACAV_SPLIT_MINK")
NONE, NARROW, WIDE, SPLIT = range(4)

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_forms.json")) as _f:
    ROWS = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _form(lib, monkeypatch, row):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in row["env"].items():
        assert name in SWITCHES
        monkeypatch.setenv(name, value)
    out = (C.c_int * 8)(*([-1] * 8))
    rc = lib.acav_kmeans_train_form(row["d"], row["k"], row["b"], row["aligned"], row["cus"], row["occ_narrow"], row["occ_split"],
                                    row["has_budget"], row["room"], row["share_lds"], out)
    assert rc == 0
    return list(out)


def test_table_covers_the_forms():
    assert 40 <= len(ROWS) <= 60 and len({r["name"] for r in ROWS}) == len(ROWS)
    assert {r["out"][0] for r in ROWS} == {NONE, NARROW, WIDE, SPLIT}
    wide = {tuple(r["out"][1:4]) for r in ROWS if r["out"][0] == WIDE}  # (ncp, nrp, one_x): every instantiation family
    assert wide == {(1, 1, 0), (1, 1, 1), (2, 1, 0), (2, 1, 1), (2, 2, 1), (4, 1, 0), (8, 1, 0)}


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_train_form_matches_recorded_choice(lib, monkeypatch, row):
    assert _form(lib, monkeypatch, row) == row["out"]


def test_k_above_256_is_never_narrow(lib, monkeypatch):
    """K = 264 ... 304 at d = 1024 once took the narrow kernel, whose sweep reads 32 centre groups, and ignored the rest."""
    for k in range(257, 320):
        row = dict(d=1024, k=k, b=32, aligned=1, cus=256, occ_narrow=1, occ_split=1, has_budget=0, room=0, share_lds=0, env={})
        out = _form(lib, monkeypatch, row)
        assert out[0] == WIDE and out[4] * 8 * out[1] >= k, (k, out)


def test_bad_arguments_are_errors(lib):
    out = (C.c_int * 8)()
    assert lib.acav_kmeans_train_form(0, 256, 32, 1, 256, 1, 1, 0, 0, 0, out) == -1
    assert lib.acav_kmeans_train_form(1024, 256, 32, 1, 256, 1, 1, 0, 0, 0, None) == -1
