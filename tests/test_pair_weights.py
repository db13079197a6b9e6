"""CPU: layer-weighted clustering pairs (`weight_type`) -- pairing.get_cluster_pairing / get_weights against the reference's
output (tests/golden/gen_golden_weights.py), the errors that replace the reference's crashes, and the CLI option."""
import itertools
import json
import os

import numpy as np
import pytest

from acav100m_amd.subset_selection.pairing import _get_weights, get_cluster_pairing, get_weights

KEYS = [(m, "layer_{}".format(i)) for m in ("SlowFast", "VGGish") for i in range(5)]


def _golden(golden_dir):
    with open(os.path.join(golden_dir, "weights_pairing.json")) as f:
        g = json.load(f)
    assert [tuple(k) for k in g["keys"]] == KEYS
    return g["cases"]


def test_weights_and_pairings_equal_the_reference(golden_dir):
    cases = _golden(golden_dir)
    n_ok = n_err = 0
    for case in cases:
        if "error" in case:
            with pytest.raises(ValueError):
                get_cluster_pairing(KEYS, case["pairing"], case["weight_type"])
            n_err += 1
            continue
        got = get_cluster_pairing(KEYS, case["pairing"], case["weight_type"])
        if case["weight_type"] is None:
            assert [list(p) for p in got] == case["pairs"], case["pairing"]
            continue
        assert set(got) == {"pairing", "weights"}
        assert [list(p) for p in got["pairing"]] == case["pairs"], case
        w = np.array(got["weights"], np.float64)
        assert np.array_equal(w, np.array(case["weights"], np.float64)), case  # float64, bit for bit
        n_ok += 1
    assert n_ok > 100 and n_err >= 1


def test_single_layer_pairings():
    assert get_cluster_pairing(KEYS, "layer_0") == [[0, 5]]
    assert get_cluster_pairing(KEYS, "Layer_3") == [[3, 8]]
    assert get_cluster_pairing(KEYS, "penultimate") == [[4, 9]]
    with pytest.raises(ValueError):
        get_cluster_pairing(KEYS[:3] + KEYS[5:8], "penultimate")  # three layer names: no fifth


def test_without_weight_type_nothing_changes():
    for name, want in (("combination", list(itertools.combinations(range(10), 2))),
                       ("bipartite", list(itertools.product(range(5), range(5, 10)))),
                       ("diagonal", [[i, i + 5] for i in range(5)])):
        got = get_cluster_pairing(KEYS, name)
        assert isinstance(got, list) and got == want
        assert get_cluster_pairing(KEYS, name, None) == want


def test_reference_quirks_kept():
    # n_layer from the pairing, not from the number of clusterings: layer_0 is the pair (0, 5) -> 3 layers
    r = get_cluster_pairing(KEYS, "layer_0", "linear_1")
    assert r["pairing"] == [[0, 5]]
    w3 = _get_weights(3, "linear_1")
    assert r["weights"] == [w3[0] * w3[2]]
    # onehot is not normalised; the median normalisation of the others
    assert list(_get_weights(5, "onehot_2")) == [0.0, 0.0, 1.0, 0.0, 0.0]
    w = _get_weights(5, "log_2")
    assert np.median(w) == 1.0
    # the weights are shared by both views: pair (i, j) weighs w[i % n] * w[j % n]
    r = get_cluster_pairing(KEYS, "combination", "exp_0.5")
    w5 = _get_weights(5, "exp_0.5")
    assert r["weights"] == [w5[i % 5] * w5[j % 5] for i, j in r["pairing"]]


@pytest.mark.parametrize("weight_type,pairs,msg", [
    ("onehot", [(0, 1), (2, 3)], "onehot needs a layer index"),
    ("cubic_1", [(0, 1), (2, 3)], "unknown function"),
    ("onehot_2", [(0, 1), (2, 3)], "out of range"),              # 2 layers
    ("linear_1", [(0, 1), (2, 4)], "indexes clustering 4"),      # max index 4 -> 2 layers, indices up to 3
    ("exp_1000", [(0, 1), (2, 3)], "non-finite"),
])
def test_errors(weight_type, pairs, msg):
    with pytest.raises(ValueError, match=msg):
        get_weights(None, pairs, weight_type)


def test_cli_option_parses_and_is_refused_where_it_would_be_ignored(tmp_path):
    from acav100m_amd.config import parse_cli
    from acav100m_amd.subset_selection.cli import Cli, prepare
    cmd, kw = parse_cli(["run", "--clustering.weight_type=linear_1", "--out_path=" + str(tmp_path / "o.csv")])
    assert cmd == "run" and kw["clustering.weight_type"] == "linear_1"
    args = prepare(**kw)
    assert args.clustering.weight_type == "linear_1" and args.clustering.pairing == "combination"
    assert prepare(out_path=str(tmp_path / "o.csv")).clustering.weight_type is None
    _, kw = parse_cli(["run", "--clustering.weight_type", "onehot_4"])
    assert kw["clustering.weight_type"] == "onehot_4"
    for measure in ("ami", "contrastive", "fm"):
        with pytest.raises(ValueError, match="weight_type"):
            Cli().run(**{"clustering.weight_type": "linear_1", "measure_name": measure,
                         "out_path": str(tmp_path / "o.csv"), "shards_path": str(tmp_path / "none-{0..1}.pkl")})


def test_measures_that_ignore_weights_warn():
    from acav100m_amd.subset_selection.measures import get_measure
    from acav100m_amd.subset_selection.run_greedy import WEIGHTED_MEASURES, check_weight_type
    assert set(WEIGHTED_MEASURES) == {"mi", "mem_mi", "batch_mi"}
    for name in ("ami", "nmi", "constant", "fm", "rand", "arand"):
        assert get_measure(name)._takes_weights is False
        with pytest.raises(ValueError):
            check_weight_type(name, "linear_1")
        check_weight_type(name, None)
    for name in WEIGHTED_MEASURES:
        assert get_measure(name)._takes_weights is True
        check_weight_type(name, "linear_1")
