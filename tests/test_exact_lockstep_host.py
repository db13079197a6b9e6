"""CPU: the host side of the exact-greedy measures in lockstep chunks (computation.concurrent_chunks > 1):
which configurations may run in lockstep (run.lockstep_supported), and the new entry point's declaration in the header
and in the ctypes table."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lockstep_supported_accepts_every_measure_but_contrastive():
    from acav100m_amd.subset_selection.measures import _REGISTRY
    from acav100m_amd.subset_selection.run import lockstep_supported
    assert {'mi', 'mem_mi', 'ami', 'nmi', 'constant', 'fm', 'rand', 'arand', 'efficient_fm', 'efficient_rand',
            'efficient_arand', 'batch_mi', 'contrastive'} <= set(_REGISTRY)
    for name in _REGISTRY:
        if name == 'contrastive':
            with pytest.raises(ValueError, match="contrastive"):
                lockstep_supported(name, 0)
        else:
            assert lockstep_supported(name, 0) is None
            assert lockstep_supported(name.upper(), 0) is None  # names are case-insensitive, as in get_measure


def test_lockstep_supported_refuses_celf():
    from acav100m_amd.subset_selection.measures import _REGISTRY
    from acav100m_amd.subset_selection.run import lockstep_supported
    for name in _REGISTRY:
        with pytest.raises(ValueError):
            lockstep_supported(name, 0.5)
    with pytest.raises(ValueError, match="celf_ratio"):
        lockstep_supported('mem_mi', 0.5)


def test_every_exact_measure_class_has_its_own_lockstep_driver():
    """the inherited EfficientBatchMI.run_greedy_multi would run a B = 1 batch greedy on an exact measure without a word"""
    from acav100m_amd.subset_selection.measures import get_measure
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    from acav100m_amd.subset_selection.measures.mi import EfficientMI
    from acav100m_amd.subset_selection.measures.pair import _PairCountingMeasure
    for name in ('mi', 'mem_mi', 'ami', 'nmi', 'constant'):
        assert get_measure(name).run_greedy_multi is EfficientMI.run_greedy_multi
    for name in ('fm', 'rand', 'arand', 'efficient_fm', 'efficient_rand', 'efficient_arand'):
        assert get_measure(name).run_greedy_multi is _PairCountingMeasure.run_greedy_multi
    assert EfficientMI.run_greedy_multi is not EfficientBatchMI.run_greedy_multi


def test_run_exact_multi_is_declared_with_nine_arguments():
    from acav100m_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "acav_hip.h")).read()
    m = re.search(r"\bint\s+acav_mi_run_exact_multi\s*\(([^;]*)\)\s*;", hdr)
    assert m, "acav_mi_run_exact_multi is not declared in include/acav_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 9
    assert params[0] == "acav_mi **mis" and params[1] == "int nchunks" and params[-1] == "int64_t *n_selected"
    sig = _lib.SIGNATURES["acav_mi_run_exact_multi"]
    assert len(sig) == 9
    src = open(os.path.join(ROOT, "acav100m_amd", "csrc", "acav_mi.hip")).read()
    assert re.search(r"ACAV_EXPORT\s+int\s+acav_mi_run_exact_multi\s*\(", src)
