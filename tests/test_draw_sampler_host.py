"""CPU-only checks of batch.sampler=draw: the prefix property that justifies it (the first B steps of randperm's loop fix the
first B entries of the permutation), the launch plan acav_mi_draw_form (iterations, generator words, the split into launches,
the short-list refusal at its exact boundary, the limits), check_sampler, and the restatement's shrink rule."""
import numpy as np
import pytest

from tests import _draw_sampler_np as R


@pytest.fixture(scope="module")
def acav():
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


def _form(*a, **kw):
    from acav100m_amd.subset_selection.measures.batch import draw_form
    return draw_form(*a, **kw)


@pytest.mark.parametrize("L,B", [(50, 20), (21, 20), (20, 20), (1000, 100)])
def test_prefix_of_randperm(acav, L, B):
    from acav100m_amd.rng import Generator
    cand = np.random.RandomState(L).permutation(10 * L)[:L].astype(np.int64)
    g1, g2, g3 = Generator(123 + L), Generator(123 + L), Generator(123 + L)
    want = cand[g1.randperm(L)][:B]
    r = cand.copy()
    got = R.draw_batch(r, 0, B, g2.u32)
    assert np.array_equal(got, want)
    assert sorted(r.tolist()) == sorted(cand.tolist())  # still the same set
    for _ in range(B):  # the second generator has consumed exactly B words
        g3.u32()
    (mt2, i2), (mt3, i3) = g2.get_state(), g3.get_state()
    assert i2 == i3 and np.array_equal(mt2, mt3)


def test_form_iterations_draws_and_launches(acav, monkeypatch):
    monkeypatch.delenv("ACAV_DRAW_GROUP", raising=False)
    f = _form([10 ** 6], [2 * 10 ** 5], 20, 4, True)
    G = f['group_max']
    assert f['code'] == 0 and f['refusal'] == 0 and f['group'] == G and G >= 1
    assert f['iters'] == [50000] and f['draws'] == [50000 * 20] and f['iters_max'] == 50000
    assert f['launches'] == -(-50000 // G) and f['step'] == 4 and f['wide'] == 0 and f['threads'] == 256
    # exactly G iterations: one launch; one more: two
    assert _form([10 ** 7], [G * 4], 20, 4, True)['launches'] == 1
    assert _form([10 ** 7], [G * 4 + 1], 20, 4, True)['launches'] == 2
    # several chunks: per-chunk plans, the longest decides the launches; max_iters caps every chunk
    f = _form([5000, 700, 90000], [1000, 101, 30], 20, 4, True)
    assert f['iters'] == [250, 26, 8] and f['draws'] == [5000, 520, 160] and f['iters_max'] == 250 and f['launches'] == 1
    assert _form([5000, 700], [1000, 101], 20, 4, True, max_iters=3)['iters'] == [3, 3]
    assert _form([5000], [1000], 20, 4, True, max_iters=0)['launches'] == 0
    # no keep: the window start moves by B
    f = _form([5000], [400], 20, 4, False)
    assert f['step'] == 20 and f['iters'] == [100] and f['draws'] == [2000]
    # wide from B = 65 on; the dynamic LDS holds the selection's and five ints per batch position behind it
    f64, f65 = _form([5000], [100], 64, 4, True), _form([5000], [100], 65, 4, True)
    assert f64['wide'] == 0 and f65['wide'] == 1
    for f, B in ((f64, 64), (f65, 65)):
        assert f['lds'] == (f['sel_lds'] + 15) // 16 * 16 + 20 * B
    monkeypatch.setenv("ACAV_DRAW_GROUP", "7")
    f = _form([10 ** 6], [400], 20, 4, True)
    assert f['group'] == 7 and f['group_max'] == G and f['launches'] == -(-100 // 7)
    monkeypatch.setenv("ACAV_DRAW_GROUP", str(10 * G))  # the variable lowers the constant, it does not raise it
    assert _form([10 ** 6], [400], 20, 4, True)['group'] == G
    monkeypatch.setenv("ACAV_DRAW_GROUP", "0")
    assert _form([10 ** 6], [400], 20, 4, True)['group'] == G


@pytest.mark.parametrize("keep", [True, False])
def test_form_short_list_boundary(acav, keep, monkeypatch):
    monkeypatch.delenv("ACAV_DRAW_GROUP", raising=False)
    B, k, iters = 20, 4, 6
    step = k if keep else B
    L_ok = B + (iters - 1) * step  # the last iteration starts at L == B
    f = _form([L_ok], [iters * k], B, k, keep)
    assert f['code'] == 0 and f['iters'] == [iters]
    assert R.plan(L_ok, iters * k, B, k, keep) == (iters, iters * B)
    f = _form([L_ok - 1], [iters * k], B, k, keep)  # ... at L == B - 1: refused
    assert f['code'] == -5 and f['refusal'] == 2 and f['chunk'] == 0 and f['left'] == B - 1
    assert f['iters'] == [0] and f['launches'] == 0
    assert R.plan(L_ok - 1, iters * k, B, k, keep) == ('short', B - 1)
    # one iteration fewer asked for: the shorter list passes
    assert _form([L_ok - 1], [(iters - 1) * k], B, k, keep)['code'] == 0
    assert _form([L_ok - 1], [iters * k], B, k, keep, max_iters=iters - 1)['code'] == 0
    # the refusal names the first short chunk
    f = _form([1000, L_ok - 1, 5], [iters * k] * 3, B, k, keep)
    assert f['code'] == -5 and f['chunk'] == 1 and f['left'] == B - 1


def test_form_limits(acav):
    assert _form([5000], [100], 1024, 1024, False)['code'] == 0  # the largest batch, every position committed
    assert _form([5000], [100], 1, 1, True)['code'] == 0
    assert _form([5000], [100], 1024, 256, True, pmax=8, dmax=5)['code'] == 0
    for bad in (dict(B=1025, k=4), dict(B=0, k=0), dict(B=20, k=21), dict(B=20, k=0), dict(B=1024, k=4, pmax=9),
                dict(B=100, k=25, pmax=82), dict(B=20, k=4, dmax=0)):
        kw = dict(pmax=1, dmax=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            _form([5000], [100], kw.pop('B'), kw.pop('k'), True, **kw)
    with pytest.raises(ValueError):
        _form([2 ** 31], [100], 20, 4, True)  # lists of 2^31 rows or more
    assert _form([2 ** 31 - 1], [100], 20, 4, True)['code'] == 0  # no 16 Mi cliff: the plan does not depend on L
    with pytest.raises(ValueError):
        _form([0], [100], 20, 4, True)
    # label rows that do not fit beside the wide selection: refused as the permutation loop refuses them
    f = _form([5000], [100], 1024, 256, True, pmax=8, dmax=30)
    assert f['code'] == -1 and f['refusal'] == 3


def test_check_sampler():
    from acav100m_amd.subset_selection.run_greedy import batch_sampler, check_sampler
    assert check_sampler('batch_mi', None) == 'permutation'
    assert check_sampler('batch_mi', 'permutation') == 'permutation'
    assert check_sampler('batch_mi', 'draw') == 'draw'
    assert check_sampler('mi', 'permutation') == 'permutation' and check_sampler('contrastive', None) == 'permutation'
    for name in ('mi', 'mem_mi', 'ami', 'contrastive', 'pca', 'fm'):
        with pytest.raises(ValueError, match="batch_mi"):
            check_sampler(name, 'draw')
    for bad in ('Draw', 'shuffle', '', 1, True):
        with pytest.raises(ValueError, match="batch.sampler"):
            check_sampler('batch_mi', bad)
    from acav100m_amd.config import SUBSET_DEFAULTS, merge
    assert batch_sampler(merge(SUBSET_DEFAULTS, {})) is None
    assert batch_sampler(merge(SUBSET_DEFAULTS, {'batch.sampler': 'draw'})) == 'draw'
    assert merge(SUBSET_DEFAULTS, {'batch.sampler': 'draw'}).batch.batch_size == 20


def test_cli_refuses_draw_for_other_measures_before_any_device_work(tmp_path):
    from acav100m_amd.subset_selection.cli import check_run, get_args
    args = get_args(measure_name='mi', **{'batch.sampler': 'draw'})
    with pytest.raises(ValueError, match="batch_mi"):
        check_run(args)
    check_run(get_args(measure_name='batch_mi', **{'batch.sampler': 'draw'}))
    with pytest.raises(ValueError, match="batch.sampler"):
        check_run(get_args(**{'batch.sampler': 'nope'}))


def test_measure_refuses_unknown_sampler():
    from acav100m_amd.subset_selection.measures.batch import EfficientBatchMI
    with pytest.raises(ValueError, match="sampler"):
        EfficientBatchMI(np.zeros((4, 2), np.int64), ncentroids=2, sampler='nope')
    assert EfficientBatchMI(np.zeros((4, 2), np.int64), ncentroids=2).sampler == 'permutation'


def test_shrink_rule_by_hand():
    # window of B = 4 at lo = 2 of an 8-element array; positions 1 and 3 of the batch are committed (in that pick order)
    r = np.array([90, 91, 10, 11, 12, 13, 70, 71], np.int64)
    lo = R.shrink(r, 2, 4, [3, 1], True)
    assert lo == 4 and r[4:6].tolist() == [10, 12]  # the unselected, in batch order, at r[lo + k .. lo + B)
    assert r[:2].tolist() == [90, 91] and r[6:].tolist() == [70, 71]  # nothing outside the window moved
    r = np.array([90, 91, 10, 11, 12, 13, 70, 71], np.int64)
    assert R.shrink(r, 2, 4, [3, 1], False) == 6 and r.tolist() == [90, 91, 10, 11, 12, 13, 70, 71]
    r = np.array([90, 91, 10, 11, 12, 13, 70, 71], np.int64)
    assert R.shrink(r, 2, 4, [2, 0, 3, 1], True) == 6  # B == k: nothing is left to keep
    # the draw on the same array with a scripted generator: the swaps are sequential and a later step sees the earlier ones
    r = np.array([90, 91, 10, 11, 12, 13, 70, 71], np.int64)
    words = iter([5, 4, 0, 2])  # L = 6: z = 5 % 6, 4 % 5, 0 % 4, 2 % 3  ->  targets 5, 5, 2, 5 (window-relative)
    batch = R.draw_batch(r, 2, 4, lambda: next(words))
    assert batch.tolist() == [71, 10, 12, 11] and r.tolist() == [90, 91, 71, 10, 12, 11, 70, 13]
    assert R.rank_batch([0.5, float('nan'), 0.7, 0.5], 3).tolist() == [2, 0, 3]
