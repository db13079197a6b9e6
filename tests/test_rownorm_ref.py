"""CPU: the numpy restatement of the row normalisation (tests/_rownorm_np.py) against independent arithmetic -- math.fsum for the
sum of squares, one float64 division and one rounding for the rows.

Bounds.  The squares are exact and non-negative, so every partial sum of the stated order is a sum of non-negative terms: a
value passes through at most ceil(d / 256) - 1 additions in its chain, 2 in the fold and 6 in the butterfly, each with a relative
error of at most u = 2^-53, and no cancellation amplifies them: |ss - exact| <= (ceil(d / 256) + 7) u ss to first order; the
test allows (ceil(d / 256) + 8) u.  A normalised entry differs from float32(x / sqrt(fsum)) by that relative error of ss (halved
by the root) plus the roundings of the root and the quotient, a few 2^-53, far below the fp32 spacing 2^-24: at most 1 fp32 ulp
where the exact quotient lies next to a rounding boundary."""
import math

import numpy as np
import pytest

from tests import _rownorm_np as R

WIDTHS = (1, 3, 63, 64, 65, 255, 256, 257, 1000, 1024, 2304)
SCALES = (1e-3, 1.0, 1e3)


def _rows(d, scale, n=6, seed=0):
    rs = np.random.RandomState(seed + d)
    return (rs.standard_normal((n, d)) * scale).astype(np.float32)


@pytest.mark.parametrize("d", WIDTHS)
def test_sumsq_against_fsum(d):
    for scale in SCALES:
        x = _rows(d, scale)
        got = R.sumsq(x)
        for i, row in enumerate(x):
            exact = math.fsum(float(v) * float(v) for v in row)
            bound = (-(-d // 256) + 8) * 2.0 ** -53
            err = abs(got[i] - exact) / exact
            assert err <= bound, (d, scale, i, err, bound)
        assert R.sumsq(x[0]) == got[0]  # one row alone: the same value


@pytest.mark.parametrize("d", WIDTHS)
def test_normalize_against_one_division(d):
    for scale in SCALES:
        x = _rows(d, scale, seed=100)
        y, zero = R.normalize(x)
        assert zero == 0 and y.dtype == np.float32
        for i, row in enumerate(x):
            norm = math.sqrt(math.fsum(float(v) * float(v) for v in row))
            want = np.float32(row.astype(np.float64) / norm)
            ulp = np.spacing(np.abs(want))
            assert (np.abs(y[i].astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (d, scale, i)
            n2 = math.fsum(float(v) * float(v) for v in y[i])
            assert abs(n2 - 1.0) <= 6e-7, (d, scale, i, n2)


def test_zero_rows_come_back_bit_identical_and_are_counted():
    x = _rows(65, 1.0, n=5, seed=7)
    x[0] = 0
    x[2] = 0
    x[2, ::2] = -0.0
    x[4] = -0.0
    before = x.copy()
    y, zero = R.normalize(x)
    assert zero == 3
    for i in (0, 2, 4):
        assert y[i].tobytes() == before[i].tobytes()
    assert np.signbit(y[2, ::2]).all() and not np.signbit(y[2, 1::2]).any()
    assert x.tobytes() == before.tobytes()  # the input is left alone
    for i in (1, 3):
        assert abs(float((y[i].astype(np.float64) ** 2).sum()) - 1.0) <= 6e-7


def test_extreme_magnitudes_stay_finite_and_unit():
    x = np.stack([np.full(300, 3e38, np.float32), np.full(300, 1e-45, np.float32)])
    y, zero = R.normalize(x)
    assert zero == 0 and np.isfinite(y).all()
    assert (np.abs((y.astype(np.float64) ** 2).sum(1) - 1.0) <= 6e-7).all()
    with pytest.raises(ValueError):
        R.normalize(np.array([[1.0, np.inf]], np.float32))
