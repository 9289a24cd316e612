"""fmh_pnorm_both (include/fmh_detmath.h) through its host build fmcmc_detmath_host(11 / 12, ...) against mpmath at 50 digits on the
grid of tests/predictive_cases.py: pnorm_grid.  The largest relative error found on the CPU build is FMH_PNORM_REL (DESIGN.md
§5.10); this test asserts twice that value, the margin for the doubles the grid does not visit, and the constant c of
csrc/diag_predictive.hpp budgets an evaluation with the same number.  A subnormal result cannot carry a relative accuracy: it
is held to 2 FMH_PNORM_REL of the truth plus one spacing of the subnormals (the one rounding of the last product onto their grid)."""
import numpy as np
import pytest

import predictive_cases as P
import importlib

SM = importlib.import_module("fmcmc_amd.summary")

mp = pytest.importorskip("mpmath")


@pytest.fixture(scope="module")
def grid():
    x = P.pnorm_grid()
    return x, P.detmath_host(11, x), P.detmath_host(12, x)


def test_both_tails_against_fifty_digits(grid):
    x, lower, upper = grid
    mp.mp.dps = 50
    sub = mp.mpf(2) ** -1074
    worst = 0.0
    fin = np.isfinite(x)
    for xv, lo, up in zip(x[fin], lower[fin], upper[fin]):
        for got, want in ((lo, mp.ncdf(mp.mpf(float(xv)))), (up, mp.ncdf(-mp.mpf(float(xv))))):
            err = abs(mp.mpf(float(got)) - want)
            if want >= mp.mpf(2.2250738585072014e-308):
                rel = float(err / want)
                if rel > worst:
                    worst, at = rel, float(xv)
            else:
                assert err <= 2 * SM.PNORM_REL * want + sub, (float(xv), float(got))
    print("largest relative error %.4g at x = %r (FMH_PNORM_REL = %.4g)" % (worst, at, SM.PNORM_REL))
    assert worst <= 2 * SM.PNORM_REL


def test_the_special_values(grid):
    x, lower, upper = grid
    at = lambda v: int(np.flatnonzero((x == v) | (np.isnan(x) & np.isnan(v)))[0])
    assert lower[at(np.inf)] == 1.0 and upper[at(np.inf)] == 0.0 and lower[at(-np.inf)] == 0.0 and upper[at(-np.inf)] == 1.0
    assert np.isnan(lower[at(np.nan)]) and np.isnan(upper[at(np.nan)])
    assert lower[at(0.0)] == 0.5 and upper[at(0.0)] == 0.5
    assert lower[at(-38.6)] == 0.0 and upper[at(-38.6)] == 1.0


def test_the_identities(grid):
    x, lower, upper = grid
    fin = ~np.isnan(x)
    assert np.array_equal(P.bits(lower[fin]), P.bits(P.detmath_host(12, -x[fin])))        # lower(x) == upper(-x), bit for bit
    assert (np.abs((lower[fin] + upper[fin]) - 1.0) <= 2 * P.EPS).all()


def test_monotone_over_neighbouring_doubles_at_the_range_breaks():
    for b in P.pnorm_breaks():
        x = [b]
        for _ in range(8):
            x = [np.nextafter(x[0], -np.inf)] + x + [np.nextafter(x[-1], np.inf)]
        lower, upper = P.detmath_host(11, np.asarray(x)), P.detmath_host(12, np.asarray(x))
        print("break %r: lower steps %s, upper steps %s" % (b, np.diff(lower).tolist(), np.diff(upper).tolist()))
        assert (np.diff(lower) >= 0).all() and (np.diff(upper) <= 0).all(), b
