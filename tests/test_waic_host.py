"""waic_host / waic_compare / WaicResult on the CPU, and the a-priori bound the device is held to (tests/waic_cases.py): float64
waic_host is inside the bound on every case of the host grid, a float32 evaluation and a wrong divisor are outside it, and the bound
itself stays below the cap of 1e-12."""
import numpy as np
import pytest

import waic_cases as W

LD = np.longdouble
TOTALS = ("elpd_waic", "p_waic", "lppd", "waic", "se_elpd", "se_p", "se_lppd")


def totals(r):
    return [getattr(r, f) for f in TOTALS]


@pytest.fixture(scope="module")
def grid():
    """every case of the host grid with its bound, computed once"""
    out = []
    for i, spec in enumerate(W.HOST_CASES):
        case = W.make_case(*spec, seed=100 + i)
        out.append((case, W.waic_bound(case)))
    return out


def test_the_public_names():
    import fmcmc_amd as F
    for name in ("waic", "waic_batch", "waic_compare", "waic_host", "WaicResult", "WaicBatch"):
        assert name in F.__all__ and hasattr(F, name), name
    assert hasattr(F.DeviceChains, "waic") and hasattr(F.McmcBatch, "waic")


def test_the_bound_stays_below_the_cap(grid):
    worst = 0.0
    for case, b in grid:
        rp, rt = W.relative_bound(b)
        top = max(float(rp.max()), float(np.nanmax(rt)))
        worst = max(worst, top)
        assert top <= W.CAP, (case.name, top)
    print("largest bound of the host grid: %.3g" % worst)


def test_float64_is_inside_the_bound_and_float32_outside(grid):
    import fmcmc_amd as F
    for case, b in grid:
        h = F.waic_host(case.model, case.draws)
        W.assert_within(h.pointwise, totals(h), b, case.name)
        assert (h.n_high, h.bad_draws, h.bad_points) == (b.truth.n_high, 0, 0) or case.n > 1
        f = F.waic_host(case.model, case.draws, np.float32)
        ep, et = W.metric(f.pointwise, b.truth.pointwise), W.metric(totals(f)[:4], W.truth_total(b.truth)[:4])
        rp, rt = W.relative_bound(b)
        assert (ep[:, :3] > rp[:, :3]).any(axis=0).all() and (et[:3] > rt[:3]).all(), case.name
        if case.n >= 15:
            assert (ep > rp).any(axis=1).all(), case.name        # every observation


def test_a_wrong_divisor_is_outside_the_bound(grid):
    for case, b in grid:
        S = case.C * case.N
        wrong = b.truth.pointwise.copy()
        wrong[:, 1] *= LD(S - 1) / LD(S)
        wrong[:, 0] = wrong[:, 2] - wrong[:, 1]
        rp, _rt = W.relative_bound(b)
        ep = W.metric(wrong, b.truth.pointwise)
        big = b.truth.pointwise[:, 1] > 1e-6
        assert big.any() and (ep[big, 1] > rp[big, 1]).all(), case.name


def test_equal_draws_have_no_variance():
    import fmcmc_amd as F
    for fam in ("linreg", "logistic", "iid"):
        case = W.make_case(fam, 17, 0 if fam == "iid" else 3, 1, 1, 33, seed=1)
        h = F.waic_host(case.model, np.repeat(case.draws[:1], 50, axis=0))
        assert (h.pointwise[:, 1] == 0.0).all() and np.array_equal(h.pointwise[:, 2], h.pointwise[:, 3]) and h.n_high == 0


def test_the_definition_by_hand():
    import fmcmc_amd as F
    rng = np.random.default_rng(0)
    X, y = rng.uniform(-2, 2, (6, 2)), rng.standard_normal(6)
    m = F.gaussian_linreg(X, y)
    th = np.array([0.1, 0.5, -0.3, 1.2]) + 0.1 * rng.standard_normal((7, 4))
    l = np.array([[-np.log(t[3]) - 0.5 * np.log(2 * np.pi) - 0.5 * (y[i] - t[0] - X[i] @ t[1:3]) ** 2 / t[3] ** 2 for i in range(6)]
                  for t in th])
    h = F.waic_host(m, th)
    assert np.allclose(h.pointwise[:, 2], np.log(np.exp(l).mean(axis=0)), rtol=1e-13)
    assert np.allclose(h.pointwise[:, 1], l.var(axis=0, ddof=1), rtol=1e-12) and np.allclose(h.pointwise[:, 3], l.mean(axis=0))
    assert np.isclose(h.waic, -2 * (h.lppd - h.p_waic)) and np.isclose(h.se_elpd, np.sqrt(6 * h.pointwise[:, 0].var(ddof=1)))
    assert sum(m(t) for t in th) == pytest.approx(l.sum(), rel=1e-12)        # the families' own closed form
    yb = (y > 0).astype(float)
    ml = F.logistic(X, yb, prior_div=8.0)
    tb = th[:, 1:3]
    lb = np.array([[np.log(1 / (1 + np.exp(-(X[i] @ t))) if yb[i] else 1 - 1 / (1 + np.exp(-(X[i] @ t)))) for i in range(6)]
                   for t in tb])
    assert np.allclose(F.waic_host(ml, tb).pointwise[:, 3], lb.mean(axis=0), rtol=1e-13)           # no prior term
    bad = th.copy()
    bad[2, 3], bad[5, 0] = -1.0, np.nan
    assert F.waic_host(m, bad).bad_draws == 2


def test_waic_compare():
    import fmcmc_amd as F
    from types import SimpleNamespace
    rng = np.random.default_rng(2)
    a, b = (SimpleNamespace(pointwise=rng.standard_normal((9, 4))) for _ in range(2))
    d = a.pointwise[:, 0] - b.pointwise[:, 0]
    c = F.waic_compare(a, b)
    assert c.elpd_diff == pytest.approx(d.sum(), rel=1e-14) and c.se_diff == pytest.approx(np.sqrt(9 * d.var(ddof=1)), rel=1e-14)
    r = F.waic_compare(b, a)
    assert r.elpd_diff == -c.elpd_diff and r.se_diff == c.se_diff
    A, B = (SimpleNamespace(pointwise=rng.standard_normal((3, 9, 4))) for _ in range(2))
    cb = F.waic_compare(A, B)
    assert cb.elpd_diff.shape == (3,) and cb.se_diff.shape == (3,)
    one = F.waic_compare(SimpleNamespace(pointwise=A.pointwise[1]), SimpleNamespace(pointwise=B.pointwise[1]))
    assert cb.elpd_diff[1] == one.elpd_diff and cb.se_diff[1] == one.se_diff
    with pytest.raises(ValueError, match="different numbers of observations"):
        F.waic_compare(a, SimpleNamespace(pointwise=np.zeros((8, 4))))
    with pytest.raises(ValueError):
        F.waic_compare(a, A)


def test_the_printed_layout():
    import fmcmc_amd as F
    point = np.zeros((262, 4))
    r = F.WaicResult(point, [-5457.44, 269.91, -5187.5, 10914.88, 692.21, 76.42, 650.0, 45, 0, 0], 4000)
    lines = str(r).split("\n")
    assert lines[1] == "Computed from 4000 by 262 log-likelihood matrix"
    assert lines[3].split() == ["Estimate", "SE"]
    assert [ln.split() for ln in lines[4:7]] == [["elpd_waic", "-5457.4", "692.2"], ["p_waic", "269.9", "76.4"],
                                                 ["waic", "10914.9", "1384.4"]]
    assert lines[8] == "45 (17.2%) p_waic estimates greater than 0.4. We recommend trying loo instead."
    quiet = F.WaicResult(point, [-1.0, 0.1, -0.9, 2.0, 0.1, 0.1, 0.1, 0, 0, 0], 10)
    assert "p_waic estimates greater" not in str(quiet) and repr(quiet).startswith("<WaicResult")
    assert r.se_waic == 2 * r.se_elpd and r.n_high == 45 and r.nobs == 262 and r.ndraws == 4000


def test_the_refusals():
    import fmcmc_amd as F
    case = W.make_case("linreg", 17, 2, 1, 1, 33, seed=4)
    fun = F.batched_fun(lambda th: th.sum(dim=1), 4)
    with pytest.raises(TypeError, match="no pointwise form"):
        F.waic_host(fun, case.draws)
    with pytest.raises(TypeError, match="no pointwise form"):
        F.waic(None, fun)
    with pytest.raises(ValueError, match=r"\[S\]\[4\]"):
        F.waic_host(case.model, case.draws[:, :3])
    with pytest.raises(ValueError, match="at least 2 draws"):
        F.waic_host(case.model, case.draws[:1])


def test_the_split_of_the_draws():
    from fmcmc_amd.summary import waic_parts
    assert waic_parts(1, 512, 17) == (32, 1) and waic_parts(1, 513, 17) == (32, 2) and waic_parts(3, 513, 17) == (32, 4)
    assert waic_parts(1024, 10000, 10000) == (10000, 64) and waic_parts(1024, 10000, 100) == (2500, 256)
    assert waic_parts(4, 2000, 1000) == (32, 16)
    lanes, P = W._lanes(3, 513, 17)
    assert P == 4 and sorted(np.concatenate([i for g in lanes for i in g]).tolist()) == list(range(3 * 513))
