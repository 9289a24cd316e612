"""ppc_host, the fold it restates and fmcmc_ppc_elem_host on the CPU (fmcmc_amd/summary.py, csrc/diag_ppc.hpp): what makes the
cases of tests/ppc_cases.py tests (no element that may flip, few draws near T_obs), float64 against longdouble within the
tolerances the device is held to, the variates against the oracle, the refusals that need no device, and the statistical sanity of
the check itself on a conjugate regression."""
import ctypes as C

import numpy as np
import pytest

import fmcmc_amd as F
from fmcmc_amd import _abi as abi
from fmcmc_amd.summary import ppc_counts, ppc_fold, ppc_observed, ppc_variates

import ppc_cases as Q

LD = np.longdouble


@pytest.mark.parametrize("spec", Q.SHAPES, ids=lambda s: "%s-m%d-p%d-ic%d-C%d-N%d" % s)
def test_the_general_cases_are_tests_and_float64_is_within_the_tolerances(spec):
    """no element within the flip bound, at most S' / 100 draws near T_obs per statistic (both asserted by assert_general), and
    ppc_host(float64) within the tolerances of the device"""
    case, kw = Q.shape_case(spec)
    truth, got = Q.host(case, LD, **kw), Q.host(case, np.float64, **kw)
    S = case.C * case.N
    stats = got.stats.reshape(case.C, case.N, Q.NSTAT).transpose(0, 2, 1)
    total = np.concatenate([[S, 0], got.counts.ravel()]).astype(np.float64)
    Q.assert_general(case, stats, total, truth)
    if case.family == "logistic":                        # no flip: the same 0 / 1 values, folded alike
        assert np.array_equal(got.yrep, np.asarray(truth.yrep, dtype=np.float64))
        assert np.array_equal(got.counts[:4], truth.counts[:4])


@pytest.mark.parametrize("spec", Q.EXACT, ids=lambda s: "%s-m%d-p%d-C%d-N%d" % s)
def test_the_exact_cases_are_exact(spec):
    """every eta is an integer, so float64 and longdouble agree on it; no chisq pair is near unless its terms are the same, so the
    counts of the device can be held to equality"""
    case, kw = Q.exact_shape_case(spec)
    truth, got = Q.host(case, LD, **kw), Q.host(case, np.float64, **kw)
    assert np.array_equal(got.eta, np.round(got.eta)) and np.array_equal(got.eta, np.asarray(truth.eta, dtype=np.float64))
    assert len(truth.flips) == 0 and truth.near[4] == 0
    assert np.array_equal(got.counts, truth.counts)
    cols = [0, 4, 5] + ([1] if case.m > 1 else [])
    assert (Q.metric(got.stats[:, cols], truth.stats[:, cols]) <= Q.CAP).all()
    assert np.array_equal(got.stats[:, 2:4], np.asarray(truth.stats[:, 2:4], dtype=np.float64))


def test_the_fold_against_numpy():
    rng = np.random.default_rng(4)
    for n in (1, 2, 15, 16, 17, 33, 100):
        v = rng.standard_normal((7, n)) * 3 + 10
        a, b = rng.uniform(size=(7, n)), rng.uniform(size=(7, n))
        got = ppc_fold(v, a, b, LD)
        vl = v.astype(LD)
        want = [vl.mean(axis=1), vl.std(axis=1, ddof=1) if n > 1 else np.full(7, np.nan), vl.min(axis=1), vl.max(axis=1),
                a.astype(LD).sum(axis=1), b.astype(LD).sum(axis=1)]
        for j, w in enumerate(want):
            if n == 1 and j == 1:
                assert np.isnan(np.asarray(got[:, 1], dtype=np.float64)).all()
            else:
                assert (Q.metric(got[:, j], w) <= 1e-17).all(), (n, j)
        f64 = ppc_fold(v, a, b)
        assert np.array_equal(f64[:, 2:4], np.stack([v.min(axis=1), v.max(axis=1)], axis=1))
    v = np.array([[1.0, np.nan, 3.0] + [2.0] * 30])
    assert np.isnan(ppc_fold(v, v, v)[0, [0, 2, 3]]).all()


def test_the_counts():
    stats = np.array([[1.0, 1, 1, 1, 5, 4], [2.0, 1, 0, 3, 4, 4], [np.nan, 1, 1, 1, 1, np.inf], [3.0, 0, 1, 2, 7, 9]])
    got = ppc_counts(stats, np.array([2.0, 1.0, 1.0, np.nan]))
    assert got.tolist() == [[1, 1, 1], [0, 3, 0], [0, 3, 0], [0, 0, 4], [1, 1, 1]]


def test_observed_is_longdouble_rounded():
    m = F.gaussian_linreg(None, np.array([0.1, 0.2, 0.4]), intercept=True)
    y = np.array([0.1, 0.2, 0.4], dtype=LD)
    mean = y.sum() / 3
    assert ppc_observed(m).tolist() == [float(mean), float(np.sqrt(((y - mean) ** 2).sum() / 2)), 0.1, 0.4]
    assert np.isnan(ppc_observed(F.gaussian_linreg(None, np.array([1.5]), intercept=True))[1])


def test_the_variates_are_the_oracles(O):
    """variate = u for the logistic family, z = fmh_qnorm(u) for the Gaussian one, bit for bit fmcmc_oracle_detmath(3, u); y_rep =
    fma(sigma, z, eta) resp. u < expit(eta); lane i & 1 of block i >> 1 of the oracle's Philox"""
    n = 37
    y = np.zeros(n)
    lin, logit = F.gaussian_linreg(None, y, intercept=True), F.logistic(np.zeros((n, 0)), y, intercept=True)
    ids, chains = np.array([5, 2 ** 32 - 1, 77]), np.array([0, 9, 2 ** 32 - 1])
    u = ppc_variates(logit, chains, ids, seed=123456789012345)
    z = ppc_variates(lin, chains, ids, seed=123456789012345)
    want = np.empty_like(u)
    dp = C.POINTER(C.c_double)
    O.lib().fmcmc_oracle_detmath(3, np.ascontiguousarray(u).ctypes.data_as(dp), want.ctypes.data_as(dp), u.size)
    assert np.array_equal(Q.bits(z), Q.bits(want)) and ((u > 0) & (u < 1)).all()
    words = (C.c_uint32 * 4)()
    seed = 123456789012345
    for s in range(3):
        for i in (0, 1, 36):
            O.lib().fmcmc_oracle_philox(int(ids[s]), int(chains[s]), i >> 1, 5, seed & 0xffffffff, seed >> 32, words)
            hi, lo = (words[2], words[3]) if i & 1 else (words[0], words[1])
            assert u[s, i] == ((((hi << 32) | lo) >> 12) + 0.5) * 2.0 ** -52
    eta, yrep, var = np.linspace(-3, 3, n), np.empty(n), np.empty(n)
    L = abi.lib()
    assert L.fmcmc_ppc_elem_host(abi.FAM_GAUSSIAN_LINREG, seed, 9, 5, n, eta.ctypes.data, 2.0, yrep.ctypes.data, var.ctypes.data) == abi.OK
    assert np.array_equal(yrep, 2.0 * var + eta)                       # (2 z is exact: one rounding either way)
    assert L.fmcmc_ppc_elem_host(abi.FAM_LOGISTIC, seed, 9, 5, n, eta.ctypes.data, 1.0, yrep.ctypes.data, var.ctypes.data) == abi.OK
    assert np.array_equal(yrep, (var < 1 / (1 + np.exp(-eta))).astype(float))


def test_the_refusals_that_need_no_device():
    L = abi.lib()
    buf = np.zeros(4)
    a = lambda fam=abi.FAM_LOGISTIC, chain=0, id_=1: (fam, 1, chain, id_, 4, buf.ctypes.data, 1.0, buf.ctypes.data, buf.ctypes.data)
    assert L.fmcmc_ppc_elem_host(*a(fam=abi.FAM_IID_NORMAL)) == abi.ERR_UNSUPPORTED and "family" in abi.last_error()
    assert L.fmcmc_ppc_elem_host(*a(id_=2 ** 32)) == abi.ERR_UNSUPPORTED and "32 bits" in abi.last_error()
    assert L.fmcmc_ppc_elem_host(*a(chain=-1)) == abi.ERR_UNSUPPORTED
    y = np.zeros(5)
    good = abi.Model(abi.FAM_GAUSSIAN_LINREG, 0, 5, None, y.ctypes.data, 1, 0, 0.0)
    assert L.fmcmc_ppc_work_len(C.byref(good), 3, 1000) == 2 * 12 + 16
    assert L.fmcmc_ppc_work_len(C.byref(good), 1, 1) == 0 and "at least 2" in abi.last_error()
    assert L.fmcmc_ppc_work_len(C.byref(good), 0, 10) == 0 and L.fmcmc_ppc_work_len(None, 1, 10) == 0
    iid = abi.Model(abi.FAM_IID_NORMAL, 0, 5, None, y.ctypes.data, 1, 0, 0.0)
    assert L.fmcmc_ppc_work_len(C.byref(iid), 3, 10) == 0 and "iid_normal" in abi.last_error()


def test_the_models_that_are_refused():
    rng = np.random.default_rng(0)
    draws = rng.standard_normal((4, 2))
    with pytest.raises(ValueError, match="iid_normal"):
        F.ppc_host(F.iid_normal(np.zeros(5)), draws, np.zeros(4), np.arange(4))
    with pytest.raises(TypeError, match="regression families"):
        F.ppc_host(F.pointwise_fun(lambda th: th, 5, 2), draws, np.zeros(4), np.arange(4))
    with pytest.raises(TypeError, match="regression families"):
        F.ppc(None, F.batched_fun(lambda th: th, 2))
    with pytest.raises(NotImplementedError, match="32 bits"):
        F.ppc_host(F.gaussian_linreg(None, np.zeros(3)), np.ones((2, 2)), [0, 0], [1, 2 ** 32])


def test_the_selection_of_posterior_predict():
    c, r = F.posterior_predict_selection(3, 10, 5)
    assert c.tolist() == [0, 0, 1, 1, 2] and r.tolist() == [0, 6, 2, 8, 4]
    c, r = F.posterior_predict_selection(2, 3, 50)
    assert c.tolist() == [0, 0, 0, 1, 1, 1] and r.tolist() == [0, 1, 2, 0, 1, 2]
    with pytest.raises(ValueError):
        F.posterior_predict_selection(2, 3, 0)


def conjugate_draws(X, y, S, rng):
    """S draws (b0, beta, sigma) from the posterior of a regression with intercept under the flat prior p(beta, log sigma) = 1"""
    A = np.column_stack([np.ones(len(y)), X])
    n, k = A.shape
    G = np.linalg.inv(A.T @ A)
    bhat = G @ A.T @ y
    sse = ((y - A @ bhat) ** 2).sum()
    sigma = np.sqrt(sse / rng.chisquare(n - k, S))
    beta = bhat[None, :] + sigma[:, None] * (rng.standard_normal((S, k)) @ np.linalg.cholesky(G).T)
    return np.column_stack([beta, sigma])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_statistical_sanity_on_a_conjugate_regression(seed):
    """n = 64, p = 3, 2000 draws of the conjugate posterior of a well-specified regression, y_rep from the Philox stream: every
    p-value inside (0.02, 0.98).  The same data with one y moved by +8 sigma: p(max) < 0.05.  The other statistics are not
    asserted to move: mean, sd and chisq are fitted by the model (the outlier inflates the sigma of every draw with them)."""
    rng = np.random.default_rng(seed)
    n, S = 64, 2000
    X = rng.uniform(-2, 2, (n, 3))
    y = 0.5 + X @ [1.5, -1.0, 0.25] + 1.3 * rng.standard_normal(n)
    chains, ids = np.divmod(np.arange(S), 500)
    clean = F.ppc_host(F.gaussian_linreg(X, y, intercept=True), conjugate_draws(X, y, S, rng), chains, 1 + ids, seed=seed)
    print("clean p:", dict(zip(abi.PPC_STATS, clean.pvalue.round(3))))
    assert ((clean.pvalue > 0.02) & (clean.pvalue < 0.98)).all() and clean.bad_draws == 0
    assert np.array_equal(clean.pvalue, clean.p_gt)                   # (no ties in continuous data)
    y2 = y.copy()
    y2[int(np.argmax(y))] += 8 * 1.3                  # (the largest y: wherever the regression puts it, it is now the maximum)
    out = F.ppc_host(F.gaussian_linreg(X, y2, intercept=True), conjugate_draws(X, y2, S, rng), chains, 1 + ids, seed=seed)
    print("outlier p:", dict(zip(abi.PPC_STATS, out.pvalue.round(3))))
    assert out.pvalue[3] < 0.05
