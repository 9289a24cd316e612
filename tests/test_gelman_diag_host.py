"""The host finish of gelman_diag() (fmcmc_amd/summary.py: gelman_diag_finish), a pure function of (partial, p, N, m,
confidence); no GPU.

Yardsticks:
 * the point estimates and mpsrf against the oracle's coda restatement (O.gelman), rtol 1e-9 as in tests/test_abi.py;
 * the upper confidence limit against `coda_gelman_ld` below: coda::gelman.diag restated from the published algorithm, from
   the raw chains, in longdouble.  (The reference never prints the upper limit, so no reference-owned output exists: the standing
   is that of heidel().)  The F quantile has no longdouble form: both sides take scipy.stats.f.ppf, each at its own degrees of
   freedom.  Bound 1e-9 relative: the degrees of freedom 2 w^2 / var.w come from the partial through sum s2^2 - m mean(s2)^2,
   which at these shapes (s2 within a few per cent of each other) loses three to four digits of 16; the quantile and the square
   root are smooth in it, which leaves at least three decades.
"""
import ctypes as C

import numpy as np
import pytest

from test_abi import abi, numpy_gelman_partial  # noqa: F401  (abi: the fixture that builds / loads the library)

LD = np.longdouble
FEW = "Convergence test with the Gelman is only available when `nchains` > 1L."


def chains(m, N, p, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m, N, p)) * (1 + rng.uniform(0, 1, (1, 1, p))) + rng.standard_normal((m, 1, p)) * 0.4 + 3.0


def coda_gelman_ld(x, confidence=0.95):
    """coda::gelman.diag(x, confidence, transform = FALSE, autoburnin = FALSE)$psrf for x [m][N][p], in longdouble."""
    from scipy import stats
    x = np.asarray(x).astype(LD)
    m, N, p = x.shape
    xbar = x.mean(1)                                             # [m][p]
    s2 = ((x - xbar[:, None, :]) ** 2).sum(1) / LD(N - 1)        # [m][p]
    cov = lambda a, b: ((a - a.mean(0)) * (b - b.mean(0))).sum(0) / LD(m - 1)
    w = s2.mean(0)
    b = N * cov(xbar, xbar)
    muhat = xbar.mean(0)
    var_w = cov(s2, s2) / m
    var_b = 2 * b * b / (m - 1)
    cov_wb = (LD(N) / m) * (cov(s2, xbar ** 2) - 2 * muhat * cov(s2, xbar))
    one_m = 1 + LD(1) / m
    V = (N - 1) * w / N + one_m * b / N
    var_V = ((N - 1) ** 2 * var_w + one_m ** 2 * var_b + 2 * (N - 1) * one_m * cov_wb) / LD(N) ** 2
    df_V = 2 * V * V / var_V
    df_adj = (df_V + 3) / (df_V + 1)
    q = (1 + confidence) / 2
    qf = np.array([stats.chi2.ppf(q, m - 1) / (m - 1) if vw == 0 else stats.f.ppf(q, m - 1, float(2 * ww * ww / vw))
                   for ww, vw in zip(w, var_w)]).astype(LD)
    fixed, random = LD(N - 1) / N, one_m * (b / w) / N
    return np.sqrt(df_adj * (fixed + random)), np.sqrt(df_adj * (fixed + qf * random))


def finish(x, confidence=0.95, split=None, **kw):
    from fmcmc_amd.summary import gelman_diag_finish
    m, N, p = x.shape
    center = x[0, 0].copy()
    split = m if split is None else split
    part = numpy_gelman_partial(x[:split], center)
    if split < m:                                                # partials of two shards add
        part = part + numpy_gelman_partial(x[split:], center)
    return gelman_diag_finish(part, p, N, confidence, **kw)


@pytest.mark.parametrize("m,N,p,confidence", [(2, 50, 1, 0.95), (3, 400, 3, 0.95), (6, 400, 6, 0.8), (4, 333, 70, 0.99),
                                              (5, 17, 2, 0.5)])
def test_psrf_against_the_oracle_and_the_longdouble_restatement(abi, O, m, N, p, confidence):
    x = chains(m, N, p, 1000 * m + p)
    g = finish(x, confidence, split=1 if m > 2 else None)
    opsrf, ompsrf = O.gelman(x)
    est, upper = coda_gelman_ld(x, confidence)
    assert g.psrf.shape == (p, 2) and g.confidence == confidence
    assert np.allclose(g.psrf[:, 0], opsrf, rtol=1e-9)
    err_est = np.abs(g.psrf[:, 0] - est) / est
    err_up = np.abs(g.psrf[:, 1] - upper) / upper
    print("m=%d N=%d p=%d: point est. %.2e, upper %.2e of the longdouble restatement" % (m, N, p, err_est.max(), err_up.max()))
    assert err_est.max() < 1e-9 and err_up.max() < 1e-9
    if p > 1:
        assert abs(g.mpsrf - ompsrf) < 1e-9 * ompsrf
    # the point estimates are fmcmc_gelman_finish's, to the bit
    part = numpy_gelman_partial(x[:1], x[0, 0]) + numpy_gelman_partial(x[1:], x[0, 0]) if m > 2 else numpy_gelman_partial(x, x[0, 0])
    psrf = np.empty(p); mps = C.c_double(); dp = C.POINTER(C.c_double)
    assert abi.lib().fmcmc_gelman_finish(part.ctypes.data_as(dp), p, N, psrf.ctypes.data_as(dp), C.byref(mps)) == abi.OK
    assert np.array_equal(psrf, g.psrf[:, 0])


def test_upper_limit_bounds_the_point_estimate_and_grows_with_confidence(abi):
    x = chains(4, 200, 5, 7)
    ups = [finish(x, c) for c in (0.5, 0.8, 0.95, 0.99)]
    for g in ups:                      # (qf((1 + c) / 2, m - 1, .) > 1 from c = 0.5 on for every m - 1 >= 1)
        assert np.all(g.psrf[:, 1] >= g.psrf[:, 0])
        assert np.array_equal(g.psrf[:, 0], ups[0].psrf[:, 0])
    for lo, hi in zip(ups, ups[1:]):
        assert np.all(hi.psrf[:, 1] > lo.psrf[:, 1])


def test_equal_chain_variances_take_the_infinite_df_quantile(abi):
    """var.w == 0: two chains that mirror each other have the same variance to the bit; scipy.stats.f.ppf(q, d, inf) is NaN,
    R's qf(q, d, Inf) is qchisq(q, d) / d (5.0238861873 at q = 0.975, d = 1)."""
    from scipy import stats
    assert abs(stats.chi2.ppf(0.975, 1) - 5.0238861873148) < 1e-9
    x = chains(1, 300, 3, 11) - 3.0 + 0.05
    x = np.concatenate([x, -x])
    part = numpy_gelman_partial(x, x[0, 0])
    p = 3
    s_s2, s_s2s2 = part[1 + p + 2 * p * p:][:p], part[1 + 2 * p + 2 * p * p:][:p]
    assert np.all(s_s2s2 - 2 * (s_s2 / 2) ** 2 == 0.0)          # the branch under test is the one taken
    g = finish(x)
    est, upper = coda_gelman_ld(x)
    assert np.all(np.isfinite(g.psrf))
    assert np.allclose(g.psrf[:, 0], est.astype(np.float64), rtol=1e-9)
    assert np.allclose(g.psrf[:, 1], upper.astype(np.float64), rtol=1e-9)
    assert np.all(g.psrf[:, 1] > g.psrf[:, 0])


def test_mpsrf_is_none_for_one_column_or_when_not_asked_for(abi):
    assert finish(chains(3, 100, 1, 1)).mpsrf is None
    g = finish(chains(3, 100, 4, 2), multivariate=False)
    assert g.mpsrf is None and g.psrf.shape == (4, 2)
    assert finish(chains(3, 100, 4, 2)).mpsrf > 0


def test_w_not_positive_definite(abi):
    x = chains(3, 100, 3, 5)
    x[:, :, 1] = 2.0                   # a constant column: W[1][1] = 0 and the Cholesky pivot is exactly 0
    with pytest.raises(ValueError, match="cannot compute: W is not positive definite"):
        finish(x)
    with np.errstate(all="ignore"):
        g = finish(x, multivariate=False)
    assert g.mpsrf is None and np.all(np.isfinite(g.psrf[[0, 2]]))


def test_printed_layout():
    from fmcmc_amd.summary import GelmanDiag
    g = GelmanDiag([[1.0012, 1.0049], [1.234, 1.5]], 1.0123, ["b0", "sigma"])
    assert str(g) == ("Potential scale reduction factors:\n"
                      "\n"
                      "      Point est. Upper C.I.\n"
                      "b0          1.00        1.0\n"
                      "sigma       1.23        1.5\n"
                      "\n"
                      "Multivariate psrf\n"
                      "\n"
                      "1.01\n")
    g = GelmanDiag([[1.0004, 1.0011], [1.0, 1.002]], None)
    assert str(g) == ("Potential scale reduction factors:\n"
                      "\n"
                      "     Point est. Upper C.I.\n"
                      "par1          1          1\n"
                      "par2          1          1\n")
    assert g.varnames == ["par1", "par2"] and g.mpsrf is None


def test_fewer_than_two_chains(abi):
    import fmcmc_amd as f
    from fmcmc_amd.summary import gelman_diag_finish
    x = chains(1, 50, 2, 3)
    with pytest.raises(ValueError) as e:
        gelman_diag_finish(numpy_gelman_partial(x, x[0, 0]), 2, 50)
    assert str(e.value) == FEW
    one = f.Mcmc(x[0], start=1, end=50, thin=1)
    for obj in (one, f.McmcList([one])):
        with pytest.raises(ValueError) as e:
            f.gelman_diag(obj)
        assert str(e.value) == FEW
