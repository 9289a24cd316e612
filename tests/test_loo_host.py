"""loo_host, the plain numpy restatement of PSIS-LOO, without a GPU: float64 against longdouble on the host
grid of tests/waic_cases.py, the generalised-Pareto fit on exact quantiles, the cases without smoothing, and loo_compare.

A numpy prototype of the definition gave, over eight shapes of the grid (S 33 ... 5000, p up to 62, all three families), at most
1.5e-15 (elpd), 1.3e-14 (k) and 1.7e-15 (n_eff) between float64 and longdouble in the metric |got - truth| / max(1, |truth|)."""
import numpy as np
import pytest

import fmcmc_amd as F
from fmcmc_amd.summary import loo_gpdfit, loo_k_threshold, loo_tail_len, waic_loglik

import loo_cases as Lc
import waic_cases as W

LD = np.longdouble


def test_the_tail_length_in_integers():
    assert [loo_tail_len(S) for S in (2, 20, 21, 25, 224, 225, 226, 120003, 1024 * 10 ** 4)] == [1, 4, 5, 5, 45, 45, 46, 1040, 9600]
    for S in (3, 7, 99, 1000, 4999, 5000, 10 ** 6 + 1):
        assert loo_tail_len(S) == int(np.ceil(min(LD(S) / 5, 3 * np.sqrt(LD(S)))))
    assert loo_k_threshold(1000) == pytest.approx(1 - 1 / 3) and loo_k_threshold(10 ** 7) == 0.7


@pytest.mark.parametrize("spec", W.HOST_CASES, ids=lambda s: "%s-n%d-p%d-ic%d-C%d-N%d" % s)
def test_float64_against_longdouble(spec):
    case = W.make_case(*spec, seed=300 + W.HOST_CASES.index(spec))
    truth = F.loo_host(case.model, case.draws, LD)
    got = F.loo_host(case.model, case.draws, np.float64)
    assert got.pointwise.dtype == np.float64 and truth.pointwise.dtype == LD and got.tail_len == loo_tail_len(case.C * case.N)
    emax = Lc.emax_of(case)
    total = [getattr(got, f) for f in Lc.TOTALS] + [got.n_k_bad, got.n_k_very_bad, got.max_k]
    Lc.assert_matches(got.pointwise, got.tail, total, truth, emax, case.name)
    assert got.bad_draws == 0 and got.bad_points == 0


@pytest.mark.parametrize("k", [-0.3, 0.1, 0.3, 0.7, 1.2])
def test_the_fit_on_exact_quantiles(k):
    M, sigma = 1040, 2.0
    p = (np.arange(1, M + 1) - 0.5) / M
    x = sigma * np.expm1(-k * np.log1p(-p)) / k
    khat, shat = loo_gpdfit(x)
    print("k = %g: k error %.4g, sigma error %.4g" % (k, abs(khat - k), abs(shat - sigma)))
    assert abs(khat - k) <= 0.02 and abs(shat - sigma) <= 0.01


@pytest.mark.parametrize("S", [2, 20])
def test_a_tail_below_five_is_not_smoothed(S):
    case = W.make_case("linreg", 17, 2, 1, 1, S, seed=41)
    got = F.loo_host(case.model, case.draws, LD)
    assert got.tail_len < 5 and np.isinf(got.pareto_k).all() and got.n_k_bad == 17 and got.n_k_very_bad == 17
    l = waic_loglik(case.model, case.draws, LD)                      # [S][n]
    direct = -np.log(np.exp(-l).mean(axis=0))                        # raw importance sampling; the cap at the raw maximum binds nowhere
    assert (W.metric(got.pointwise[:, 0], direct) <= 1e-17 * 50).all()
    assert np.array_equal(got.tail, np.sort(-l.T, axis=1)[:, S - got.tail_len:])
    assert np.array_equal(got.pointwise[:, 5], np.sort(-l.T, axis=1)[:, S - got.tail_len - 1])


def test_equal_draws():
    case = W.make_case("logistic", 15, 2, 1, 2, 100, seed=42)
    draws = np.ascontiguousarray(np.broadcast_to(case.draws[:1], case.draws.shape))
    got = F.loo_host(case.model, draws, LD)
    l = waic_loglik(case.model, draws[:1], LD)[0]
    assert np.isinf(got.pareto_k).all()
    assert (W.metric(got.pointwise[:, 0], l) <= 1e-17).all() and (W.metric(got.pointwise[:, 2], l) <= 1e-17).all()
    assert (np.abs(got.pointwise[:, 1]) <= 1e-17).all() and abs(got.p_loo) <= 1e-16
    assert (W.metric(got.n_eff, 200) <= 1e-15).all()


def test_the_smoothed_tail_is_ordered_and_capped():
    case = W.make_case("linreg", 17, 5, 1, 5, 1000, seed=43)
    got = F.loo_host(case.model, case.draws, LD)
    fin = np.isfinite(got.pareto_k.astype(np.float64))
    assert fin.all()
    assert (np.diff(got.smoothed, axis=1) >= 0).all()
    # after the shift and the cap the weights of the tail are <= 0; the smoothed values themselves may pass 0 before the cap
    assert (np.minimum(got.smoothed, 0) <= 0).all() and (got.smoothed[:, 0] <= 0).all()
    assert (got.n_eff > 1).all() and (got.n_eff <= 5000).all()
    assert (got.pointwise[:, 0] <= got.pointwise[:, 2]).all()        # leaving an observation out never helps predicting it


def test_loo_compare_is_the_direct_computation():
    ca = W.make_case("linreg", 64, 3, 1, 2, 100, seed=44)
    a = F.loo_host(ca.model, ca.draws, LD)
    mb = F.gaussian_linreg(ca.model.X[:, :2], ca.model.y)
    b = F.loo_host(mb, np.ascontiguousarray(ca.draws[:, [0, 1, 2, 4]]), LD)
    got = F.loo_compare(a, b)
    d = a.pointwise[:, 0] - b.pointwise[:, 0]
    assert got.elpd_diff == float(d.sum())
    assert got.se_diff == pytest.approx(float(np.sqrt(64 * ((d - d.mean()) ** 2).sum() / 63)), rel=1e-15)
    assert F.loo_compare(b, a).elpd_diff == -got.elpd_diff
    with pytest.raises(ValueError):
        F.loo_compare(a, F.loo_host(F.gaussian_linreg(ca.model.X[:10], ca.model.y[:10]), ca.draws, LD))


def test_a_user_defined_model_is_refused():
    with pytest.raises(TypeError, match="no pointwise form"):
        F.loo_host(object(), np.zeros((4, 2)))


def test_the_exports_are_declared_and_the_plan_needs_no_device():
    import os
    from fmcmc_amd import _abi as abi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fmcmc_amd.h")).read()
    L = abi.lib()
    for name in ("fmcmc_loo_tail_len", "fmcmc_loo_plan", "fmcmc_loo_work_len", "fmcmc_loo_state_offset", "fmcmc_loo_dev",
                 "fmcmc_loo_groups_dev"):
        assert name in abi.EXPORTS and name + "(" in header and hasattr(L, name), name
    for name in ("loo", "loo_batch", "loo_compare", "loo_host", "loo_plan", "LooResult", "LooBatch"):
        assert name in F.__all__ and hasattr(F, name), name
    assert hasattr(F.DeviceChains, "loo") and hasattr(F.McmcBatch, "loo")
    assert L.fmcmc_abi_version() == 6
    for S in (2, 20, 21, 225, 226, 5000, 120003, 1024 * 10 ** 4, 29826161):
        assert L.fmcmc_loo_tail_len(S) == loo_tail_len(S)
    assert loo_tail_len(29826161) == 16384 and loo_tail_len(29826162) == 16385
    P = F.loo_plan(1024, 10000, 10000)                               # the headline shape
    assert (P.M, P.cap, P.target, P.ustride, P.forms) == (9600, 32768, 17736, 184, (5, 8193)) and P.rank >= 96
    small = F.loo_plan(3, 11, 7)                                     # every draw is in the subsample: the threshold is exact
    assert small.ustride == 1 and small.sub_rows == 33 and small.rank == small.target >= small.M + 1
    with pytest.raises(NotImplementedError):
        F.loo_plan(1, 29826162, 5)
    with pytest.raises(ValueError):
        F.loo_plan(1, 1, 5)
    r = F.LooResult(np.array([[-1.0, 0.2, -0.8, 0.3, 50.0, 2.0], [-2.0, 0.5, -1.5, np.inf, 3.0, 4.0]]),
                    [-3.0, 0.7, -2.3, 6.0, 1.0, 0.3, 0.7, 1, 1, np.inf, 0, 0], 100)
    assert r.tail_len == 20 and r.n_k_bad == 1 and "Pareto k diagnostic values" in str(r) and "elpd_loo" in str(r)
    assert [c for _l, c, _p, _n in r.k_table()] == [1, 0, 1]
