"""loo_predictive_host, the executable definition of loo_predictive(), without a GPU: float64 against
longdouble on every case of tests/loo_predictive_cases.py within its cap (1e-10), an independent plain implementation on the
tie-free cases, ties (repeated rows, the run that straddles the boundary, permutations of the draws), unsmoothed tails, the sum of
the weights against loo_host, the exact leave-one-out predictive of a conjugate regression, the C-ABI names, the refusals and the
result object."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import loo_predictive_cases as Q
import loo_cases as Lc
import waic_cases as W

LD = Q.LD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", Q.NAMES)
def test_float64_meets_the_cap_on_every_case(name):
    import fmcmc_amd as F
    case = Q.get_case(name)
    truth = Q.truth_of(case)                                         # (asserts the precondition)
    got = F.loo_predictive_host(case.model, case.draws)
    Q.assert_matches(got.point, truth, name)
    assert got.bad_points == 0 and truth.bad_points == 0 and got.bad_draws == 0
    gauss = case.family == "linreg"
    assert np.isnan(got.pit).all() != gauss
    if gauss:
        assert ((got.pit >= 0) & (got.pit <= 1)).all() and (got.sd > 0).all()
    else:
        assert ((got.mean > 0) & (got.mean < 1)).all()


def plain(case, dtype=LD):
    """An independent statement for draws without ties: a stable argsort of r, loo_gpdfit on the shifted tail, weights by rank."""
    from fmcmc_amd.summary import loo_gpdfit, loo_tail_len, waic_loglik
    from scipy.special import ndtr
    th = case.draws.astype(dtype)
    l = waic_loglik(case.model, th, dtype)
    S, n = l.shape
    M = loo_tail_len(S)
    X, y = case.model.X.astype(dtype), case.model.y.astype(dtype)
    eta = (th[:, :1] if case.ic else 0) + th[:, case.ic:case.ic + case.p] @ X.T
    out = np.zeros((n, 3), dtype=dtype)
    for i in range(n):
        r = -l[:, i]
        order = np.argsort(r, kind="stable")
        lw = r[order] - r[order[-1]]
        tl, cut = lw[S - M:], lw[S - M - 1]
        if M >= 5 and tl[-1] - tl[0] >= np.finfo(np.float64).eps / 100:
            k, sigma = loo_gpdfit(np.exp(tl) - np.exp(cut))
            if np.isfinite(k):
                p = (np.arange(1, M + 1).astype(dtype) - dtype(0.5)) / dtype(M)
                lw[S - M:] = np.minimum(np.log(np.exp(cut) + sigma * np.expm1(-k * np.log1p(-p)) / k), 0)
        w = np.empty(S, dtype=dtype)
        w[order] = np.exp(lw)
        w = w / w.sum()
        if case.family == "linreg":
            sg = th[:, -1]
            m = (w * eta[:, i]).sum()
            out[i] = (m, np.sqrt((w * ((eta[:, i] - m) ** 2 + sg * sg)).sum()),
                      (w * ndtr(((y[i] - eta[:, i]) / sg).astype(np.float64))).sum())
        else:
            q = (w / (1 + np.exp(-eta[:, i]))).sum()
            out[i] = (q, np.sqrt(q * (1 - q)), np.nan)
    return out


@pytest.mark.parametrize("name", Q.TIE_FREE)
def test_an_independent_plain_implementation_agrees(name):
    case = Q.get_case(name)
    truth, ref = Q.truth_of(case), plain(case)
    e = W.metric(np.nan_to_num(truth.point[:, :3].astype(LD)), np.nan_to_num(ref))
    print("%s: %.3g" % (name, float(e.max())))
    assert (e <= Q.CAP).all()
    assert np.array_equal(np.isnan(truth.point[:, 2]), np.isnan(ref[:, 2]))


@pytest.mark.parametrize("name", ["runs", "runs-logistic", "straddle"])
def test_ties_make_the_weights_a_function_of_the_value(name):
    import fmcmc_amd as F
    case = Q.get_case(name)
    truth = Q.truth_of(case)
    l = F.waic_loglik(case.model, case.draws, LD)
    S = l.shape[0]
    for i in range(case.n):
        r, w = -l[:, i], truth.weights[i]
        _v, inv = np.unique(r, return_inverse=True)
        first = np.zeros(inv.max() + 1, dtype=np.int64)
        first[inv[::-1]] = np.arange(S)[::-1]
        assert np.array_equal(w, w[first[inv]])                     # equal r, equal weight
    if name == "straddle":
        M = truth.loo.tail_len
        r = -l                                                      # [S][n]
        cut = truth.loo.pointwise[:, 5]
        c_all = (r == cut[None, :]).sum(axis=0)
        c_tail = (truth.loo.tail == cut[:, None]).sum(axis=1)
        assert (c_tail == M - case.n_far).all() and (c_all > c_tail + 1).all()
    # a permutation of the draws changes the order of the sums alone
    perm = np.random.default_rng(3).permutation(S)
    again = F.loo_predictive_host(case.model, case.draws[perm], LD)
    Q.assert_matches(again.point, truth, name + " permuted")
    assert (W.metric(again.weights[:, np.argsort(perm)], truth.weights) <= Q.CAP).all()


def test_an_unsmoothed_tail_gives_raw_ratio_weights():
    import fmcmc_amd as F
    for case in (Q.get_case("linreg-n17-p2-ic1-C1-N20"), Q.get_case("linreg-n17-p2-ic1-C1-N2")):
        t = Q.truth_of(case)
        l = F.waic_loglik(case.model, case.draws, LD)
        assert np.isinf(t.pareto_k).all()
        raw = np.exp(-l - (-l).max(axis=0)[None, :]).T
        assert (W.metric(t.weights, raw) <= 1e-18).all()
    # a constant tail: every draw the same row
    case = W.make_case("linreg", 5, 2, 1, 1, 40, seed=1)
    draws = np.repeat(case.draws[:1], 40, axis=0)
    t = F.loo_predictive_host(case.model, draws, LD)
    assert np.isinf(t.pareto_k).all() and np.array_equal(t.weights, np.ones_like(t.weights))
    one = F.predict_host(case.model, draws, None, (), "linpred", LD)
    assert (W.metric(t.mean, one.mean) <= 1e-18).all() and (W.metric(t.sd, np.full(5, draws[0, -1], dtype=LD)) <= 1e-15).all()


@pytest.mark.parametrize("name", ["linreg-n65-p3-ic1-C2-N33", "linreg-n17-p2-ic1-C1-N513", "runs", "straddle", "fallback",
                                  "logistic-n17-p2-ic0-C3-N200"])
def test_the_weights_sum_to_the_denominator_of_loo(name):
    import fmcmc_amd as F
    case = Q.get_case(name)
    t = Q.truth_of(case)
    lo = F.loo_host(case.model, case.draws, LD)
    l = F.waic_loglik(case.model, case.draws, LD)
    S, M = l.shape[0], lo.tail_len
    for i in range(case.n):
        r = np.sort(-l[:, i])
        R = lo.tail[i, -1]
        lw = np.concatenate([r[:S - M] - R, np.minimum(lo.smoothed[i], 0)])
        den, den2 = np.exp(lw).sum(), np.exp(2 * lw).sum()
        assert W.metric(den * den / den2, lo.n_eff[i]) <= 1e-15      # this den is the one behind loo's n_eff
        assert W.metric(t.sum_w[i], den) <= 1e-15
    assert np.array_equal(t.n_eff, lo.n_eff) and np.array_equal(t.pareto_k, lo.pareto_k)


def test_the_exact_leave_one_out_predictive_of_a_conjugate_regression():
    """S = 20000 independent draws from the exact posterior of a 30 x 2 regression under p(beta, sigma^2) ~ 1 / sigma^2.  The
    exact leave-one-out predictive of y_i is Student-t with n - 1 - p degrees of freedom, location y_i - e_i / (1 - h_ii) and
    squared scale s_(-i)^2 / (1 - h_ii).  An importance-sampling estimate of E[h] has standard error sd(h) / sqrt(n_eff):
    6 of those for the mean (sd(y) = sd_i) and for the pit (Phi lies in [0, 1], so its sd is at most 1/2)."""
    import fmcmc_amd as F
    from scipy.special import stdtr
    rng = np.random.default_rng(2024)
    n, p, S = 30, 2, 20000
    X = np.column_stack([np.ones(n), rng.uniform(-1.0, 1.0, n)])
    y = X @ np.array([0.5, 1.5]) + 0.8 * rng.standard_normal(n)
    XtXi = np.linalg.inv(X.T @ X)
    bhat = XtXi @ X.T @ y
    e = y - X @ bhat
    rss = float(e @ e)
    sigma2 = rss / rng.chisquare(n - p, S)
    beta = bhat[None, :] + np.sqrt(sigma2)[:, None] * (rng.standard_normal((S, p)) @ np.linalg.cholesky(XtXi).T)
    draws = np.column_stack([beta, np.sqrt(sigma2)])
    model = F.gaussian_linreg(X[:, 1:], y, intercept=True)
    got = F.loo_predictive_host(model, draws)
    assert (got.pareto_k < 0.7).all(), float(got.pareto_k.max())
    h = np.einsum("ij,jk,ik->i", X, XtXi, X)
    loc = y - e / (1 - h)
    nu = n - 1 - p
    scale = np.sqrt((rss - e * e / (1 - h)) / nu / (1 - h))
    cdf = stdtr(nu, (y - loc) / scale)
    z_mean = np.abs(got.mean - loc) / (got.sd / np.sqrt(got.n_eff))
    z_pit = np.abs(got.pit - cdf) / (0.5 / np.sqrt(got.n_eff))
    print("largest k %.3g, least n_eff %.0f, mean %.3g and pit %.3g standard errors off at most"
          % (got.pareto_k.max(), got.n_eff.min(), z_mean.max(), z_pit.max()))
    assert (z_mean <= 6).all() and (z_pit <= 6).all()
    # the sd of a Student-t with nu degrees of freedom, loosely: the weights' noise in a second moment is not bounded as above
    assert np.allclose(got.sd, scale * math.sqrt(nu / (nu - 2.0)), rtol=0.05)
    # the in-sample PIT is pulled towards 1/2, which is what the LOO form is there to undo
    insample = F.predictive_host(model, draws, probs=()).pit
    assert np.abs(got.pit - 0.5).mean() > np.abs(insample - 0.5).mean()


def test_the_abi_names():
    from fmcmc_amd import _abi as abi
    header = open(os.path.join(ROOT, "include", "fmcmc_amd.h")).read()
    L = abi.lib()
    for name in ("fmcmc_loo_predictive_work_len", "fmcmc_loo_predictive_dev"):
        assert name in abi.EXPORTS and name + "(" in header and hasattr(L, name), name


def test_the_refusals_of_the_c_entry_need_no_device():
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    X, y = np.zeros((3, 17)), np.zeros(17)
    xp, yp = X.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)           # (host pointers: never dereferenced)
    model = lambda fam=abi.FAM_GAUSSIAN_LINREG, p=3: abi.Model(fam, p, 17, xp, yp, 1, 0, 0.0)
    buf = C.c_void_p(8)
    call = lambda m=None, k=5, S=40, row0=0, N=33, Cn=1, work=buf, point=buf, total=buf: L.fmcmc_loo_predictive_dev(
        C.byref(m if m is not None else model()), buf, Cn, k, S, row0, N, work, point, None, total, None)
    assert call(k=4) == abi.ERR_ARG and "fmcmc_loo_predictive_dev" in abi.last_error() and "family has 5" in abi.last_error()
    assert call(N=1) == abi.ERR_ARG and "at least 2" in abi.last_error()
    assert call(row0=8) == abi.ERR_ARG and "outside" in abi.last_error()
    assert call(work=None) == abi.ERR_ARG and call(point=None) == abi.ERR_ARG and call(total=None) == abi.ERR_ARG
    assert "null argument" in abi.last_error()
    assert call(model(abi.FAM_IID_NORMAL, 0), k=2) == abi.ERR_UNSUPPORTED and "iid_normal" in abi.last_error()
    big = 29826162
    assert call(S=big, N=big) == abi.ERR_UNSUPPORTED and "16384" in abi.last_error()
    m = model()
    assert L.fmcmc_loo_predictive_work_len(C.byref(m), 1, 1) == 0 and L.fmcmc_loo_predictive_work_len(None, 1, 33) == 0
    assert L.fmcmc_loo_predictive_work_len(C.byref(model(abi.FAM_IID_NORMAL, 0)), 1, 33) == 0
    base, mine = L.fmcmc_loo_work_len(C.byref(m), 1, 2, 33), L.fmcmc_loo_predictive_work_len(C.byref(m), 2, 33)
    M = L.fmcmc_loo_tail_len(66)
    assert mine == base + 17 * (3 * M + 8) + 2 * 66 + 10 * 17 * abi.lib().fmcmc_waic_parts(2, 33, 17)
    lg = model(abi.FAM_LOGISTIC)
    assert L.fmcmc_loo_predictive_work_len(C.byref(lg), 2, 33) == L.fmcmc_loo_work_len(C.byref(lg), 1, 2, 33) + 17 * (3 * M + 8) \
        + 10 * 17 * abi.lib().fmcmc_waic_parts(2, 33, 17)


def test_the_refusals_of_the_python_entries():
    import fmcmc_amd as F
    case = Q.get_case("linreg-n17-p2-ic1-C1-N35")
    pw = F.pointwise_fun(lambda th: th[:, :1].repeat(1, 4), 4, 3)
    for entry in (lambda m: F.loo_predictive(None, m), lambda m: F.loo_predictive_host(m, case.draws)):
        with pytest.raises(TypeError, match="says nothing of the mean or the distribution of an observation"):
            entry(pw)
        with pytest.raises(TypeError, match="a BatchedFun says nothing"):
            entry(F.batched_fun(lambda th: th.sum(dim=1), 3))
        with pytest.raises(ValueError, match="iid_normal has no covariates to predict at"):
            entry(F.iid_normal(np.zeros(5)))
        with pytest.raises(TypeError, match="needs a gaussian_linreg or logistic object; got a"):
            entry(object())
    batch = F.McmcBatch.__new__(F.McmcBatch)
    with pytest.raises(TypeError, match=r"loo_predictive\(ans\[d\], models\[d\]\) per dataset"):
        F.loo_predictive(batch, case.model)
    with pytest.raises(ValueError, match="one shape"):
        F.loo_predictive_host_matrix(np.zeros((5, 2)), np.zeros((5, 3)))
    with pytest.raises(ValueError, match=r"sigma must be \[5\]"):
        F.loo_predictive_host_matrix(np.zeros((5, 2)), np.zeros((5, 2)), np.ones(4))


def test_the_result_object():
    import fmcmc_amd as F
    y = np.array([1.0, 2.0, 4.0, 3.0])
    point = np.array([[1.5, 1.0, 0.30, 0.1, 50.0, -1.0], [2.0, 1.0, 0.50, 0.2, 60.0, -1.1],
                      [3.0, 1.0, 0.96, 0.9, 9.0, -2.5], [3.5, 1.0, 0.04, 0.3, 40.0, -1.2]])
    loo_point = np.column_stack([point[:, 5], np.full(4, 0.1), point[:, 5] + 0.1, point[:, 3], point[:, 4], np.ones(4)])
    total = np.array([-5.8, 0.4, -5.4, 11.6, 0.7, 0.1, 0.6, 1, 0, 0.9, 0, 0, 0.0])
    r = F.LooPredictiveResult(point, loo_point, total, 400, y, "gaussian_linreg")
    assert np.array_equal(r.residuals, y - point[:, 0]) and r.nobs == 4 and r.ndraws == 400 and r.bad_points == 0
    assert isinstance(r.loo, F.LooResult) and r.loo.n_k_bad == 1 and np.array_equal(r.pareto_k, r.loo.pareto_k)
    assert r.coverage(0.9) == 0.5 and r.coverage(0.5) == 0.5 and r.coverage(0.95) == 1.0
    counts, edges = r.pit_hist(4)
    assert counts.tolist() == [1, 1, 1, 1] and edges.tolist() == [0.0, 0.25, 0.5, 0.75, 1.0]
    m = r.metrics()
    e = y - point[:, 0]
    assert m["rmse"] == float(np.sqrt((e * e).mean())) and m["mae"] == float(np.abs(e).mean())
    assert m["r2"] == float(1 - (e * e).sum() / ((y - y.mean()) ** 2).sum())
    s = str(r)
    assert "Leave-one-out predictive checks of 4 observations from 400 draws" in s and "rmse" in s and "coverage 90%" in s
    assert "1 (25.0%) Pareto k estimates above" in s and "LooPredictiveResult gaussian_linreg n=4" in repr(r)
    yb = np.array([1.0, 0.0, 1.0, 0.0])
    pb = point.copy()
    pb[:, 0], pb[:, 2] = [0.9, 0.2, 0.4, 0.1], np.nan
    total[7] = 0
    b = F.LooPredictiveResult(pb, loo_point, total, 400, yb, "logistic")
    assert b.metrics() == dict(brier=float(((yb - pb[:, 0]) ** 2).mean()), accuracy=0.75)
    assert "brier" in str(b) and "All Pareto k estimates are good" in str(b)
    with pytest.raises(ValueError, match="needs the PIT"):
        b.coverage(0.9)
    with pytest.raises(ValueError, match="needs the PIT"):
        b.pit_hist()
    with pytest.raises(ValueError, match="strictly inside"):
        r.coverage(1.0)
