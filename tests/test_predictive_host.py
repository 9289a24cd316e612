"""predictive_host (fmcmc_amd/summary.py), the executable definition of predictive(), in float64 against the truth and the
acceptance property of tests/predictive_cases.py on the five input families; every case finishes within the cap of passes on this
restatement, which is what makes the cap legitimate on the device; the bracket property at pass 0; the refusals of predictive()
and of the C entry that come before any device call."""
import ctypes as C
import warnings

import numpy as np
import pytest

import predictive_cases as P
import predict_cases as PC

LD = np.longdouble


@pytest.fixture(scope="module", params=P.FAMILIES)
def solved(request):
    import fmcmc_amd as F
    case = P.family_case(request.param)
    return case, F.predictive_host(case.model, case.draws, probs=P.PROBS, max_passes=P.MAX_PASSES)


def test_every_case_finishes_within_the_cap(solved):
    case, r = solved
    print("%s: passes %d .. %d per prob %s" % (case.name, r.passes.min(), r.passes.max(), r.passes.max(axis=0).tolist()))
    assert r.converged.all() and (r.passes >= 1).all() and (r.passes <= P.MAX_PASSES).all()
    assert r.quantiles.shape == (case.m, len(P.PROBS)) and r.ndraws == case.C * case.N and r.bad_draws == 0


def test_the_acceptance_property(solved):
    case, r = solved
    P.assert_accepted(case, r.quantiles, P.PROBS, P.SM.predictive_host_tol(r.ndraws, P.PROBS)[0], P.eta_error(case))
    assert (np.diff(r.quantiles, axis=1) >= 0).all()                                   # the probs ascend


def test_the_bracket_encloses_the_root_at_pass_zero(solved):
    case, r = solved
    pr = np.asarray(P.PROBS)
    Glo, Ghi = P.truth(case, r.lo0, P.PROBS)[0], P.truth(case, r.hi0, P.PROBS)[0]
    assert (Glo <= 0).all() and (Ghi >= 0).all(), (float(Glo.max()), float(Ghi.min()))
    assert (r.lo0 <= r.quantiles).all() and (r.quantiles <= r.hi0).all()
    assert pr.size == r.lo0.shape[1]


def test_equal_draws_give_the_closed_form():
    """(b): t = eta + sigma qnorm(p) within 4 ulp (P.closed_form_ulps: of the closed form's largest term)"""
    import fmcmc_amd as F
    case = P.family_case("b")
    r = F.predictive_host(case.model, case.draws, probs=P.PROBS)
    ulps = P.closed_form_ulps(r.quantiles, r.eta[0], r.sigma[0], P.PROBS)
    print("largest distance from the closed form: %.3g ulp" % ulps.max())
    assert (ulps <= 4).all()


def test_the_moments_and_the_pit():
    import fmcmc_amd as F
    case = P.family_case("a")
    r = F.predictive_host(case.model, case.draws, probs=(0.5,))
    ref = F.predict_host(case.model, case.draws, None, (), "linpred", LD)
    assert (P.metric(r.mean, ref.mean) <= P.CAP).all() and (P.metric(r.sd_pred, ref.sd_pred) <= P.CAP).all()
    assert ((r.pit > 0) & (r.pit < 1)).all() and (np.abs(r.pit + r.pit_upper - 1) <= 4 * P.EPS).all()
    G = P.truth(case, case.y[:, None], (0.5,))[0][:, 0] + LD(0.5)                       # F(y) in longdouble
    assert (np.abs(r.pit - G) <= 1e-13).all()
    new = np.random.default_rng(3).uniform(-2, 2, (5, case.p))
    assert F.predictive_host(case.model, case.draws, new).pit is None
    assert F.predictive_host(case.model, case.draws, new, y=np.zeros(5)).pit.shape == (5,)
    with pytest.raises(ValueError, match="y has 4 entries but there are 5 points"):
        F.predictive_host(case.model, case.draws, new, y=np.zeros(4))


def test_a_small_cap_is_reported_not_hidden():
    import fmcmc_amd as F
    case = P.family_case("c")
    r = F.predictive_host(case.model, case.draws, probs=P.PROBS, max_passes=1)
    assert not r.converged.all() and (r.passes[~r.converged] == 0).all()


def test_the_refusals_of_the_python_entries():
    import fmcmc_amd as F
    case = P.family_case("a")
    mo, d = case.model, case.draws
    for bad in ((0.0,), (1.0,), (0.5, 1.5), (float("nan"),)):
        with pytest.raises(ValueError, match="strictly inside"):
            F.predictive_host(mo, d, probs=bad)
        with pytest.raises(ValueError, match="strictly inside"):
            F.predictive(None, mo, probs=bad)
    with pytest.raises(ValueError, match="at most 16 probs"):
        F.predictive(None, mo, probs=[0.5] * 17)
    X = np.asarray(mo.X)
    with pytest.raises(ValueError, match=r"predict\(x, model, newdata, kind=\"epred\"\)"):
        F.predictive(None, F.logistic(X, (case.y > 0).astype(float), intercept=True))
    with pytest.raises(ValueError, match="summary"):
        F.predictive(None, F.iid_normal(case.y))
    with pytest.raises(TypeError, match="to_host"):
        F.predictive(None, F.batched_fun(lambda th: th.sum(axis=1), k=2))
    with pytest.raises(TypeError, match="to_host"):
        F.predictive(None, F.pointwise_fun(lambda th: th[:, :1].repeat(1, 3), 3, 2))
    with pytest.raises(ValueError, match="y has 3 entries"):
        F.predictive(None, mo, newdata=X[:5], y=np.zeros(3))
    batch = object.__new__(F.McmcBatch)
    with pytest.raises(TypeError, match=r"predictive\(ans\[d\], models\[d\]"):
        F.predictive(batch, mo)
    for name in ("predictive", "predictive_host", "PredictiveResult"):
        assert name in F.__all__ and hasattr(F, name)
    assert hasattr(F.DeviceChains, "predictive")


def test_the_refusals_of_the_c_entry_need_no_device():
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    X = np.zeros((3, 17))
    y = np.zeros(17)
    xp, yp = X.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)           # (host pointers: never dereferenced)
    model = lambda fam=abi.FAM_GAUSSIAN_LINREG, p=3: abi.Model(fam, p, 17, xp, yp, 1, 0, 0.0)
    pr = lambda *v: np.asarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    buf = C.c_void_p(8)
    call = lambda m=None, k=5, S=40, row0=0, N=33, probs=pr(0.5), nprobs=1, npasses=4, resume=0, Cn=1: L.fmcmc_predictive_dev(
        C.byref(m if m is not None else model()), buf, Cn, k, S, row0, N, probs, nprobs, npasses, resume, buf, buf, buf, None)
    assert call(k=4) == abi.ERR_ARG and "family has 5" in abi.last_error()
    assert call(N=1) == abi.ERR_ARG and "at least 2" in abi.last_error()
    assert call(row0=8) == abi.ERR_ARG and "outside" in abi.last_error()
    assert call(probs=pr(*([0.5] * 17)), nprobs=17) == abi.ERR_ARG and "nprobs" in abi.last_error()
    for bad in (0.0, 1.0, float("nan")):
        assert call(probs=pr(bad)) == abi.ERR_ARG and "strictly inside" in abi.last_error()
    assert call(probs=None) == abi.ERR_ARG and "null" in abi.last_error()
    assert call(npasses=0) == abi.ERR_ARG and "npasses" in abi.last_error()
    assert call(resume=2) == abi.ERR_ARG and "resume" in abi.last_error()
    assert call(m=model(abi.FAM_LOGISTIC), k=4) == abi.ERR_UNSUPPORTED and "Bernoulli" in abi.last_error()
    assert call(m=abi.Model(abi.FAM_IID_NORMAL, 0, 17, None, yp, 1, 0, 0.0), k=2) == abi.ERR_UNSUPPORTED and "iid_normal" in abi.last_error()
    wl = lambda m, Cn=4, N=500, nprobs=3: L.fmcmc_predictive_work_len(C.byref(m), Cn, N, nprobs)
    assert wl(model()) > 0 and wl(model(abi.FAM_LOGISTIC)) == 0 and wl(model(), nprobs=17) == 0 and wl(model(), Cn=1, N=1) == 0
    # the documented layout: 4 per 256 draws, 8 totals, 1 / sigma per draw, then per part and point 4 + 16 + 2, per point 4 + 8 slots
    upp, nparts = P.SM.waic_parts(4, 500, 17)
    assert wl(model()) == 4 * 8 + 8 + 2000 + nparts * 17 * (4 + 16 + 2) + 17 * 4 + 17 * 4 * 8
    assert L.fmcmc_abi_version() == 6
    for name in ("fmcmc_predictive_work_len", "fmcmc_predictive_dev", "fmcmc_detmath_host"):
        assert name in abi.EXPORTS and hasattr(L, name)


def test_the_result_object():
    import fmcmc_amd as F
    point = np.array([[1.0, 2.0, 0.25, 0.75, 0.5, 1e-17, 1e-3, 3.0, 2.5, 1e-9, 0.5, 0.0]])
    r = F.PredictiveResult(point, (0.1, 0.9), 80, y=[1.5], total_passes=4)
    assert r.quantiles.tolist() == [[0.5, 2.5]] and r.converged.tolist() == [[True, False]] and r.passes.tolist() == [[3, 0]]
    assert r.coverage(0.1, 0.9) == 1.0 and r.pit[0] == 0.25 and r.pit_upper[0] == 0.75 and r.sd_pred[0] == 2.0
    assert "Posterior predictive of y at 1 point from 80 draws (4 passes)" in str(r) and "1 quantile(s) not converged" in str(r)
    none = F.PredictiveResult(point[:, :4], (), 80, y=[1.5])                      # the PIT alone
    assert none.quantiles.shape == (1, 0) and none.pit[0] == 0.25 and none.converged.all()
    assert F.PredictiveResult(point, (0.1, 0.9), 80).pit is None
    with pytest.raises(ValueError, match="needs the y"):
        F.PredictiveResult(point, (0.1, 0.9), 80).coverage(0.1, 0.9)
