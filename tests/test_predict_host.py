"""predict_host, the refusals of predict() and of the C entries, and the reference of tests/test_gpu_predict.py, where there is no
GPU: predict_host in float64 against numpy's own quantiles and moments of the explicit matrix; that float64 stays within the
moment cap of longdouble on every case of the GPU file (so no input sits where the reference itself would break the cap); the
refusals that come before any device call; fmcmc_predict_work_len without a device."""
import ctypes as C

import numpy as np
import pytest

import fmcmc_amd as F
from fmcmc_amd import _abi as abi
from fmcmc_amd.summary import type7_quantiles, type7_ranks

import predict_cases as P


@pytest.mark.parametrize("family", P.FAMILIES)
@pytest.mark.parametrize("kind", P.KINDS)
def test_predict_host_is_numpys_quantiles_and_moments(family, kind):
    case = P.make_case(family, 23, 3, 1, 3, 57, seed=5)
    new = np.random.default_rng(6).uniform(-2, 2, (9, 3))
    probs = (0.0, 0.025, 0.3, 0.5, 0.975, 1.0)
    for nd in (None, new):
        got = F.predict_host(case.model, case.draws, nd, probs, kind)
        Xn = case.model.X if nd is None else nd
        eta = case.draws[:, :1] + case.draws[:, 1:4] @ Xn.T
        q = 1.0 / (1.0 + np.exp(-eta)) if (family == "logistic" and kind == "epred") else eta
        assert got.point.shape == (Xn.shape[0], 4 + len(probs)) and got.ndraws == 171 and got.bad_draws == 0
        np.testing.assert_allclose(got.quantiles, np.quantile(q, probs, axis=0, method="linear").T, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got.mean, q.mean(axis=0), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got.sd, q.std(axis=0, ddof=1), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got.mean_eta, eta.mean(axis=0), rtol=1e-12, atol=1e-14)
        if family == "linreg":
            want = np.sqrt(eta.var(axis=0, ddof=1) + (case.draws[:, -1] ** 2).mean())
            np.testing.assert_allclose(got.sd_pred, want, rtol=1e-12)
        else:
            assert got.sd_pred is None and np.isnan(got.point[:, 2]).all()


def test_the_logistic_map_does_not_overflow():
    X = np.array([[1.0], [-1.0], [0.0]])
    model = F.logistic(X, np.zeros(3), intercept=False)
    got = F.predict_host(model, np.array([[800.0], [800.0], [900.0]]), probs=(0.5,), kind="epred")
    assert np.array_equal(got.mean, [1.0, 0.0, 0.5]) and np.array_equal(got.quantiles[:, 0], [1.0, 0.0, 0.5])


@pytest.mark.parametrize("spec", P.SHAPES, ids=lambda s: "%s-m%d-p%d-ic%d-C%d-N%d" % s)
def test_float64_stays_within_the_cap_of_longdouble(spec):
    case = P.shape_case(spec)
    emax = P.eta_error(case)
    for kind in P.KINDS:
        truth = F.predict_host(case.model, case.draws, None, P.PROBS, kind, np.longdouble)
        got = F.predict_host(case.model, case.draws, None, P.PROBS, kind)
        assert truth.point.dtype == np.longdouble
        P.assert_matches(case, got.point, truth, emax, kind)


def test_the_exact_cases_are_exact_and_repeat():
    for family in P.FAMILIES:
        case = P.exact_case(family, 65, 3, 3, 181, seed=11)
        a = F.predict_host(case.model, case.draws, None, P.PROBS, "linpred")
        b = F.predict_host(case.model, case.draws, None, P.PROBS, "linpred", np.longdouble)
        assert np.array_equal(a.eta, b.eta.astype(np.float64)) and np.array_equal(a.eta, np.round(a.eta))
        srt = np.sort(a.eta, axis=0)
        _, lo, hi = type7_ranks(a.ndraws, P.PROBS)
        want = type7_quantiles(np.stack([srt[lo - 1].T, srt[hi - 1].T], axis=-1), a.ndraws, P.PROBS)
        assert np.array_equal(P.bits(a.quantiles), P.bits(want))


def _mcmc():
    return F.Mcmc(np.random.default_rng(1).standard_normal((20, 3)))


def test_predict_refuses_before_any_device_call():
    """none of these reaches the upload of the chains (there is no device here)"""
    rng = np.random.default_rng(2)
    X, y = rng.uniform(-2, 2, (12, 2)), rng.standard_normal(12)
    model = F.logistic(X, (y > 0).astype(float), intercept=True)
    with pytest.raises(ValueError, match=r"summary\(\)"):
        F.predict(_mcmc(), F.iid_normal(y))
    with pytest.raises(TypeError, match="callback"):
        F.predict(_mcmc(), F.batched_fun(lambda th: th.sum(1), 3))
    with pytest.raises(TypeError, match="callback"):
        F.predict(_mcmc(), F.pointwise_fun(lambda th: th, 3, 3))
    with pytest.raises(ValueError, match=r"3 column\(s\).*p = 2"):
        F.predict(_mcmc(), model, newdata=np.zeros((4, 3)))
    with pytest.raises(ValueError, match="at most 16"):
        F.predict(_mcmc(), model, probs=np.linspace(0, 1, 17))
    with pytest.raises(ValueError, match="1.5"):
        F.predict(_mcmc(), model, probs=(0.5, 1.5))
    with pytest.raises(ValueError, match="nan"):
        F.predict(_mcmc(), model, probs=(float("nan"),))
    with pytest.raises(ValueError, match="linpred"):
        F.predict(_mcmc(), model, kind="response")
    with pytest.raises(ValueError, match=r"summary\(\)"):
        F.predict_host(F.iid_normal(y), np.ones((4, 2)))
    with pytest.raises(ValueError, match="at least 2"):
        F.predict_host(model, np.ones((1, 3)))


def test_an_mcmc_batch_is_pointed_to_its_datasets():
    ans = object.__new__(F.McmcBatch)
    with pytest.raises(TypeError, match=r"predict\(ans\[d\], models\[d\]"):
        F.predict(ans, None)


def _model(family, m, p, intercept=1):
    return abi.Model(family, p, m, 8 if p else None, None, intercept, 0, 0.0)     # (X is never dereferenced by the length)


def test_work_len_refuses_what_the_call_refuses():
    L = abi.lib()
    ok = _model(abi.FAM_GAUSSIAN_LINREG, 100, 3)
    wl = lambda m, Cn=4, N=500, nprobs=3: L.fmcmc_predict_work_len(C.byref(m), Cn, N, nprobs)
    assert wl(ok) > 0
    assert L.fmcmc_predict_work_len(None, 4, 500, 3) == 0
    assert wl(ok, nprobs=17) == 0 and "nprobs" in abi.last_error()
    assert wl(ok, nprobs=-1) == 0
    assert wl(ok, Cn=1, N=1) == 0 and "at least 2" in abi.last_error()
    assert wl(ok, Cn=0) == 0 and wl(ok, N=0) == 0
    assert wl(_model(abi.FAM_IID_NORMAL, 100, 0)) == 0 and "iid_normal" in abi.last_error()
    assert wl(_model(7, 100, 3)) == 0 and "unknown family" in abi.last_error()
    assert wl(_model(abi.FAM_LOGISTIC, 0, 3)) == 0
    assert wl(_model(abi.FAM_LOGISTIC, 100, 0, intercept=0)) == 0            # no parameter at all
    assert wl(_model(abi.FAM_GAUSSIAN_LINREG, 100, abi.MAX_K)) == 0 and wl(_model(abi.FAM_LOGISTIC, 100, abi.MAX_K, 0)) > 0
    assert wl(ok, Cn=1 << 20, N=1 << 12) == 0 and "2^31" in abi.last_error()


def test_work_len_never_shrinks():
    """in N, in nprobs and in m: over the part cap's switch at m = 1024 and the units at which a part grows beyond 32"""
    L = abi.lib()
    wl = lambda fam, m, Cn, N, nprobs: L.fmcmc_predict_work_len(C.byref(_model(fam, m, 3)), Cn, N, nprobs)
    for fam in (abi.FAM_GAUSSIAN_LINREG, abi.FAM_LOGISTIC):
        for m, Cn, nprobs in ((1, 1, 0), (100, 3, 3), (1024, 16, 16), (1025, 16, 1), (5000, 1024, 3)):
            seq = [wl(fam, m, Cn, N, nprobs) for N in (2, 15, 16, 17, 511, 512, 513, 8191, 8192, 8193, 8208, 8209, 10000, 131071,
                                                      131072, 131073)]
            assert seq[0] > 0 and all(b >= a for a, b in zip(seq, seq[1:])), (fam, m, Cn, nprobs, seq)
        for m, Cn, N in ((1, 1, 2), (100, 3, 181), (1025, 1024, 10000)):
            seq = [wl(fam, m, Cn, N, nprobs) for nprobs in range(17)]
            assert seq[0] > 0 and all(b >= a for a, b in zip(seq, seq[1:])), (fam, m, Cn, N, seq)
        for Cn, N, nprobs in ((1, 2, 0), (3, 181, 3), (16, 8193, 16), (1024, 10000, 3)):
            seq = [wl(fam, m, Cn, N, nprobs) for m in (1, 63, 64, 65, 130, 1023, 1024, 1025, 1026, 4096, 10000)]
            assert seq[0] > 0 and all(b >= a for a, b in zip(seq, seq[1:])), (fam, Cn, N, nprobs, seq)


def test_the_result_prints_a_table():
    case = P.make_case("linreg", 25, 2, 1, 2, 17, seed=3)
    h = F.predict_host(case.model, case.draws)
    r = F.PredictResult(h.point, h.probs, h.kind, h.ndraws, True)
    text = str(r)
    assert "Prediction (epred) at 25 points from 34 draws" in text and "SD pred" in text and "97.5%" in text and "..." in text
    assert "[1]" in text and "[10]" in text and "[11]" not in text and "[16]" in text and "[25]" in text
    assert r.quantiles.shape == (25, 3) and r.sd_pred.shape == (25,) and r.npoints == 25 and "npoints=25" in repr(r)
    lg = F.PredictResult(np.zeros((3, 4)), (), "linpred", 10, False)
    assert lg.sd_pred is None and "SD pred" not in str(lg) and "..." not in str(lg)
