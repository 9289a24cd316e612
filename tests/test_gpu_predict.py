"""fmcmc_predict_dev and predict() on the GPU (csrc/diag_predict.hpp): every shape edge of the fold and of the select against
predict_host in longdouble within the a-priori tolerances of tests/predict_cases.py, the exact cases bit for bit, the bit-for-bit
properties of the plan, the bad draws, the caller's stream, an McmcBatch slice, and MCMC() end to end.

Measured on an MI355X over all cases of this file: mean, sd, sd_pred and the mean of eta within 6.1e-16 (cap 1e-12), the largest
quantile error / tolerance 0.27."""
import ctypes as C
import time

import numpy as np
import pytest

import predict_cases as P

pytestmark = pytest.mark.gpu
LD = np.longdouble


def check(case, kind, probs=P.PROBS, newdata=None, what=None, **kw):
    import fmcmc_amd as F
    point, total = P.device_predict(case, kind, probs, newdata, **kw)
    truth = F.predict_host(case.model, case.draws, newdata, probs, kind, LD)
    P.assert_matches(case, point, truth, P.eta_error(case, newdata), kind, what)
    assert total[0] == case.C * case.N and total[1] == 0 and total[3] == 0
    if case.family == "logistic":
        assert np.isnan(total[2])
    else:
        assert P.metric(total[2], (case.draws[:, -1].astype(LD) ** 2).mean()) <= P.CAP
    return point, total


@pytest.mark.parametrize("spec", P.SHAPES, ids=lambda s: "%s-m%d-p%d-ic%d-C%d-N%d" % s)
def test_shape_edges_within_the_tolerances(spec):
    case = P.shape_case(spec)
    for kind in P.KINDS:
        check(case, kind)


def test_the_parts_the_cases_straddle():
    from fmcmc_amd.summary import waic_parts
    assert [waic_parts(3, N, 65)[1] for N in (33, 181, 350)] == [1, 2, 3]


@pytest.fixture(scope="module")
def wide():
    """m = 130 points (three tiles of 64, the last of two points), three chains, two parts, the logistic map"""
    case = P.make_case("logistic", 130, 3, 1, 3, 181, seed=77)
    return case, P.device_predict(case, "epred")


@pytest.mark.parametrize("name", list(P.PROB_SETS))
@pytest.mark.parametrize("family", P.FAMILIES)
def test_the_probs(family, name):
    """none; one; 16 (32 ranks, four batches of the select); the least and the largest draw; a prob given twice"""
    probs = P.PROB_SETS[name]
    case = P.make_case(family, 65, 3, 1, 3, 33, seed=31)
    for kind in P.KINDS:
        point, _ = check(case, kind, probs)
        assert point.shape == (65, 4 + len(probs))
    if name == "least-and-largest":                                  # (kind epred: the map of the extremes of the device's eta)
        lin, _ = P.device_predict(case, "linpred", probs)
        assert (lin[:, 4] <= lin[:, 0]).all() and (lin[:, 0] <= lin[:, 5]).all()
    if name == "duplicate":
        assert np.array_equal(P.bits(point[:, 4]), P.bits(point[:, 6]))


@pytest.mark.parametrize("family", P.FAMILIES)
def test_exact_draws_give_the_exact_quantiles(family):
    """integer covariates and draws, most rows repeating their predecessor: every quantile of linpred is type7_quantiles of the
    sorted exact eta, bit for bit; the moments within the cap"""
    import fmcmc_amd as F
    case = P.exact_case(family, 65, 3, 3, 181, seed=11)
    probs = (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0)
    point, _ = check(case, "linpred", probs)
    want = F.predict_host(case.model, case.draws, None, probs, "linpred")
    assert np.array_equal(want.eta, np.round(want.eta))
    assert np.array_equal(P.bits(point[:, 4:]), P.bits(want.quantiles))
    check(case, "epred", probs)


def test_new_points_and_the_models_own(wide):
    """newdata = None is newdata = model.X to the bit; other points within the tolerances"""
    case, (point, total) = wide
    same = P.device_predict(case, "epred", newdata=case.model.X)
    assert np.array_equal(P.bits(point), P.bits(same[0])) and np.array_equal(P.bits(total), P.bits(same[1]))
    new = np.random.default_rng(8).uniform(-2, 2, (67, case.p))
    for kind in P.KINDS:
        check(case, kind, newdata=new, what="67 new points")


def test_two_calls_give_the_same_bits(wide):
    case, (point, total) = wide
    again = P.device_predict(case, "epred")
    assert np.array_equal(P.bits(point), P.bits(again[0])) and np.array_equal(P.bits(total), P.bits(again[1]))


def test_the_window_may_sit_anywhere(wide):
    case, (point, total) = wide
    rng = np.random.default_rng(5)
    S2, row2 = case.S + 40, 22
    moved = rng.standard_normal((case.C, case.k, S2)) + 3.0
    moved[:, :, row2:row2 + case.N] = case.samples[:, :, case.row0:case.row0 + case.N]
    got = P.device_predict(case, "epred", samples=moved, row0=row2)
    assert np.array_equal(P.bits(point), P.bits(got[0])) and np.array_equal(P.bits(total), P.bits(got[1]))


def test_a_points_row_does_not_depend_on_the_other_points(wide):
    """both calls have m <= 1024, so the same parts: the rows of the first 64 points alone"""
    case, (point, _total) = wide
    got = P.device_predict(case, "epred", newdata=case.model.X[:64])
    assert got[0].shape == (64, 7) and np.array_equal(P.bits(got[0]), P.bits(point[:64]))


def test_three_parts():
    from fmcmc_amd.summary import waic_parts
    case = P.make_case("linreg", 130, 5, 1, 5, 400, seed=41)
    assert waic_parts(case.C, case.N, case.m)[1] == 4
    for kind in P.KINDS:
        check(case, kind)


def test_bad_draws_are_counted_and_refused():
    import torch
    import fmcmc_amd as F
    for family, bad in (("linreg", 2), ("logistic", 1)):
        case = P.make_case(family, 17, 2, 1, 2, 33, seed=3)
        x = case.samples.copy()
        x[1, 1, case.row0 + 20] = np.nan
        if family == "linreg":
            x[0, case.k - 1, case.row0 + 4] = 0.0
        x[0, 0, 0] = np.nan                                 # outside the window: not a draw
        _point, total = P.device_predict(case, samples=x)
        assert total[1] == bad and total[0] == 66
        window = np.ascontiguousarray(x[:, :, case.row0:case.row0 + case.N])
        dc = F.DeviceChains(torch.as_tensor(window).cuda(), None, None, np.arange(1, case.N + 1), 1, None, 0, case.C)
        with pytest.raises(ValueError, match="%d draw" % bad):
            F.predict(dc, case.model)


def test_the_refusals_come_before_any_device_call():
    import torch
    from fmcmc_amd import _abi as abi
    case = P.make_case("linreg", 17, 2, 1, 1, 33, seed=4)
    L_, cm = abi.lib(), case.model.device_model("cuda").c()
    buf = torch.zeros(256, dtype=torch.float64, device="cuda")
    pr = lambda *v: np.asarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    args = lambda k=case.k, S=40, row0=0, N=33, kind=0, probs=pr(0.5), nprobs=1, Cn=1: (
        C.byref(cm), buf.data_ptr(), Cn, k, S, row0, N, kind, probs, nprobs, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None)
    assert L_.fmcmc_predict_dev(*args(k=case.k - 1)) == abi.ERR_ARG and "family has 4" in abi.last_error()
    assert L_.fmcmc_predict_dev(*args(N=1)) == abi.ERR_ARG and "at least 2" in abi.last_error()
    assert L_.fmcmc_predict_dev(*args(row0=8)) == abi.ERR_ARG and "outside" in abi.last_error()
    assert L_.fmcmc_predict_dev(*args(kind=2)) == abi.ERR_ARG and "kind" in abi.last_error()
    assert L_.fmcmc_predict_dev(*args(probs=pr(*([0.5] * 17)), nprobs=17)) == abi.ERR_ARG and "nprobs" in abi.last_error()
    assert L_.fmcmc_predict_dev(*args(probs=pr(1.5))) == abi.ERR_ARG and "probability" in abi.last_error()
    assert L_.fmcmc_predict_dev(*args(probs=pr(float("nan")))) == abi.ERR_ARG
    assert L_.fmcmc_predict_dev(*args(probs=None)) == abi.ERR_ARG and "null" in abi.last_error()
    iid = abi.Model(abi.FAM_IID_NORMAL, 0, 17, None, cm.y, 1, 0, 0.0)
    a = list(args(k=2))
    a[0] = C.byref(iid)
    assert L_.fmcmc_predict_dev(*a) == abi.ERR_UNSUPPORTED and "iid_normal" in abi.last_error()
    torch.cuda.synchronize()


def test_the_call_stays_on_the_callers_stream(wide):
    """behind a gate on a side stream, with the draws written on that stream after the gate: the bits of the ungated call, and
    the call returns while the gate is closed"""
    import torch
    from test_gpu_streams import Gate, decoy, quiet_host, side_streams
    case, (point, total) = wide
    side = side_streams()[0]
    seen = {}

    def run(inputs, bufs, call):
        xd = inputs[0]
        true = xd.clone()
        xd.copy_(decoy(xd))
        quiet_host()
        gate = Gate(side)
        with torch.cuda.stream(side):
            xd.copy_(true)
            for b in bufs:
                b.fill_(float("nan"))
            t0 = time.perf_counter()
            rc = call(C.c_void_p(side.cuda_stream))
            seen["closed"], seen["ms"] = gate.closed(), 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        seen["gate"] = gate
        return rc

    got = P.device_predict(case, "epred", run=run)
    assert seen["closed"], seen["gate"].too_short(seen["ms"])
    assert np.array_equal(P.bits(point), P.bits(got[0])) and np.array_equal(P.bits(total), P.bits(got[1]))


def test_a_dataset_of_a_batch_is_its_chains_alone():
    """predict(ans[d], models[d], X) on the slice of an McmcBatch against the same chains uploaded on their own; the batch
    itself is pointed to its datasets"""
    import torch
    import fmcmc_amd as F
    rng = np.random.default_rng(21)
    n, D = 40, 3
    X = rng.uniform(-2, 2, (D, n, 2))
    models = F.model_batch([F.gaussian_linreg(X[d], 0.5 + X[d] @ [1.0, -0.5] + rng.standard_normal(n)) for d in range(D)])
    init = np.array([0.5, 1.0, -0.5, 1.0]) + 0.01 * np.arange(2)[:, None]
    ans = F.MCMC_batch(init, models, 200, seed=5, nchains=2, burnin=20, kernel=F.kernel_normal(scale=0.05))
    with pytest.raises(TypeError, match=r"predict\(ans\[d\], models\[d\]"):
        F.predict(ans, models)
    new = rng.uniform(-2, 2, (7, 2))
    for d in (0, 2):
        got = F.predict(ans[d], models[d], new)
        alone = F.DeviceChains(ans[d].samples.clone().contiguous(), None, None, ans[d].iters, ans[d].thin, None, 0, 2)
        ref = F.predict(alone, models[d], new)
        assert np.array_equal(P.bits(got.point_dev.cpu().numpy()), P.bits(ref.point_dev.cpu().numpy()))
        assert got.ndraws == 2 * 180 and got.quantiles.shape == (7, 3)
    torch.cuda.synchronize()


def test_predict_through_the_public_api():
    """MCMC() of a 200 x 3 regression, 4 chains x 500 steps: predict(ans, model) against predict_host of the copied draws within
    the tolerances; newdata = X[:5] equals the first five rows to the bit; the printed table; the logistic family the same way"""
    from types import SimpleNamespace
    import fmcmc_amd as F
    rng = np.random.default_rng(12)
    n = 200
    X = rng.uniform(-2, 2, (n, 3))
    lin = 0.5 + X @ [1.5, -1.0, 0.25]
    fits = (("linreg", F.gaussian_linreg(X, lin + rng.standard_normal(n)), [0.5, 1.5, -1.0, 0.25, 1.0], 0.03),
            ("logistic", F.logistic(X, (rng.uniform(size=n) < 1 / (1 + np.exp(-lin))).astype(float), intercept=True),
             [0.5, 1.5, -1.0, 0.25], 0.1))
    for family, model, start, scale in fits:
        init = np.asarray(start) + 0.01 * np.arange(4)[:, None]
        dc = F.MCMC(init, model, 500, seed=8, nchains=4, kernel=F.kernel_normal(scale=scale), _return_device=True)
        assert isinstance(dc, F.DeviceChains)
        smp = dc.samples.cpu().numpy()
        case = SimpleNamespace(family=family, p=3, ic=1, model=model, name="MCMC " + family,
                               draws=np.ascontiguousarray(smp.transpose(0, 2, 1).reshape(4 * smp.shape[2], -1)))
        emax = P.eta_error(case)
        for kind in P.KINDS:
            r = dc.predict(model, kind=kind)
            assert isinstance(r, F.PredictResult) and r.ndraws == case.draws.shape[0] and r.npoints == n and r.kind == kind
            assert np.array_equal(r.point_dev.cpu().numpy()[:, 0], r.mean) and (r.sd_pred is None) == (family == "logistic")
            truth = F.predict_host(model, case.draws, None, r.probs, kind, LD)
            P.assert_matches(case, r.point_dev.cpu().numpy(), truth, emax, kind)
            five = F.predict(dc, model, newdata=X[:5], kind=kind)
            assert np.array_equal(P.bits(five.point_dev.cpu().numpy()), P.bits(r.point_dev.cpu().numpy()[:5]))
        assert "Prediction (epred) at 200 points from %d draws" % r.ndraws in str(r) and "..." in str(r)
        half = F.predict(dc, model, newdata=X[:5], autoburnin=True)
        assert half.ndraws < r.ndraws
