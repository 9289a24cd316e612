"""fmcmc_loo_predictive_dev and loo_predictive() on the GPU (csrc/diag_loo_predictive.hpp) against loo_predictive_host in longdouble
within 1e-10 (tests/loo_predictive_cases.py: the cap and the precondition on the cases): every shape edge of the tile kernel,
both regimes of the tail length, every form of the B operand, two parts, repeated rows, the run that straddles the boundary, the
exact fallback of the selection, the logistic family; bad_points = 0 on every case (the integrity counts hold); the bit-for-bit
properties, the loo part of the call against fmcmc_loo_dev, the caller's stream and the public entry through MCMC().

Measured on an MI355X over the twenty named cases, the 130-observation case and the regression through MCMC(): largest error of the mean 3.5e-14, of sd 1.6e-13, of pit 1.1e-14 (all three:
the straddle case), of pareto_k 4.2e-14 and of n_eff 3.5e-14."""
import ctypes as C
import time

import numpy as np
import pytest

import loo_predictive_cases as Q
import loo_cases as Lc
import waic_cases as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", Q.NAMES)
def test_every_case_against_the_truth(name):
    case = Q.get_case(name)
    want_state = name in ("fallback", "straddle")
    got, truth, _ = Q.check_case(case, want_state=want_state)
    point = got[0]
    assert np.isfinite(point[:, [0, 1, 4, 5]]).all()
    assert np.isnan(point[:, 2]).all() == (case.family == "logistic")
    if name == "fallback":
        P, state = case.plan, got[3]
        assert (state[:, 3] == 1).all() and (state[:, 1] <= P.M).all()       # the exact fallback served every observation
    if name == "straddle":
        state = got[3]
        assert (state[:, 1] == case.n_far).all() and (state[:, 2] > truth.loo.tail_len - case.n_far + 1).all()


@pytest.fixture(scope="module")
def wide():
    """n = 130 observations (three tiles of 64, the last of two rows), three chains, two parts"""
    case = W.make_case("linreg", 130, 3, 1, 3, 513, seed=77)
    case.name = "wide"
    return case, Q.device_loo_predictive(case)


def same_bits(a, b):
    return all(np.array_equal(Q.bits(x), Q.bits(y)) for x, y in zip(a[:3], b[:3]))


def test_two_calls_give_the_same_bits(wide):
    case, first = wide
    Q.assert_matches(first[0], Q.truth_of(case), "wide")
    assert same_bits(first, Q.device_loo_predictive(case))
    again = Q.device_loo_predictive(case, want_loo_point=False)      # loo_point = NULL: the rest as before
    assert np.array_equal(Q.bits(first[0]), Q.bits(again[0])) and np.array_equal(Q.bits(first[2]), Q.bits(again[2]))
    assert np.isnan(again[1]).all()


def test_ties_and_the_fallback_give_the_same_bits_twice():
    for name in ("runs", "fallback"):
        case = Q.get_case(name)
        assert same_bits(Q.device_loo_predictive(case), Q.device_loo_predictive(case))


def test_the_window_may_sit_anywhere(wide):
    case, first = wide
    rng = np.random.default_rng(5)
    S2, row2 = case.S + 40, 22
    moved = rng.standard_normal((case.C, case.k, S2)) + 3.0
    moved[:, :, row2:row2 + case.N] = case.samples[:, :, case.row0:case.row0 + case.N]
    assert same_bits(first, Q.device_loo_predictive(case, samples=moved, row0=row2))


@pytest.mark.parametrize("name", ["wide", "runs", "logistic-n65-p5-ic1-C2-N33", "linreg-n65-p70-ic1-C2-N300"])
def test_the_loo_part_is_fmcmc_loo_dev(name, wide):
    """loo_point and total[0 .. 12) are bit for bit what fmcmc_loo_dev writes; the last three columns of point are copied"""
    case = wide[0] if name == "wide" else Q.get_case(name)
    point, loo_point, total = wide[1] if name == "wide" else Q.device_loo_predictive(case)
    lp, _tail, lt = Lc.device_loo(case)
    assert np.array_equal(Q.bits(loo_point), Q.bits(lp)) and np.array_equal(Q.bits(total[:12]), Q.bits(lt))
    assert np.array_equal(Q.bits(point[:, 3:]), Q.bits(lp[:, [3, 4, 0]])) and total[12] == 0


def test_the_tile_edge_masks_the_observations_beyond_n(wide):
    import fmcmc_amd as F
    case, first = wide
    m17 = F.gaussian_linreg(case.model.X[:17], case.model.y[:17])
    got = Q.device_loo_predictive(case, model=m17)
    assert got[0].shape == (17, 6) and np.array_equal(Q.bits(got[0]), Q.bits(first[0][:17]))


def test_bad_draws_are_counted_and_refused():
    import torch
    import fmcmc_amd as F
    case = W.make_case("linreg", 17, 2, 1, 2, 33, seed=3)
    x = case.samples.copy()
    x[0, case.k - 1, case.row0 + 4] = -1.0
    x[1, 1, case.row0 + 20] = np.nan
    _point, _lp, total = Q.device_loo_predictive(case, samples=x)
    assert total[10] == 2
    window = np.ascontiguousarray(x[:, :, case.row0:case.row0 + case.N])
    dc = F.DeviceChains(torch.as_tensor(window).cuda(), None, None, np.arange(1, case.N + 1), 1, None, 0, case.C)
    with pytest.raises(ValueError, match="2 draw"):
        F.loo_predictive(dc, case.model)


def test_the_refusals_come_before_any_device_call():
    import torch
    from fmcmc_amd import _abi as abi
    case = W.make_case("linreg", 17, 2, 1, 1, 33, seed=4)
    L_, cm = abi.lib(), case.model.device_model("cuda").c()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    b = buf.data_ptr()
    call = lambda k=case.k, S=40, row0=0, N=33: L_.fmcmc_loo_predictive_dev(C.byref(cm), b, 1, k, S, row0, N, b, b, b, b, None)
    assert call(k=case.k - 1) == abi.ERR_ARG and "family has 4" in abi.last_error()
    assert call(N=1) == abi.ERR_ARG and "at least 2" in abi.last_error()
    assert call(row0=8) == abi.ERR_ARG and "outside" in abi.last_error()
    assert L_.fmcmc_loo_predictive_dev(C.byref(cm), b, 1, case.k, 40, 0, 33, None, b, b, b, None) == abi.ERR_ARG
    torch.cuda.synchronize()
    assert (buf == 0).all()


def test_the_call_stays_on_the_callers_stream(wide):
    """behind a gate on a side stream, with the draws written on that stream after the gate: the bits of the ungated call, and
    the call returns while the gate is closed"""
    import torch
    from test_gpu_streams import Gate, decoy, quiet_host, side_streams
    case, first = wide
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

    got = Q.device_loo_predictive(case, run=run)
    assert seen["closed"], seen["gate"].too_short(seen["ms"])
    assert same_bits(first, got)


def test_loo_predictive_through_the_public_api():
    """MCMC() on a small regression and on a logistic model: loo_predictive() equals the raw entry on the same rows bit for bit,
    meets the truth, and its derived figures are those of the arrays"""
    import fmcmc_amd as F
    rng = np.random.default_rng(12)
    n = 40
    X = rng.uniform(-2, 2, (n, 1))
    y = 0.5 + 1.5 * X[:, 0] + rng.standard_normal(n)
    yb = (rng.uniform(size=n) < 1 / (1 + np.exp(-(0.3 + 1.2 * X[:, 0])))).astype(np.float64)
    for model, init0, fam in ((F.gaussian_linreg(X, y), [0.5, 1.5, 1.0], "linreg"), (F.logistic(X, yb, intercept=True), [0.3, 1.2], "logistic")):
        init = np.asarray(init0) + 0.01 * np.arange(3)[:, None]
        dc = F.MCMC(init, model, 700, seed=8, nchains=3, burnin=100, kernel=F.kernel_normal(scale=0.08), _return_device=True)
        r = dc.loo_predictive(model)
        half = F.loo_predictive(dc, model, autoburnin=True)
        assert isinstance(r, F.LooPredictiveResult) and r.ndraws == 1800 and half.ndraws == 3 * 350 and r.nobs == n
        assert np.array_equal(Q.bits(r.point_dev.cpu().numpy()), Q.bits(r.point)) and r.bad_points == 0
        smp = dc.samples.cpu().numpy()
        case = W.SimpleNamespace(family=fam, n=n, p=1, ic=1, C=3, N=600, k=smp.shape[1], S=600, row0=0, model=model, samples=smp,
                                 name="MCMC " + fam)
        Lc.finish_case(case)
        raw = Q.device_loo_predictive(case)
        assert np.array_equal(Q.bits(raw[0]), Q.bits(r.point)) and np.array_equal(Q.bits(raw[1]), Q.bits(r.loo.pointwise))
        ref = dc.loo(model)
        assert np.array_equal(Q.bits(ref.pointwise), Q.bits(r.loo.pointwise)) and ref.elpd_loo == r.loo.elpd_loo
        Q.assert_matches(r.point, Q.truth_of(case), case.name)       # (MH rows repeat: ties are the normal case)
        assert "Leave-one-out predictive checks of 40 observations from 1800 draws" in str(r)
        m = r.metrics()
        if fam == "linreg":
            assert 0.5 < m["r2"] < 1 and 0.5 <= r.coverage(0.9) <= 1 and r.pit_hist(5)[0].sum() == n
            assert m["rmse"] == float(np.sqrt(((y - r.mean) ** 2).mean()))
        else:
            assert 0 < m["brier"] < 0.25 and m["accuracy"] > 0.5 and np.isnan(r.pit).all()
