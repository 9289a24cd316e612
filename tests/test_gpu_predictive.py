"""fmcmc_predictive_dev and predictive() on the GPU (csrc/diag_predictive.hpp): every shape edge of the fold, of the evaluation
pass and of the batches against the acceptance property and the bounds of tests/predictive_cases.py, the input families, the
bit-for-bit statements of the contract (two calls, the window, the other points, resume, the early return of finished
workgroups), the cap of passes, the bad draws, the refusals, the caller's stream, the detmath codes, and MCMC() end to end.

Nothing here was measured when this file was written; the figures it prints are recorded in DESIGN.md §5.10 where they were."""
import ctypes as C
import time
import warnings

import numpy as np
import pytest

import predict_cases as PC
import predictive_cases as P

pytestmark = pytest.mark.gpu
LD = np.longdouble
PROBS3 = (0.025, 0.5, 0.975)


def check(case, probs=PROBS3, newdata=None, y="own", what=None, **kw):
    """one device call to the cap of passes: everything finished, the acceptance property of every quantile, the head and the
    PIT within their bounds of the longdouble restatement, total"""
    import fmcmc_amd as F
    point, total = P.device_predictive(case, probs, newdata, y, **kw)
    nprobs = len(probs)
    head, t, g, width, done = P.split(point, nprobs)
    m = point.shape[0]
    emax = P.eta_error(case, newdata)
    tol = P.device_tol(case, m, probs)
    assert total[0] == case.C * case.N and total[1] == 0 and total[5] == 0, total
    assert (done >= 1).all() and (done <= P.MAX_PASSES).all()
    if nprobs:
        P.assert_accepted(case, t, probs, tol, emax, newdata, what)
    ref = F.predict_host(case.model, case.draws, newdata, (), "linpred", LD)
    for got, want in ((head[:, 0], ref.mean), (head[:, 1], ref.sd_pred)):                  # P.moment_bound: CAP and the eta's own
        err = np.abs(got.astype(LD) - want)
        assert (err <= P.moment_bound(want, emax)).all(), float((err / P.moment_bound(want, emax)).max())
    sg = case.draws[:, -1].astype(LD)
    assert P.metric(total[2], (sg ** 2).mean()) <= P.CAP and total[3] == float(sg.min()) and total[4] == float(sg.max())
    yv = (case.y if newdata is None else None) if isinstance(y, str) else y
    if yv is None:
        assert np.isnan(head[:, 2:]).all()
    else:                                                            # F(y) and 1 - F(y): each a direct sum, each relative
        yy = np.asarray(yv, dtype=np.float64)[:, None]
        Glo, d, uphi = P.truth(case, yy, (0.25,), newdata)
        lower = Glo[:, 0] + LD(0.25)
        upper = LD(0.25) - P.truth(case, yy, (0.75,), newdata)[0][:, 0]                # (1 - p) - G
        c = P.SM.predictive_tol(case.C, case.N, m, (0.5,))[1]
        for got, want in ((head[:, 2], lower), (head[:, 3], upper)):
            bound = want * (c * P.EPS + P.SM.NDTR_REL + 2 * P.SM.PNORM_REL) + 2 * d[:, 0] * (emax + P.EPS * np.abs(yy[:, 0])) + P.EPS * uphi[:, 0]
            assert (np.abs(got.astype(LD) - want) <= bound).all(), float((np.abs(got.astype(LD) - want) / bound).max())
    return point, total


# (m, p, intercept, chains, rows): the points at the wavefront, workgroup and WAIC_SMALL_N edges; the rows at the tile edges with
# 1, 2, 3 and 5 chains; two and five parts (a part: 32 units of 16 rows; 3 x 181 rows are 36 units, 3 x 700 are 132, 2 x 1100 138); the coefficient counts of every NQR form and of the LDS form; no intercept
POINTS = [(m, 3, 1, 2, 33) for m in (1, 15, 16, 17, 63, 64, 65, 130, 1025)]
ROWS = [(17, 2, 1, C_, N) for C_ in (1, 2, 3, 5) for N in (1, 2, 15, 16, 17, 33) if C_ * N >= 2]
PARTS = [(65, 3, 1, 3, 181), (65, 3, 1, 3, 700), (65, 3, 1, 2, 1100)]
WIDTHS = [(17, kw - 1, 1, 2, 17) for kw in (1, 4, 5, 8, 9, 16, 17, 64, 65)]
NO_INTERCEPT = [(17, p, 0, 2, 33) for p in (3, 8, 9)]
SHAPES = POINTS + ROWS + PARTS + WIDTHS + NO_INTERCEPT


@pytest.mark.parametrize("spec", SHAPES, ids=lambda s: "m%d-p%d-ic%d-C%d-N%d" % s)
def test_shape_edges(spec):
    case = PC.make_case("linreg", *spec, seed=6000 + SHAPES.index(spec))
    case.y = np.asarray(case.model.y, dtype=np.float64)
    check(case)


def test_the_parts_the_cases_straddle():
    from fmcmc_amd.summary import waic_parts
    assert [waic_parts(C_, N, 65)[1] for C_, N in ((2, 33), (3, 181), (3, 700), (2, 1100))] == [1, 2, 5, 5]


def test_one_draw_is_refused():
    from fmcmc_amd import _abi as abi
    case = PC.make_case("linreg", 17, 2, 1, 1, 2, seed=1)
    cm = case.model.device_model("cuda").c()
    assert abi.lib().fmcmc_predictive_work_len(C.byref(cm), 1, 1, 3) == 0 and "at least 2" in abi.last_error()


@pytest.mark.parametrize("nprobs", [0, 1, 8, 9, 16])
def test_the_batches_of_probs(nprobs):
    """the PIT alone; one prob; a full batch; a batch and one; two full batches"""
    case = P.family_case("a", m=65, C_=3, N=33)
    probs = tuple(np.linspace(0.01, 0.99, nprobs)) if nprobs > 1 else (0.3,)[:nprobs]
    point, _ = check(case, probs)
    assert point.shape == (65, 4 + 4 * nprobs)
    if nprobs == 9:                                                  # a prob's column does not depend on its batch
        alone = P.device_predictive(case, probs[8:])[0]
        assert np.array_equal(P.bits(alone[:, 4:8]), P.bits(point[:, 4 + 32:4 + 36]))


@pytest.fixture(scope="module")
def wide():
    """m = 130 points (three workgroups, the last of two points), three chains, two parts, all six probs"""
    case = P.family_case("a", m=130, C_=3, N=700)
    return case, P.device_predictive(case, P.PROBS)


def test_the_tail_probs_and_the_host_restatement(wide):
    """the six probs of predictive_cases.PROBS, 1 - 10^-6 among them; the device's quantiles against predictive_host in float64"""
    import fmcmc_amd as F
    case, (point, total) = wide
    head, t, g, width, done = P.split(point, len(P.PROBS))
    assert total[5] == 0 and (done >= 1).all()
    P.assert_accepted(case, t, P.PROBS, P.device_tol(case, 130, P.PROBS), P.eta_error(case))
    r = F.predictive_host(case.model, case.draws, probs=P.PROBS)
    print("passes: device %s, host %s" % (done.max(axis=0).tolist(), r.passes.max(axis=0).tolist()))
    # two roots of the same G within their bounds of it: apart by at most the two bounds over the density (first order, x 2)
    G, d, uphi = P.truth(case, t, P.PROBS)
    gap = (P.device_tol(case, 130, P.PROBS) + r.tol)[None, :] + 2 * P.b_f(r.tol, P.PROBS, t, d, uphi, P.eta_error(case))
    assert (np.abs(t - r.quantiles) <= 2 * gap / d + 4 * np.spacing(np.abs(t))).all()
    assert (np.abs(head[:, 2] - r.pit) <= 1e-12).all()


@pytest.mark.parametrize("name", ["b", "c", "e"])
def test_the_input_families(name):
    case = P.family_case(name)
    point, _ = check(case, P.PROBS)
    head, t, g, width, done = P.split(point, len(P.PROBS))
    print("%s: passes per prob %s" % (case.name, done.max(axis=0).tolist()))
    if name == "b":
        th = case.draws[0].astype(LD)
        eta = np.asarray(th[0] + np.asarray(case.model.X, dtype=LD) @ th[1:-1], dtype=np.float64)
        ulps = P.closed_form_ulps(t, eta, case.draws[0, -1], P.PROBS)
        print("largest distance from the closed form: %.3g ulp" % ulps.max())
        assert (ulps <= 4).all()
    if name == "e":                                                  # only the width of the bracket can end these
        assert (width[np.abs(g) > P.device_tol(case, case.m, P.PROBS)[None, :]] <= 2 * np.spacing(np.abs(t).max())).all()


def test_two_calls_give_the_same_bits(wide):
    case, (point, total) = wide
    again = P.device_predictive(case, P.PROBS)
    assert np.array_equal(P.bits(point), P.bits(again[0])) and np.array_equal(P.bits(total), P.bits(again[1]))


def test_the_window_may_sit_anywhere(wide):
    case, (point, total) = wide
    rng = np.random.default_rng(5)
    S2, row2 = case.S + 40, 22
    moved = np.abs(rng.standard_normal((case.C, case.k, S2))) + 3.0
    moved[:, :, row2:row2 + case.N] = case.samples[:, :, case.row0:case.row0 + case.N]
    got = P.device_predictive(case, P.PROBS, samples=moved, row0=row2)
    assert np.array_equal(P.bits(point), P.bits(got[0])) and np.array_equal(P.bits(total), P.bits(got[1]))


def test_a_points_row_does_not_depend_on_the_other_points(wide):
    """both calls have m <= 1024, so the same parts: the rows of the first 64 points alone"""
    case, (point, _total) = wide
    got = P.device_predictive(case, P.PROBS, newdata=case.model.X[:64], y=case.y[:64])
    assert np.array_equal(P.bits(got[0]), P.bits(point[:64]))


def test_eight_passes_are_four_and_four(wide):
    case, _ = wide
    one = P.device_predictive(case, P.PROBS, passes=(8,))
    two = P.device_predictive(case, P.PROBS, passes=(4, 4))
    assert np.array_equal(P.bits(one[0]), P.bits(two[0])) and np.array_equal(P.bits(one[1]), P.bits(two[1]))
    more = P.device_predictive(case, P.PROBS, passes=(3, 1, 2, 2))
    assert np.array_equal(P.bits(one[0]), P.bits(more[0]))


def test_the_early_return_changes_no_bit():
    """64 points that finish early (every draw equal: pass 1) as one whole workgroup, which then returns at once while the
    second workgroup's slow points (two chains 100 sigma apart in their covariate) go on; then the same points spread among the
    slow ones, where no workgroup is ever finished early"""
    rng = np.random.default_rng(9)
    case = P.family_case("c", m=128, p=1, C_=2, N=40)
    x = case.samples
    x[:, 0, :] = x[:1, 0, :1]                                        # one intercept for every draw ...
    x[:, 2, :] = x[:1, 2, :1]                                        # ... one sigma ...
    x[0, 1, :], x[1, 1, :] = 0.5, 0.5 + 100.0 * x[0, 2, 0]           # ... and a slope that differs between the chains
    PC.finish(case)
    fast, slow = np.zeros((64, 1)), rng.uniform(0.5, 2.0, (64, 1))   # at x = 0 every draw gives the same eta
    grouped = np.concatenate([fast, slow])
    order = np.arange(128).reshape(2, 64).T.ravel()                  # fast, slow, fast, slow, ...
    a = P.device_predictive(case, P.PROBS, newdata=grouped, y=None)[0]
    b = P.device_predictive(case, P.PROBS, newdata=grouped[order], y=None)[0]
    da, db = P.split(a, 6)[4], P.split(b, 6)[4]
    print("the fast workgroup finished by pass %d, the slow one by pass %d" % (da[:64].max(), da[64:].max()))
    assert (da[:64] >= 1).all() and da[:64].max() + 4 <= da[64:].max()      # passes that the fast workgroup skips whole
    assert np.array_equal(P.bits(a[order]), P.bits(b))


def test_a_small_cap_is_reported_and_a_larger_one_finishes():
    import torch
    import fmcmc_amd as F
    case = P.family_case("c")
    window = np.ascontiguousarray(case.samples[:, :, case.row0:case.row0 + case.N])
    dc = F.DeviceChains(torch.as_tensor(window).cuda(), None, None, np.arange(1, case.N + 1), 1, None, 0, case.C)
    with pytest.warns(RuntimeWarning, match="had not converged after max_passes = 1"):
        r = F.predictive(dc, case.model, probs=P.PROBS, max_passes=1)
    assert not r.converged.all() and (r.passes[~r.converged] == 0).all() and r.total_passes == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        full = dc.predictive(case.model, probs=P.PROBS)
    assert full.converged.all() and full.total_passes <= P.MAX_PASSES and "Posterior predictive of y at 17 points" in str(full)
    raw = P.device_predictive(case, P.PROBS, passes=(full.total_passes,))[0]
    assert np.array_equal(P.bits(raw), P.bits(full.point_dev.cpu().numpy()))


def test_bad_draws_are_counted_and_refused():
    import torch
    import fmcmc_amd as F
    case = P.family_case("a")
    x = case.samples.copy()
    x[1, 1, case.row0 + 20] = np.nan
    x[0, case.k - 1, case.row0 + 4] = 0.0
    x[0, 0, 0] = np.nan                                              # outside the window: not a draw
    _point, total = P.device_predictive(case, PROBS3, samples=x, passes=(4,))
    assert total[1] == 2 and total[0] == case.C * case.N
    window = np.ascontiguousarray(x[:, :, case.row0:case.row0 + case.N])
    dc = F.DeviceChains(torch.as_tensor(window).cuda(), None, None, np.arange(1, case.N + 1), 1, None, 0, case.C)
    with pytest.raises(ValueError, match="2 draw"):
        F.predictive(dc, case.model)


def test_the_refusals_come_before_any_device_call():
    import torch
    from fmcmc_amd import _abi as abi
    case = PC.make_case("linreg", 17, 2, 1, 1, 33, seed=4)
    L_, cm = abi.lib(), case.model.device_model("cuda").c()
    buf = torch.zeros(256, dtype=torch.float64, device="cuda")
    pr = lambda *v: np.asarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    args = lambda k=case.k, S=40, row0=0, N=33, probs=pr(0.5), nprobs=1, npasses=4, resume=0, Cn=1: (
        C.byref(cm), buf.data_ptr(), Cn, k, S, row0, N, probs, nprobs, npasses, resume, buf.data_ptr(), buf.data_ptr(),
        buf.data_ptr(), None)
    assert L_.fmcmc_predictive_dev(*args(k=case.k - 1)) == abi.ERR_ARG and "family has 4" in abi.last_error()
    assert L_.fmcmc_predictive_dev(*args(N=1)) == abi.ERR_ARG and "at least 2" in abi.last_error()
    assert L_.fmcmc_predictive_dev(*args(row0=8)) == abi.ERR_ARG and "outside" in abi.last_error()
    assert L_.fmcmc_predictive_dev(*args(probs=pr(*([0.5] * 17)), nprobs=17)) == abi.ERR_ARG and "nprobs" in abi.last_error()
    assert L_.fmcmc_predictive_dev(*args(probs=pr(1.0))) == abi.ERR_ARG and "strictly inside" in abi.last_error()
    assert L_.fmcmc_predictive_dev(*args(probs=pr(0.0))) == abi.ERR_ARG and "strictly inside" in abi.last_error()
    assert L_.fmcmc_predictive_dev(*args(npasses=0)) == abi.ERR_ARG and "npasses" in abi.last_error()
    assert L_.fmcmc_predictive_dev(*args(probs=None)) == abi.ERR_ARG and "null" in abi.last_error()
    logit = abi.Model(abi.FAM_LOGISTIC, 2, 17, cm.X, cm.y, 1, 0, 0.0)
    a = list(args(k=3))
    a[0] = C.byref(logit)
    assert L_.fmcmc_predictive_dev(*a) == abi.ERR_UNSUPPORTED and "Bernoulli" in abi.last_error()
    torch.cuda.synchronize()
    assert (buf == 0).all()


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

    got = P.device_predictive(case, P.PROBS, run=run, passes=(12,))
    want = P.device_predictive(case, P.PROBS, passes=(12,))
    assert seen["closed"], seen["gate"].too_short(seen["ms"])
    assert np.array_equal(P.bits(want[0]), P.bits(got[0])) and np.array_equal(P.bits(want[1]), P.bits(got[1]))


def test_the_detmath_codes_on_the_device_equal_the_host_build():
    import torch
    from fmcmc_amd import _abi as abi
    x = P.pnorm_grid()
    xd = torch.as_tensor(x).cuda()
    for which in (11, 12):
        od = torch.empty_like(xd)
        assert abi.lib().fmcmc_detmath_dev(which, xd.data_ptr(), od.data_ptr(), x.size, 0, None) == abi.OK
        torch.cuda.synchronize()
        assert np.array_equal(P.bits(od.cpu().numpy()), P.bits(P.detmath_host(which, x))), which


def test_predictive_through_the_public_api():
    """MCMC() of a 200 x 3 regression generated from the model: the 95 % interval's coverage() of the model's own y lies in
    [0.9, 1.0] and is the count the host restatement gives; the PIT is the in-sample one"""
    import fmcmc_amd as F
    rng = np.random.default_rng(12)
    n = 200
    X = rng.uniform(-2, 2, (n, 3))
    y = 0.5 + X @ [1.5, -1.0, 0.25] + rng.standard_normal(n)
    model = F.gaussian_linreg(X, y)
    init = np.asarray([0.5, 1.5, -1.0, 0.25, 1.0]) + 0.01 * np.arange(4)[:, None]
    dc = F.MCMC(init, model, 500, seed=8, nchains=4, kernel=F.kernel_normal(scale=0.03), _return_device=True)
    r = F.predictive(dc, model)
    assert isinstance(r, F.PredictiveResult) and r.npoints == n and r.converged.all() and r.probs == (0.025, 0.5, 0.975)
    cover = r.coverage(0.025, 0.975)
    print("coverage of the 95 %% interval: %.3f in %d passes" % (cover, r.total_passes))
    assert 0.9 <= cover <= 1.0
    smp = dc.samples.cpu().numpy()
    draws = np.ascontiguousarray(smp.transpose(0, 2, 1).reshape(4 * smp.shape[2], -1))
    h = F.predictive_host(model, draws)
    inside = (h.quantiles[:, 0] <= y) & (y <= h.quantiles[:, 2])
    assert int(round(cover * n)) == int(inside.sum())
    assert (np.abs(r.pit - h.pit) <= 1e-12).all() and ((r.pit > 0) & (r.pit < 1)).all()
    five = dc.predictive(model, newdata=X[:5], y=y[:5])
    assert np.array_equal(P.bits(five.point_dev.cpu().numpy()), P.bits(r.point_dev.cpu().numpy()[:5]))
    assert F.predictive(dc, model, newdata=X[:5]).pit is None
    with pytest.raises(ValueError, match="among probs"):
        r.coverage(0.05, 0.95)
