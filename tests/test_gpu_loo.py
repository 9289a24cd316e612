"""fmcmc_loo_dev and loo() on the GPU (csrc/diag_loo.hpp) against loo_host in longdouble: 1e-12 for elpd_loo, p_loo, lppd, their
totals and standard errors, 1e-10 for pareto_k, n_eff and max_k, the tail and the cutoff within the a-priori evaluation error of
l (tests/loo_cases.py); every shape edge of the tile kernel and of the tail length, the selection machinery driven from
fmcmc_loo_plan through its hit path, both kinds of miss and ties at the cutoff, each side of every form change the plan reports,
a headline-sized tail (M = 9600), the refusals, the bit-for-bit properties, the bad draws, the caller's stream, and loo_compare
through MCMC().

Measured on an MI355X over all cases of this file and of tests/test_gpu_batch_loo.py (71 tests): largest error of elpd_loo, p_loo,
lppd, their totals and standard errors 9.4e-15, of pareto_k and n_eff 2.5e-13 (both: the starved selection case, n = 65), the tail
within 0.43 and the cutoff within 0.22 of the a-priori evaluation error of l."""
import ctypes as C
import time

import numpy as np
import pytest

import loo_cases as Lc
import waic_cases as W

pytestmark = pytest.mark.gpu

# (family, n, p, intercept, chains, rows): WAIC's edges of rows, observations, chains (odd S, row0 = 5) and widths, the logistic
# and iid_normal families, and the edges of the tail length: S = 2, 20 (M = 1, 4: no fit), 21, 25 (M = 5), 224, 225, 226 (where
# 0.2 S meets 3 sqrt S).
ROWS = [("linreg", 17, 2, 1, 1, N) for N in (2, 15, 16, 17, 511, 512, 513, 1025)]
OBS = [("linreg", n, 3, 1, 2, 33) for n in (1, 15, 16, 17, 63, 64, 65, 130)]
CHAINS = [("linreg", 17, 2, 1, C_, 35) for C_ in (1, 2, 3, 5)]
WIDTH = [("linreg", 17, p, 1, 2, 17) for p in (0, 2, 7, 15, 62, 254)]
LOGIT = [("logistic", 65, p, 1, 2, 33) for p in (1, 5)] + [("logistic", 17, 2, 0, 3, 513)]
TAILS = [("linreg", 17, 2, 1, 1, N) for N in (20, 21, 25, 224, 225, 226)]
SHAPES = ROWS + OBS + CHAINS + WIDTH + LOGIT + [("iid", 65, 0, 1, 3, 67)] + TAILS


@pytest.mark.parametrize("spec", SHAPES, ids=lambda s: "%s-n%d-p%d-ic%d-C%d-N%d" % s)
def test_shape_edges(spec):
    case = W.make_case(*spec, seed=2000 + SHAPES.index(spec))
    Lc.check_case(case)


def test_the_plan_is_what_the_documentation_says():
    from fmcmc_amd import _abi as abi
    assert [abi.lib().fmcmc_loo_tail_len(S) for S in (0, 2, 20, 21, 225, 226, 120003, 1024 * 10 ** 4)] == \
        [0, 1, 4, 5, 45, 46, 1040, 9600]
    for C_, N, n in ((3, 40001, 17), (1024, 10000, 10000), (4, 2000, 1000), (1, 33, 5)):
        P = Lc.plan(C_, N, n)
        S = C_ * N
        assert P.M == Lc.loo_tail_len(S) and P.cap >= 3 * P.M and P.cap & (P.cap - 1) == 0 and P.cap < 6 * P.M + 8
        assert P.M + 1 <= P.target <= min(S, P.cap) and P.ustride == max(1, P.target // 96)
        T = (N + 15) // 16
        units = [u for u in range(0, C_ * T, P.ustride)]
        assert P.sub_units == len(units)
        assert P.sub_rows == sum(16 if u % T < T - 1 else N - 16 * (T - 1) for u in units)
        assert P.rank == min(P.sub_rows, max(1, (P.sub_rows * P.target + S // 2) // S))
        assert P.forms == (5, 8193)
    assert Lc.plan(1, 33, 5).ustride == 1 and Lc.plan(1, 33, 5).sub_rows == 33


# ------------------------------------------------------------------------------------------- the selection machinery
SEL_C, SEL_N = 3, 40001


sub_rows_mask = Lc.sub_rows_mask


def selection_case(kind, n):
    """A regression with S = 120003 draws (M = 1040) whose rows are arranged around the plan: see the kinds below."""
    P = Lc.plan(SEL_C, SEL_N, n)
    case = Lc.big_case("linreg", n, 2, SEL_C, SEL_N, seed=500 + n, row0=3)
    rng = np.random.default_rng(7)
    win = case.samples[:, :, case.row0:case.row0 + SEL_N]            # a view [C][k][N]
    insub = sub_rows_mask(P, SEL_C, SEL_N)
    assert P.M == 1040 and P.ustride > 1 and insub.sum() == P.sub_rows

    sd = float(np.median(win[:, -1, :]))

    def push(mask, lo, hi):                                          # an intercept lo .. hi sigma off: a large -l for every observation
        win[:, 0, :][mask] += sd * rng.uniform(lo, hi, int(mask.sum())) * rng.choice([-1.0, 1.0], int(mask.sum()))

    if kind in ("overflow", "starved", "straddle"):
        # one sigma for every row: the offsets alone order the kinds of row, and the largest -l stays within the range of exp
        # above the cutoff (beyond it the ratios of the tail underflow in float64 and nothing is smoothed, which longdouble
        # does not share)
        win[:, -1, :] = sd

    if kind == "overflow":                                           # more extreme draws than the capacity, none in the subsample
        pick = np.flatnonzero(~insub.ravel())
        mask = np.zeros(insub.size, dtype=bool)
        mask[rng.choice(pick, P.cap + 500, replace=False)] = True
        push(mask.reshape(insub.shape), 8.0, 10.0)
    elif kind == "starved":                                          # the threshold lands among extremes only the subsample has
        pick = np.flatnonzero(insub.ravel())
        assert 3 * P.rank < P.M
        mask = np.zeros(insub.size, dtype=bool)
        mask[rng.choice(pick, 3 * P.rank, replace=False)] = True
        push(mask.reshape(insub.shape), 8.0, 10.0)
    elif kind == "runs":                                             # MH-like: every row repeated 1 .. 8 times
        for c in range(SEL_C):
            src = np.repeat(np.arange(SEL_N), rng.integers(1, 9, SEL_N))[:SEL_N]
            win[c] = win[c][:, src]
    elif kind == "straddle":                                         # 95 % of the rows one far-off row, 500 rows further off
        same = rng.uniform(size=insub.shape) < 0.95
        one = win[0, :, 11].copy()
        one[0] += 14.0 * sd
        for c in range(SEL_C):
            win[c][:, same[c]] = one[:, None]
        far = np.zeros(insub.size, dtype=bool)
        far[rng.choice(np.flatnonzero(~same.ravel()), 500, replace=False)] = True
        push(far.reshape(insub.shape), 26.0, 28.0)
    elif kind == "equal":
        win[:] = win[0, :, 11].copy()[None, :, None]
    else:
        assert kind == "plain"
    return P, Lc.finish_case(case)


@pytest.mark.parametrize("n", [17, 65])
@pytest.mark.parametrize("kind", ["plain", "overflow", "starved", "runs", "straddle", "equal"])
def test_the_selection_machinery(kind, n):
    P, case = selection_case(kind, n)
    (point, tail, total, state), truth, _ = Lc.check_case(case, "%s n%d" % (kind, n), want_state=True)
    n_gt, n_eq, flag = state[:, 1], state[:, 2], state[:, 3]
    assert ((n_gt <= P.cap) & (n_gt + n_eq >= P.M + 1)).all()
    if kind in ("overflow", "starved"):
        assert (flag == 1).all() and (n_gt <= P.M).all()             # the exact fallback served every observation
    if kind == "plain":
        assert (flag == 0).all() and (n_gt > P.M).all()
    if kind == "straddle":
        assert (flag == 0).all() and (n_gt == 500).all() and (n_eq > P.cap).all()
        assert (Lc.bits(tail[:, :P.M - 500]) == Lc.bits(point[:, 5])[:, None]).all()     # copies of the cutoff fill the tail
        assert (tail[:, P.M - 500] > point[:, 5]).all()
    if kind == "equal":
        assert (Lc.bits(tail) == Lc.bits(point[:, 5])[:, None]).all() and np.isinf(point[:, 3]).all()
        assert np.array_equal(Lc.bits(point[:, 0]), Lc.bits(point[:, 2])) or (W.metric(point[:, 0], point[:, 2]) <= 1e-15).all()
    if kind == "runs":
        ties = (np.diff(tail, axis=1) == 0).sum()
        assert ties > 0
    # the tail is a sort of values the device evaluated: ascending (check_case), and it ends at the largest -l
    assert (tail[:, 0] >= point[:, 5]).all()


# ----------------------------------------------------------------------------------------- form changes, the long tail
def iid_case(S, n, C_, seed):
    assert S % C_ == 0
    return Lc.big_case("iid", n, 0, C_, S // C_, seed=seed, row0=1)


@pytest.mark.parametrize("S,C_", [(7456540, 4), (7456541, 1)], ids=["M8192", "M8193"])
def test_each_side_of_the_form_change_of_the_finishing_kernel(S, C_):
    """(M = 4 | 5, the other form change of the plan, is S = 20 | 21 of the shape edges)"""
    from fmcmc_amd.summary import loo_tail_len
    assert loo_tail_len(S) == (8192 if S % 2 == 0 else 8193)
    Lc.check_case(iid_case(S, 2, C_, seed=600 + C_))


def test_a_headline_sized_tail():
    case = iid_case(1024 * 10 ** 4, 2, 8, seed=610)
    (point, tail, total), truth, _ = Lc.check_case(case, "headline tail")
    assert tail.shape == (2, 9600) and np.isfinite(point[:, 3]).all()


# --------------------------------------------------------------------------------------------------------- properties
@pytest.fixture(scope="module")
def wide():
    """n = 130 observations (three tiles of 64, the last of two rows), three chains, two parts"""
    case = W.make_case("linreg", 130, 3, 1, 3, 513, seed=77)
    return case, Lc.device_loo(case)


def same_bits(a, b):
    return all(np.array_equal(Lc.bits(x), Lc.bits(y)) for x, y in zip(a[:3], b[:3]))


def test_two_calls_give_the_same_bits(wide):
    case, first = wide
    assert same_bits(first, Lc.device_loo(case))
    again = Lc.device_loo(case, want_tail=False)                    # tail = NULL: the rest as before
    assert np.array_equal(Lc.bits(first[0]), Lc.bits(again[0])) and np.array_equal(Lc.bits(first[2]), Lc.bits(again[2]))
    assert np.isnan(again[1]).all()


def test_the_fallback_gives_the_same_bits_twice():
    _P, case = selection_case("overflow", 17)
    assert same_bits(Lc.device_loo(case), Lc.device_loo(case))


def test_the_window_may_sit_anywhere(wide):
    case, first = wide
    rng = np.random.default_rng(5)
    S2, row2 = case.S + 40, 22
    moved = rng.standard_normal((case.C, case.k, S2)) + 3.0
    moved[:, :, row2:row2 + case.N] = case.samples[:, :, case.row0:case.row0 + case.N]
    assert same_bits(first, Lc.device_loo(case, samples=moved, row0=row2))


def test_the_tile_edge_masks_the_observations_beyond_n(wide):
    import fmcmc_amd as F
    case, first = wide
    m17 = F.gaussian_linreg(case.model.X[:17], case.model.y[:17])
    got = Lc.device_loo(case, model=m17)
    assert got[0].shape == (17, 6) and np.array_equal(Lc.bits(got[0]), Lc.bits(first[0][:17]))
    assert np.array_equal(Lc.bits(got[1]), Lc.bits(first[1][:17]))


def test_bad_draws_are_counted_and_refused():
    import torch
    import fmcmc_amd as F
    case = W.make_case("linreg", 17, 2, 1, 2, 33, seed=3)
    x = case.samples.copy()
    x[0, case.k - 1, case.row0 + 4] = -1.0
    x[1, 1, case.row0 + 20] = np.nan
    x[0, 0, 0] = np.nan                                     # outside the window: not a draw
    _point, _tail, total = Lc.device_loo(case, samples=x)
    assert total[10] == 2
    window = np.ascontiguousarray(x[:, :, case.row0:case.row0 + case.N])
    dc = F.DeviceChains(torch.as_tensor(window).cuda(), None, None, np.arange(1, case.N + 1), 1, None, 0, case.C)
    with pytest.raises(ValueError, match="2 draw"):
        F.loo(dc, case.model)


def test_the_refusals_come_before_any_device_call():
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    case = W.make_case("linreg", 17, 2, 1, 1, 33, seed=4)
    L_, cm = abi.lib(), case.model.device_model("cuda").c()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    b = buf.data_ptr()
    args = lambda k, S, row0, N, Cn=1: (C.byref(cm), b, Cn, k, S, row0, N, b, b, b, b, None)
    assert L_.fmcmc_loo_dev(*args(case.k - 1, 40, 0, 33)) == abi.ERR_ARG and "family has 4" in abi.last_error()
    assert L_.fmcmc_loo_dev(*args(case.k, 40, 0, 1)) == abi.ERR_ARG and "at least 2" in abi.last_error()
    assert L_.fmcmc_loo_dev(*args(case.k, 40, 8, 33)) == abi.ERR_ARG and "outside" in abi.last_error()
    big = 29826162                                                   # the first S whose tail passes 16384
    assert L_.fmcmc_loo_tail_len(big - 1) == 16384 and L_.fmcmc_loo_tail_len(big) == 16385
    assert L_.fmcmc_loo_dev(*args(case.k, big, 0, big)) == abi.ERR_UNSUPPORTED and "16384" in abi.last_error()
    assert L_.fmcmc_loo_dev(C.byref(cm), b, 1, case.k, 40, 0, 33, None, b, b, b, None) == abi.ERR_ARG
    assert L_.fmcmc_loo_dev(C.byref(cm), b, 1, case.k, 40, 0, 33, b, None, b, b, None) == abi.ERR_ARG
    assert L_.fmcmc_loo_dev(C.byref(cm), b, 1, case.k, 40, 0, 33, b, b, b, None, None) == abi.ERR_ARG
    assert L_.fmcmc_loo_dev(C.byref(cm), None, 1, case.k, 40, 0, 33, b, b, b, b, None) == abi.ERR_ARG
    assert L_.fmcmc_loo_dev(None, b, 1, case.k, 40, 0, 33, b, b, b, b, None) == abi.ERR_ARG
    assert (buf == 0).all()
    assert L_.fmcmc_loo_work_len(C.byref(cm), 1, 1, 1) == 0 and L_.fmcmc_loo_work_len(C.byref(cm), 1, 1, 2) > 0
    assert L_.fmcmc_loo_work_len(C.byref(cm), 1, 1, big) == 0 and L_.fmcmc_loo_work_len(None, 1, 1, 33) == 0
    assert L_.fmcmc_loo_state_offset(C.byref(cm), 1, 1, 1) == -1
    out = (C.c_int64 * abi.LOO_PLAN_LEN)()
    assert L_.fmcmc_loo_plan(1, big, 5, out) == abi.ERR_UNSUPPORTED and L_.fmcmc_loo_plan(1, 1, 5, out) == abi.ERR_ARG
    with pytest.raises(TypeError, match="no pointwise form"):
        F.loo(None, object())                                        # (a batched_fun, or anything else that is no closed-form family)


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

    got = Lc.device_loo(case, run=run)
    assert seen["closed"], seen["gate"].too_short(seen["ms"])
    assert same_bits(first, got)


def test_loo_through_the_public_api():
    """MCMC() on a regression and on the same data without its covariate (mis-specified): loo() of both, the printed form, the
    results against loo_host in longdouble, and loo_compare, which prefers the true model."""
    import fmcmc_amd as F
    rng = np.random.default_rng(12)
    n = 40
    X = rng.uniform(-2, 2, (n, 1))
    y = 0.5 + 1.5 * X[:, 0] + rng.standard_normal(n)
    res = []
    for Xm, init0 in ((X, [0.5, 1.5, 1.0]), (None, [0.5, 2.0])):
        model = F.gaussian_linreg(Xm, y)
        init = np.asarray(init0) + 0.01 * np.arange(3)[:, None]
        dc = F.MCMC(init, model, 700, seed=8, nchains=3, burnin=100, kernel=F.kernel_normal(scale=0.08), _return_device=True)
        w = dc.loo(model)
        half = F.loo(dc, model, autoburnin=True)
        assert isinstance(w, F.LooResult) and w.ndraws == 1800 and half.ndraws == 3 * 350 and w.nobs == n and w.tail_len == 128
        assert "elpd_loo" in str(w) and "Computed from 1800 by 40 log-likelihood matrix" in str(w) and "Pareto k" in str(w)
        assert np.array_equal(w.pointwise_dev.cpu().numpy(), w.pointwise) and w.pareto_k.shape == (n,) and w.n_eff.shape == (n,)
        smp = dc.samples.cpu().numpy()
        draws = np.ascontiguousarray(smp.transpose(0, 2, 1).reshape(1800, -1))
        truth = F.loo_host(model, draws, Lc.LD)
        case = W.SimpleNamespace(family="linreg", n=n, p=0 if Xm is None else 1, ic=1, C=3, N=600, model=model, draws=draws)
        total = [getattr(w, f) for f in Lc.TOTALS] + [w.n_k_bad, w.n_k_very_bad, w.max_k]
        Lc.assert_matches(w.pointwise, truth.tail, total, truth, Lc.emax_of(case), "MCMC p=%d" % case.p)
        assert sum(c for _l, c, _p, _n in w.k_table()) == n
        res.append((w, truth))
    (wa, ta), (wb, tb) = res
    got, ref = F.loo_compare(wa, wb), F.loo_compare(ta, tb)
    assert got.elpd_diff > 2 * got.se_diff > 0                       # the true model predicts better
    # every pointwise elpd is within 1e-12 max(1, |elpd_i|) of the truth: the sum of these bounds, and their 2-norm for the se
    tol_i = Lc.CAP_ELPD * (np.maximum(1, np.abs(ta.pointwise[:, 0])) + np.maximum(1, np.abs(tb.pointwise[:, 0])))
    assert abs(got.elpd_diff - ref.elpd_diff) <= float(tol_i.sum()) + 2e-16 * abs(ref.elpd_diff)
    assert abs(got.se_diff - ref.se_diff) <= float(np.sqrt(Lc.LD(n) / (n - 1)) * np.sqrt((tol_i ** 2).sum())) + 2e-16 * ref.se_diff
    assert F.loo_compare(wb, wa).elpd_diff == -got.elpd_diff
