"""fmcmc_waic_dev and waic() on the GPU (csrc/diag_waic.hpp): every shape edge of the tile kernel against waic_host in longdouble
within the a-priori bound of tests/waic_cases.py (the bound itself capped at 1e-12), the bit-for-bit properties, the bad draws,
the caller's stream, and waic_compare through MCMC().

Measured on an MI355X over the 48 shape cases of the issue's list: largest error 3.0e-15 (p = 254), largest error / bound 0.197."""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np
import pytest

import waic_cases as W

pytestmark = pytest.mark.gpu

TOTALS = ("elpd_waic", "p_waic", "lppd", "waic", "se_elpd", "se_p", "se_lppd")


def part_rows():
    from fmcmc_amd import _abi as abi
    return int(abi.lib().fmcmc_waic_part_rows())


# (family, n, p, intercept, chains, rows).  Rows: the 16-row tile and the part length on both sides (512: pinned below);
# observations: the 16 of a wavefront and the 64 of a workgroup on both sides; chains with an odd S and row0 = 5 (a 16-row load
# is 8-byte aligned only); operand columns k' at the multiples of four, at the 64 columns that stay in registers, at FMCMC_MAX_K.
L = 512
ROWS = [("linreg", 17, 2, 1, 1, N) for N in (2, 15, 16, 17, 33, L - 1, L, L + 1, 2 * L + 1)] + [("linreg", 17, 2, 1, 3, L + 1)]
OBS = [("linreg", n, 3, 1, 2, 33) for n in (1, 15, 16, 17, 63, 64, 65, 130)]
CHAINS = [("linreg", 17, 2, 1, C_, 35) for C_ in (1, 2, 3, 5)]
# (k = 9 and k = 17 besides: the kernel keeps the B tile of up to 2, 4 and 16 steps of four columns in registers, in a form each)
WIDTH = [("linreg", 17, p, ic, 2, 17) for p in (0, 1, 2, 3, 4, 5, 62, 63, 254) for ic in (0, 1)] + \
    [("linreg", 17, 7, 1, 2, 17), ("linreg", 17, 15, 1, 2, 17)]
LOGIT = [("logistic", 65, p, ic, 2, 33) for p in (1, 4, 5) for ic in (0, 1)] + [("logistic", 17, 2, 1, 3, L + 1)]
SHAPES = ROWS + OBS + CHAINS + WIDTH + LOGIT + [("iid", 65, 0, 1, 3, 67)]


def test_the_part_length_the_cases_straddle():
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import waic_parts
    assert part_rows() == L
    for C_, N, n in ((1, L, 17), (1, L + 1, 17), (3, L + 1, 17), (1, 2 * L + 1, 17), (1024, 10000, 10000), (1024, 10000, 100),
                     (4, 2000, 1000)):
        assert abi.lib().fmcmc_waic_parts(C_, N, n) == waic_parts(C_, N, n)[1], (C_, N, n)
    assert [waic_parts(1, N, 17)[1] for N in (L - 1, L, L + 1, 2 * L + 1)] == [1, 1, 2, 3]
    assert waic_parts(1024, 10000, 10000)[1] == 64 and waic_parts(1024, 10000, 100)[1] == 256


@pytest.mark.parametrize("spec", SHAPES, ids=lambda s: "%s-n%d-p%d-ic%d-C%d-N%d" % s)
def test_shape_edges_within_the_bound(spec):
    case = W.make_case(*spec, seed=1000 + SHAPES.index(spec))
    point, total = W.device_waic(case)
    b = W.waic_bound(case)
    W.assert_within(point, total, b, case.name)
    # the counts: n_high up to the observations whose p_waic_i lies within its bound of the threshold
    near = int((np.abs(b.truth.pointwise[:, 1] - 0.4) <= b.point[:, 1]).sum())
    assert abs(int(total[7]) - b.truth.n_high) <= near and total[8] == 0 and total[9] == 0


@pytest.fixture(scope="module")
def wide():
    """n = 130 observations (three tiles of 64, the last of two rows), three chains, two parts"""
    case = W.make_case("linreg", 130, 3, 1, 3, L + 1, seed=77)
    return case, W.device_waic(case)


def test_two_calls_give_the_same_bits(wide):
    case, (point, total) = wide
    again = W.device_waic(case)
    assert np.array_equal(W.bits(point), W.bits(again[0])) and np.array_equal(W.bits(total), W.bits(again[1]))


def test_the_window_may_sit_anywhere(wide):
    case, (point, total) = wide
    rng = np.random.default_rng(5)
    S2, row2 = case.S + 40, 22
    moved = rng.standard_normal((case.C, case.k, S2)) + 3.0
    moved[:, :, row2:row2 + case.N] = case.samples[:, :, case.row0:case.row0 + case.N]
    got = W.device_waic(case, samples=moved, row0=row2)
    assert np.array_equal(W.bits(point), W.bits(got[0])) and np.array_equal(W.bits(total), W.bits(got[1]))


def test_the_tile_edge_masks_the_observations_beyond_n(wide):
    import fmcmc_amd as F
    case, (point, _total) = wide
    m17 = F.gaussian_linreg(case.model.X[:17], case.model.y[:17])
    got = W.device_waic(case, model=m17)
    assert got[0].shape == (17, 4) and np.array_equal(W.bits(got[0]), W.bits(point[:17]))


@pytest.mark.parametrize("family", ["linreg", "logistic"])
def test_equal_draws_have_no_variance(family):
    case = W.make_case(family, 65, 3, 1, 3, L + 1, seed=9)
    same = np.ascontiguousarray(np.broadcast_to(case.samples[:1, :, 7:8], case.samples.shape))
    point, total = W.device_waic(case, samples=same)
    assert (point[:, 1] == 0.0).all() and np.array_equal(W.bits(point[:, 2]), W.bits(point[:, 3]))
    assert np.array_equal(W.bits(point[:, 0]), W.bits(point[:, 2])) and total[1] == 0.0 and total[7] == 0


def test_bad_draws_are_counted_and_refused():
    import torch
    import fmcmc_amd as F
    case = W.make_case("linreg", 17, 2, 1, 2, 33, seed=3)
    x = case.samples.copy()
    x[0, case.k - 1, case.row0 + 4] = -1.0
    x[1, 1, case.row0 + 20] = np.nan
    x[0, 0, 0] = np.nan                                     # outside the window: not a draw
    _point, total = W.device_waic(case, samples=x)
    assert total[8] == 2
    window = np.ascontiguousarray(x[:, :, case.row0:case.row0 + case.N])
    dc = F.DeviceChains(torch.as_tensor(window).cuda(), None, None, np.arange(1, case.N + 1), 1, None, 0, case.C)
    with pytest.raises(ValueError, match="2 draw"):
        F.waic(dc, case.model)


def test_the_refusals_come_before_any_device_call():
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    case = W.make_case("linreg", 17, 2, 1, 1, 33, seed=4)
    L_, cm = abi.lib(), case.model.device_model("cuda").c()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    args = lambda k, S, row0, N, Cn=1: (C.byref(cm), buf.data_ptr(), Cn, k, S, row0, N, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                                        None)
    assert L_.fmcmc_waic_dev(*args(case.k - 1, 40, 0, 33)) == abi.ERR_ARG and "family has 4" in abi.last_error()
    assert L_.fmcmc_waic_dev(*args(case.k, 40, 0, 1)) == abi.ERR_ARG and "at least 2" in abi.last_error()
    assert L_.fmcmc_waic_dev(*args(case.k, 40, 8, 33)) == abi.ERR_ARG and "outside" in abi.last_error()
    assert L_.fmcmc_waic_work_len(C.byref(cm), 1, 1, 1) == 0 and L_.fmcmc_waic_work_len(C.byref(cm), 1, 1, 2) > 0


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

    got = W.device_waic(case, run=run)
    assert seen["closed"], seen["gate"].too_short(seen["ms"])
    assert np.array_equal(W.bits(point), W.bits(got[0])) and np.array_equal(W.bits(total), W.bits(got[1]))


def test_waic_through_the_public_api():
    """MCMC() on a small regression and on the same data with two noise covariates: waic() of both, their printed form, and
    waic_compare of the two against the compare of the two waic_host results in longdouble, within the bounds of both."""
    import fmcmc_amd as F
    rng = np.random.default_rng(12)
    n = 40
    X = rng.uniform(-2, 2, (n, 1))
    y = 0.5 + 1.5 * X[:, 0] + rng.standard_normal(n)
    X3 = np.hstack([X, rng.uniform(-2, 2, (n, 2))])
    res = []
    for Xm in (X, X3):
        model = F.gaussian_linreg(Xm, y)
        init = np.concatenate([[0.5, 1.5], np.zeros(Xm.shape[1] - 1), [1.0]]) + 0.01 * np.arange(3)[:, None]
        dc = F.MCMC(init, model, 700, seed=8, nchains=3, burnin=100, kernel=F.kernel_normal(scale=0.08), _return_device=True)
        assert isinstance(dc, F.DeviceChains)
        w = dc.waic(model)
        half = F.waic(dc, model, autoburnin=True)
        assert isinstance(w, F.WaicResult) and w.ndraws == 3 * 600 and half.ndraws == 3 * 350 and w.nobs == n     # (labels 101 .. 700: coda keeps those from 351 on)
        assert "elpd_waic" in str(w) and "Computed from 1800 by 40 log-likelihood matrix" in str(w)
        assert np.array_equal(w.pointwise_dev.cpu().numpy(), w.pointwise)
        smp = dc.samples.cpu().numpy()
        case = SimpleNamespace(family="linreg", n=n, p=Xm.shape[1], ic=1, C=3, N=600, model=model,
                               draws=np.ascontiguousarray(smp.transpose(0, 2, 1).reshape(1800, -1)))
        b = W.waic_bound(case)
        W.assert_within(w.pointwise, [getattr(w, f) for f in TOTALS], b, "MCMC p=%d" % case.p)
        res.append((w, b))
    (wa, ba), (wb, bb) = res
    both = ba.point[:, 0] + bb.point[:, 0]
    tol_diff = min(float(both.sum()), W.CAP * max(1.0, abs(float(ba.truth.elpd_waic - bb.truth.elpd_waic))))
    for (x, bx), (z, bz) in (((wa, ba), (wb, bb)), ((wb, bb), (wa, ba))):           # either sign of the difference
        got, ref = F.waic_compare(x, z), F.waic_compare(bx.truth, bz.truth)
        assert abs(got.elpd_diff - ref.elpd_diff) <= tol_diff + 2e-16 * abs(ref.elpd_diff)     # (ref: a rounded longdouble)
        tol_se = min(float(np.sqrt(W.LD(n) / (n - 1)) * np.sqrt((both ** 2).sum())), W.CAP * max(1.0, ref.se_diff))
        assert abs(got.se_diff - ref.se_diff) <= tol_se + 2e-16 * ref.se_diff
    assert F.waic_compare(wa, wb).elpd_diff == -F.waic_compare(wb, wa).elpd_diff
