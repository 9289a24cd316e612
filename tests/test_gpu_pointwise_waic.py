"""fmcmc_waic_fun_dev (csrc/diag_pointwise.hpp) on the GPU: table matrices (tests/pointwise_cases.py) against
waic_host_matrix in longdouble within the project's cap of 1e-12 (the arithmetic is fmcmc_waic_dev's merge, so its cap carries
over; the device and the host see the same l to the bit); the same bits for every block size, call and position of the window;
the special values; and a real model end to end against the gaussian_linreg family."""
from types import SimpleNamespace

import numpy as np
import pytest

import pointwise_cases as P
import waic_cases as W

pytestmark = pytest.mark.gpu
LD = np.longdouble
TOTALS = ("elpd_waic", "p_waic", "lppd", "waic", "se_elpd", "se_p", "se_lppd")


def _truth_total(t):
    return np.array([getattr(t, f) for f in TOTALS], dtype=LD)


def _assert_cap(point, total, truth, what):
    ep, et = W.metric(point, truth.pointwise), W.metric(total[:7], _truth_total(truth))
    n = point.shape[0]
    ok_t = np.ones(7, dtype=bool) if n > 1 else np.array([1, 1, 1, 1, 0, 0, 0], dtype=bool)
    print("%s: largest pointwise error %.3g, largest total error %.3g" % (what, float(ep.max()), float(et[ok_t].max())))
    assert (ep <= W.CAP).all(), (what, float(ep.max()))
    assert (et[ok_t] <= W.CAP).all(), (what, et)
    if n == 1:
        assert np.isnan(total[4:7]).all()


# n on both sides of the 64 observations of a workgroup; one chain and four; N = 17 (a last tile of one row), 1000 (a last tile
# of 8 rows) and 1024 (none): with four chains of 1024 rows the plan has 8 parts of 32 units
@pytest.mark.parametrize("C_,N", [(1, 17), (4, 17), (1, 1000), (4, 1000), (1, 1024), (4, 1024)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 70])
def test_table_matrices_against_the_host_and_the_same_bits_for_every_block(n, C_, N):
    L = P.smooth_matrix(C_ * N, n, seed=100 * n + C_ + N)
    truth = __import__("fmcmc_amd").waic_host_matrix(L.astype(LD), LD)
    x = P.index_samples(C_, N)
    ref = None
    for br in P.BLOCK_ROWS:
        tab = P.Table(L)
        point, total = P.device_fun("waic", tab, n, x, N, br)
        U = C_ * ((N + 15) // 16)
        assert len(tab.calls) == P.blocks(U, br, n) and sum(tab.calls) == C_ * N
        assert max(tab.calls) <= (16 * ((br + 15) // 16) if br else C_ * N)
        if ref is None:
            ref = (point, total)
            _assert_cap(point, total, truth, "n%d C%d N%d" % (n, C_, N))
            assert total[8] == 0 and total[9] == 0 and total[7] == truth.n_high
        assert np.array_equal(P.bits(point), P.bits(ref[0])) and np.array_equal(P.bits(total), P.bits(ref[1])), br
    # again, and with the window elsewhere in a longer `samples`
    again = P.device_fun("waic", P.Table(L), n, x, N, 48)
    moved = P.device_fun("waic", P.Table(L), n, P.index_samples(C_, N, row0=12, pad=7), N, 48, row0=12)
    for got in (again, moved):
        assert np.array_equal(P.bits(got[0]), P.bits(ref[0])) and np.array_equal(P.bits(got[1]), P.bits(ref[1]))


def test_the_special_values():
    """a constant column has p_waic exactly 0; a -Inf entry is a draw of likelihood zero and leaves lppd finite; a NaN entry makes
    its observation a bad point; the other observations hold the bits of the plain matrix"""
    C_, N, n = 4, 1000, 70
    L = P.smooth_matrix(C_ * N, n, seed=7)
    L[:, 3] = -1.25
    x = P.index_samples(C_, N)
    plain, ptotal = P.device_fun("waic", P.Table(L), n, x, N, 48)
    assert plain[3, 1] == 0.0 and plain[3, 2] == -1.25 and plain[3, 3] == -1.25 and plain[3, 0] == -1.25
    assert ptotal[9] == 0
    Ls = L.copy()
    Ls[1234, 10] = -np.inf
    Ls[77, 65] = np.nan
    point, total = P.device_fun("waic", P.Table(Ls), n, x, N, 48)
    col = L[:, 10].astype(LD)
    col = np.delete(col, 1234)
    lppd = col.max() + np.log(np.exp(col - col.max()).sum() / LD(C_ * N))
    assert np.isfinite(point[10, 2]) and W.metric(point[10, 2], lppd) <= W.CAP
    assert np.isnan(point[65]).all()
    assert total[9] == 2 and total[8] == 0                     # (p_waic of a column with a -Inf is not a number either)
    others = np.setdiff1d(np.arange(n), [10, 65])
    assert np.array_equal(P.bits(point[others]), P.bits(plain[others]))


def test_a_draw_that_is_not_finite():
    import torch
    import fmcmc_amd as F
    C_, N, n = 4, 100, 5
    L = P.smooth_matrix(C_ * N, n, seed=8)
    x = P.index_samples(C_, N)
    x[2, 0, P.ROW0 + 37] = np.nan
    x[0, 0, 0] = np.inf                                          # (outside the window: not counted)
    point, total = P.device_fun("waic", P.Table(L), n, x, N, 0)
    assert total[8] == 1
    dc = F.DeviceChains(torch.as_tensor(np.ascontiguousarray(x[:, :, P.ROW0:P.ROW0 + N])).cuda(), None, None,
                        np.arange(1, N + 1), 1, None, 0, C_)
    with pytest.raises(ValueError, match="1 draw.* not finite"):
        F.waic(dc, F.pointwise_fun(P.Table(L), n, 1))
    with pytest.raises(ValueError, match="1 draw.* not finite"):
        dc.loo(F.pointwise_fun(P.Table(L), n, 1))


def test_the_python_layer_and_its_refusals():
    import torch
    import fmcmc_amd as F
    C_, N, n = 2, 100, 9
    L = P.smooth_matrix(C_ * N, n, seed=9)
    x = P.index_samples(C_, N, row0=0, pad=0)
    dc = F.DeviceChains(torch.as_tensor(x).cuda(), None, None, np.arange(1, N + 1), 1, None, 0, C_)
    truth = F.waic_host_matrix(L.astype(LD), LD)
    w = F.waic(dc, F.pointwise_fun(P.Table(L), n, 1))
    w16 = dc.waic(F.pointwise_fun(P.Table(L), n, 1), block_rows=16)
    assert isinstance(w, F.WaicResult) and w.ndraws == 200 and w.nobs == n and "Computed from 200 by 9" in str(w)
    assert np.array_equal(P.bits(w.pointwise), P.bits(w16.pointwise)) and w.elpd_waic == w16.elpd_waic
    _assert_cap(w.pointwise, np.array([getattr(w, f) for f in TOTALS]), truth, "waic()")
    half = F.waic(dc, F.pointwise_fun(P.Table(L), n, 1), autoburnin=True)
    assert half.ndraws == 100
    # what fn returns is checked: shape, dtype, device
    for bad, text in ((lambda th: torch.zeros(th.shape[0], n + 1, dtype=torch.float64, device=th.device), r"\(200, 10\)"),
                      (lambda th: torch.zeros(th.shape[0], n, dtype=torch.float32, device=th.device), "torch.float32"),
                      (lambda th: torch.zeros(th.shape[0], n, dtype=torch.float64), "on cpu"),
                      (lambda th: None, "NoneType")):
        with pytest.raises(ValueError, match=r"float64 tensor of shape \[200, 9\] on cuda:\d.*got.*" + text):
            F.waic(dc, F.pointwise_fun(bad, n, 1))
    with pytest.raises(ValueError, match="k = 1 parameters, the pointwise_fun has 2"):
        F.waic(dc, F.pointwise_fun(P.Table(L), n, 2))
    with pytest.raises(ValueError, match="block_rows"):
        F.waic(dc, F.pointwise_fun(P.Table(L), n, 1), block_rows=-16)
    with pytest.raises(ValueError, match="block_rows applies to a pointwise_fun"):
        F.waic(dc, F.iid_normal(np.zeros(4)), block_rows=16)
    # an exception in fn surfaces as itself, and the next call is not affected
    with pytest.raises(ZeroDivisionError):
        F.waic(dc, F.pointwise_fun(lambda th: 1 / 0, n, 1))
    assert np.array_equal(P.bits(F.waic(dc, F.pointwise_fun(P.Table(L), n, 1)).pointwise), P.bits(w.pointwise))


def test_an_mcmc_batch_with_a_pointwise_fun_is_refused():
    import fmcmc_amd as F
    rng = np.random.default_rng(3)
    ys = [rng.standard_normal(20) for _ in range(2)]
    batch = F.model_batch([F.iid_normal(y) for y in ys])
    ans = F.MCMC_batch(np.array([0.0, 1.0]), batch, 60, nchains=2, seed=4, kernel=F.kernel_normal(scale=0.1))
    pw = F.pointwise_fun(lambda th: th, 20, 2)
    for f in (F.waic, F.loo):
        with pytest.raises(TypeError, match="McmcBatch.*pointwise_fun scores one dataset"):
            f(ans, pw)


def test_a_regression_written_in_torch_end_to_end():
    """MCMC() on a Gaussian regression given as a batched_fun log-posterior, then waic() and loo() with its pointwise_fun, against
    waic_host / loo_host of the gaussian_linreg family in longdouble on the copied draws.  The callback and the family evaluate
    eta differently, so the tolerance is the family tests' a-priori evaluation bound (waic_cases.loglik_error, carried through
    the reduction by waic_cases.waic_bound) plus the cap of 1e-12; for LOO: the largest evaluation error of the observation plus
    the caps of tests/loo_cases.py."""
    import torch
    import fmcmc_amd as F
    import loo_cases as Lc
    rng = np.random.default_rng(31)
    n, C_ = 70, 3
    X = rng.uniform(-2, 2, (n, 1))
    y = 0.5 + 1.5 * X[:, 0] + rng.standard_normal(n)
    Xd, yd = torch.as_tensor(X).cuda(), torch.as_tensor(y).cuda()

    def pointwise(th):
        r = yd[None, :] - th[:, :1] - th[:, 1:2] * Xd[:, 0][None, :]
        return -torch.log(th[:, 2:3]) - 0.9189385332046727 - 0.5 * r * r / (th[:, 2:3] * th[:, 2:3])

    def logpost(th):
        return torch.where(th[:, 2] > 0, pointwise(torch.where(th[:, 2:3] > 0, th, torch.ones_like(th))).sum(dim=1),
                           torch.full_like(th[:, 2], -float("inf")))

    init = np.array([0.5, 1.5, 1.0]) + 0.01 * np.arange(C_)[:, None]
    dc = F.MCMC(init, F.batched_fun(logpost, 3), 700, seed=8, nchains=C_, burnin=100, kernel=F.kernel_normal(scale=0.08),
                _return_device=True)
    pw, fam = F.pointwise_fun(pointwise, n, 3), F.gaussian_linreg(X, y)
    smp = dc.samples.cpu().numpy()
    assert (smp[:, 2, :] > 0).all()
    case = SimpleNamespace(family="linreg", n=n, p=1, ic=1, C=C_, N=600, model=fam,
                           draws=np.ascontiguousarray(smp.transpose(0, 2, 1).reshape(C_ * 600, 3)))
    b = W.waic_bound(case)
    w = dc.waic(pw)
    rp, rt = W.relative_bound(b)
    ep = W.metric(w.pointwise, b.truth.pointwise)
    et = W.metric([getattr(w, f) for f in TOTALS], _truth_total(b.truth))
    print("waic: largest error %.3g (pointwise), %.3g (totals); largest bound %.3g" % (ep.max(), et.max(), rp.max()))
    assert (ep <= rp + W.CAP).all() and (et <= rt + W.CAP).all()
    assert np.array_equal(P.bits(dc.waic(pw, block_rows=160).pointwise), P.bits(w.pointwise))
    # LOO
    truth = F.loo_host(fam, case.draws, LD)
    emax = Lc.emax_of(case)
    lo = dc.loo(pw)
    e3 = W.metric(lo.pointwise[:, :3], truth.pointwise[:, :3])
    ek, en = W.metric(lo.pointwise[:, 3], truth.pointwise[:, 3]), W.metric(lo.pointwise[:, 4], truth.pointwise[:, 4])
    print("loo: elpd / p_loo / lppd %.3g, k %.3g, n_eff %.3g" % (e3.max(), ek.max(), en.max()))
    assert (e3 <= (emax + Lc.CAP_ELPD)[:, None]).all()
    assert (ek <= emax + Lc.CAP_K).all() and (en <= emax + Lc.CAP_K).all()
    assert (np.abs(lo.pointwise[:, 5].astype(LD) - truth.pointwise[:, 5]) <= emax).all()
    assert np.array_equal(P.bits(dc.loo(pw, block_rows=160).pointwise), P.bits(lo.pointwise))
    # the family's own device result and the callback's, compared
    lf = dc.loo(fam)
    tol = float((2 * emax + 2 * Lc.CAP_ELPD * np.maximum(1, np.abs(truth.pointwise[:, 0]))).sum())
    d = F.loo_compare(lf, lo)
    print("loo_compare(family, pointwise): elpd_diff %.3g, tolerance %.3g" % (d.elpd_diff, tol))
    assert abs(d.elpd_diff) <= tol
    assert abs(F.waic_compare(dc.waic(fam), w).elpd_diff) <= float((2 * b.point[:, 0]).sum()) + 2 * W.CAP * n
