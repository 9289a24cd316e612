"""pointwise_fun, waic_host_matrix and loo_host_matrix on the host: the matrix forms are the host restatements split in two
(waic_loglik, then the matrix), bit for bit; the constructor's refusals; the new symbols of the library.  No GPU."""
import numpy as np
import pytest

import waic_cases as W

LD = np.longdouble
CASES = [("linreg", 17, 5, 1, 2, 100), ("logistic", 15, 2, 0, 1, 33), ("iid", 65, 0, 1, 3, 67)]


def _same(a, b):
    for name, v in vars(a).items():
        w = getattr(b, name)
        v, w = np.asarray(v), np.asarray(w)          # (values, not bytes: a longdouble carries padding)
        assert type(getattr(a, name)) is type(getattr(b, name)) and v.dtype == w.dtype and v.shape == w.shape, name
        assert np.array_equal(v, w, equal_nan=True) and np.array_equal(np.signbit(v), np.signbit(w)), name
    assert sorted(vars(a)) == sorted(vars(b))


@pytest.mark.parametrize("dtype", [np.float64, LD], ids=["float64", "longdouble"])
@pytest.mark.parametrize("family,n,p,ic,C_,N", CASES, ids=[c[0] for c in CASES])
def test_the_matrix_forms_are_the_host_restatements(family, n, p, ic, C_, N, dtype):
    import fmcmc_amd as F
    case = W.make_case(family, n, p, ic, C_, N, seed=21)
    l = F.waic_loglik(case.model, case.draws, dtype)
    assert l.dtype == dtype and l.shape == (C_ * N, n)
    _same(F.waic_host_matrix(l, dtype), F.waic_host(case.model, case.draws, dtype))
    _same(F.loo_host_matrix(l, dtype), F.loo_host(case.model, case.draws, dtype))


def test_a_pointwise_fun_on_cpu_tensors_is_the_family():
    """the Gaussian regression written in torch, evaluated by waic_host / loo_host on CPU tensors, against the family: the two
    evaluate eta differently, so the family tests' evaluation bound decides"""
    import torch
    import fmcmc_amd as F
    case = W.make_case("linreg", 17, 2, 1, 2, 100, seed=22)
    X, y = torch.as_tensor(case.model.X), torch.as_tensor(case.model.y)

    def fn(th):
        r = y[None, :] - th[:, :1] - th[:, 1:3] @ X.T
        return -torch.log(th[:, 3:4]) - 0.9189385332046727 - 0.5 * r * r / (th[:, 3:4] * th[:, 3:4])

    pw = F.pointwise_fun(fn, 17, 4)
    l, ref = F.waic_loglik(pw, case.draws), F.waic_loglik(case.model, case.draws, LD)
    assert (np.abs(l - ref) <= 2 * W.loglik_error(case, ref)).all()
    a, b = F.waic_host(pw, case.draws), F.waic_host(case.model, case.draws)
    assert np.allclose(a.pointwise, b.pointwise, rtol=1e-12, atol=1e-12) and a.bad_draws == 0
    c, d = F.loo_host(pw, case.draws), F.loo_host(case.model, case.draws)
    assert np.allclose(c.pointwise[:, :3], d.pointwise[:, :3], rtol=1e-12, atol=1e-12)
    assert abs(F.loo_compare(c, d).elpd_diff) <= 1e-11
    bad = case.draws.copy()
    bad[3, 1] = np.inf
    assert F.waic_host(pw, bad).bad_draws == 1
    with pytest.raises(ValueError, match=r"\[S\]\[4\]"):
        F.waic_host(pw, case.draws[:, :3])
    wrong = F.pointwise_fun(lambda th: fn(th)[:, :5], 17, 4)
    with pytest.raises(ValueError, match=r"shape \[200, 17\].*got torch.float64 \(200, 5\)"):
        F.waic_host(wrong, case.draws)


def test_the_refusals_of_pointwise_fun():
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    fn = lambda th: th
    with pytest.raises(TypeError, match="callable"):
        F.pointwise_fun(3, 5, 2)
    with pytest.raises(ValueError, match="k = 0"):
        F.pointwise_fun(fn, 5, 0)
    with pytest.raises(ValueError, match="k = %d" % (abi.MAX_K + 1)):
        F.pointwise_fun(fn, 5, abi.MAX_K + 1)
    with pytest.raises(ValueError, match="n = 0"):
        F.pointwise_fun(fn, 0, 2)
    with pytest.raises(ValueError, match="3 names"):
        F.pointwise_fun(fn, 5, 2, names=["a", "b", "c"])
    pw = F.pointwise_fun(fn, 5, abi.MAX_K, names=None)
    assert isinstance(pw, F.PointwiseFun) and pw.n == 5 and pw.k == abi.MAX_K
    assert F.pointwise_fun(fn, 1, 2, names=["a", "b"]).names == ["a", "b"]
    # a batched_fun still has no pointwise form, and the message says what to write instead
    with pytest.raises(TypeError, match="no pointwise form.*pointwise_fun"):
        F.waic_host(F.batched_fun(lambda th: th.sum(dim=1), 2), np.zeros((4, 2)))
    with pytest.raises(TypeError, match="pointwise_fun"):
        F.loo(None, F.batched_fun(lambda th: th.sum(dim=1), 2))


def test_the_library_exports_the_entries():
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    assert L.fmcmc_abi_version() == 6
    for name in ("fmcmc_pointwise_block_rows", "fmcmc_waic_fun_work_len", "fmcmc_waic_fun_dev", "fmcmc_loo_fun_work_len",
                 "fmcmc_loo_fun_state_offset", "fmcmc_loo_fun_dev"):
        assert name in abi.EXPORTS and getattr(L, name) is not None


def test_the_block_rule_and_the_checks_need_no_device():
    """block_rows is rounded up to whole units of 16 rows and never exceeds the draws; 0 is about 2^25 doubles, in whole parts
    where a part fits; what the entries
    refuse they refuse in the *_work_len calls too, with the text in fmcmc_last_error()"""
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    rows = L.fmcmc_pointwise_block_rows
    assert rows(70, 4, 1024, 16) == 16 and rows(70, 4, 1024, 17) == 32 and rows(70, 4, 1024, 528) == 528
    assert rows(70, 4, 1024, 10 ** 6) == 4096 and rows(70, 4, 1024, 0) == 4096
    assert rows(10000, 4, 10000, 0) == 3200                  # 209 units fit 2^25 doubles: five whole parts of 40 units
    assert rows(10000, 1024, 10000, 0) == 3344               # a part has 10000 units there: 209 units of it
    assert rows(1 << 30, 4, 100, 0) == 16
    small, big = L.fmcmc_waic_fun_work_len(70, 4, 1024, 16), L.fmcmc_waic_fun_work_len(70, 4, 1024, 0)
    assert 0 < small < big and big - small == (4096 - 16) * (70 + abi.MAX_K)
    assert L.fmcmc_loo_fun_work_len(70, 4, 1024, 16) > small
    assert 0 < L.fmcmc_loo_fun_state_offset(70, 4, 1024, 16) < L.fmcmc_loo_fun_work_len(70, 4, 1024, 16)
    for args, text in (((0, 4, 1024, 0), "n = 0"), ((70, 0, 1024, 0), "nchains = 0"), ((70, 1, 1, 0), "at least 2"),
                       ((70, 4, 1024, -1), "block_rows = -1")):
        assert L.fmcmc_waic_fun_work_len(*args) == 0 and text in abi.last_error(), (args, abi.last_error())
        assert L.fmcmc_loo_fun_work_len(*args) == 0 and L.fmcmc_loo_fun_state_offset(*args) == -1
    assert L.fmcmc_loo_fun_work_len(1, 1, 30000000, 0) == 0 and "tail" in abi.last_error()
    # the entries themselves: null pointers and a window outside the rows, before any device call
    cb = abi.POINTWISE_FN(lambda *a: 0)
    assert L.fmcmc_waic_fun_dev(cb, None, 70, None, 4, 1, 1030, 5, 1024, 0, None, None, None, None) == abi.ERR_ARG
    assert "null" in abi.last_error()
    one = 8
    assert L.fmcmc_waic_fun_dev(cb, None, 70, one, 4, 1, 1030, 7, 1024, 0, one, one, one, None) == abi.ERR_ARG
    assert "window" in abi.last_error()
    assert L.fmcmc_loo_fun_dev(cb, None, 70, one, 4, 0, 1030, 5, 1024, 0, one, one, None, one, None) == abi.ERR_ARG
    assert "k = 0" in abi.last_error()
