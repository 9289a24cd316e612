"""User-defined log-posteriors through a batched callback (fmcmc_logpost_fn), the parts that need no GPU: the new C-ABI
symbols, fmcmc_validate_fun's messages and refusals, and the Python front end's checks before any device work."""
import ctypes as C

import numpy as np
import pytest

from test_abi import _host_specs, declared_functions


@pytest.fixture(scope="module")
def abi():
    from fmcmc_amd import _abi, build
    if build.needs_build():
        build.build()
    _abi.lib()
    return _abi


def test_callback_entry_points_are_declared_and_exported(abi):
    names = declared_functions()
    new = ["fmcmc_validate_fun", "fmcmc_mcmc_run_fun_dev", "fmcmc_mcmc_run_fun_host"]
    assert set(new) <= set(names)
    assert set(new) <= set(abi.EXPORTS)
    L = abi.lib()
    assert all(hasattr(L, n) for n in new)
    assert "fmcmc_logpost_fn" not in names          # (the callback type is not a function the library exports)
    assert abi.ERR_FUN == 5 and L.fmcmc_abi_version() == 6


def _validate_fun(abi, **kw):
    m, kk, r, keep = _host_specs(abi, **kw)
    return abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)), kk, r, keep


@pytest.mark.parametrize("kw,substr", [
    (dict(burnin=100), "-burnin- (100) cannot be >= than -nsteps- (100)."),
    (dict(thin=100), "-thin- (100) cannot be > than -nsteps- (100)."),
    (dict(thin=0), "-thin- should be >= 1."),
    (dict(nchains=0), "`nchains` must be an integer greater than 1."),
    (dict(fixed=[1, 1, 1]), "cannot be zero"),
    (dict(kind=2, lb=[0, 0, 1.0], ub=[1, 1, 1.0]), "-ub- cannot be <= than -lb-."),
])
def test_validate_fun_reproduces_the_run_messages(abi, kw, substr):
    """The run-argument checks of fmcmc_validate (R/mcmc.R:501-520) with their messages; the model's own check (the length
    of -initial-) is the caller's: the callback has no parameter count of its own."""
    rc, kk, r, keep = _validate_fun(abi, **kw)
    assert rc == abi.ERR_ARG
    assert substr in abi.last_error()


@pytest.mark.parametrize("k", [1, 3, 64, 65, 256])
@pytest.mark.parametrize("kind,scheme", [(1, 0), (1, 1), (1, 2), (2, 0), (5, 1), (6, 0), (3, 0), (4, 0)])
def test_validate_fun_accepts_the_kernels_in_scope(abi, k, kind, scheme):
    """every scheme of the normal / uniform kernels at every k (the family path takes only 'joint' beyond 64), kernel_adapt
    (bw = 0, freq = 1), kernel_ram"""
    rc, kk, r, keep = _validate_fun(abi, k=k, kind=kind, lb=[-1.0] * k, ub=[1.0] * k)
    kk.scheme = scheme
    assert abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)) == abi.OK, abi.last_error()
    assert abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)) == abi.OK


@pytest.mark.parametrize("kind,bw,freq,substr", [(7, 0, 1, "mirror kernels"), (8, 0, 1, "mirror kernels"),
                                                 (3, 5, 1, "bw = 0 and freq = 1"), (3, 0, 2, "bw = 0 and freq = 1")])
def test_validate_fun_refuses_what_is_out_of_scope(abi, kind, bw, freq, substr):
    rc, kk, r, keep = _validate_fun(abi, kind=kind, lb=[-1.0] * 3, ub=[1.0] * 3)
    kk.bw, kk.freq, kk.warmup = bw, freq, 10
    assert abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)) == abi.ERR_UNSUPPORTED
    assert substr in abi.last_error()


def test_validate_fun_keeps_the_kernel_checks(abi):
    rc, kk, r, keep = _validate_fun(abi, kind=4, lb=[-1.0] * 3, ub=[1.0] * 3)
    kk.ram_qfun = 3
    assert abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)) == abi.ERR_ARG
    assert "unknown -qfun- family" in abi.last_error()
    rc, kk, r, keep = _validate_fun(abi, k=300)
    assert rc == abi.ERR_UNSUPPORTED and "outside [1, 256]" in abi.last_error()


def test_batched_fun_constructor_checks():
    import fmcmc_amd as F
    f = F.batched_fun(lambda th: th.sum(1), 4, names=["a", "b", "c", "d"])
    assert isinstance(f, F.BatchedFun) and f.k == 4 and f.names == ["a", "b", "c", "d"]
    with pytest.raises(TypeError):
        F.batched_fun(3.0, 2)
    with pytest.raises(ValueError):
        F.batched_fun(lambda th: th, 0)
    with pytest.raises(ValueError):
        F.batched_fun(lambda th: th, 257)
    with pytest.raises(ValueError):
        F.batched_fun(lambda th: th, 2, names=["a"])


@pytest.mark.parametrize("checker", [False, True])
def test_wrong_initial_length_is_refused_before_device_work(checker):
    import fmcmc_amd as F
    calls = []
    f = F.batched_fun(lambda th: calls.append(1) or th.sum(1), 3)
    kw = dict(conv_checker=F.convergence_gelman(50)) if checker else {}
    with pytest.raises(ValueError, match="Incorrect length of -initial-"):
        F.MCMC(np.zeros((2, 4)), f, 100, nchains=2, seed=1, **kw)
    assert not calls


def test_a_plain_callable_keeps_the_type_error():
    import fmcmc_amd as F
    with pytest.raises(TypeError, match="closed-form families"):
        F.MCMC([0.0, 1.0], lambda th: -np.sum(th ** 2), 100, seed=1)
