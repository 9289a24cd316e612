"""FMCMC_MAX_K = 256 on the host side (no GPU needed): the ceiling the library reports and validates, what it still refuses
above 64 parameters, the Gelman finish at 200 and 256 columns, and the oracle running kernel_ram / kernel_adapt at 256
parameters on worker threads (the checker of the device kernels' new range)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_abi import numpy_gelman_partial


@pytest.fixture(scope="module")
def abi():
    from fmcmc_amd import _abi, build
    if build.needs_build():
        build.build()
    _abi.lib()
    return _abi


def _linreg_specs(abi, k, kind, scheme=0):
    """A Gaussian linear regression with intercept of k parameters (p = k - 2 covariates) and a kernel over all of them."""
    keep = []

    def arr(a, dt=np.float64):
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data
    p, n = max(k - 2, 0), 10
    m = abi.Model(abi.FAM_GAUSSIAN_LINREG, p, n, arr(np.zeros((p, n))), arr(np.zeros(n)), 1, 1, 0.0)
    kk = abi.Kernel(kind, k, arr(np.zeros(k)), arr(np.ones(k)), arr([-1e308] * k), arr([1e308] * k), arr([0] * k, np.uint8),
                    scheme, 1, 0, 0, float("inf"), 1e-4, 0.234, 0.0)
    r = abi.Run(2, 100, 0, 1, 1, 0, 0, 0, 0, None, None)
    return m, kk, r, keep


def test_max_k_is_256(abi):
    assert abi.MAX_K == 256
    assert abi.lib().fmcmc_abi_version() == abi.ABI_VERSION == 6


@pytest.mark.parametrize("k", [200, 256])
@pytest.mark.parametrize("kind_name", ["KERNEL_RAM", "KERNEL_ADAPT"])
def test_validate_accepts_up_to_256_parameters(abi, k, kind_name):
    m, kk, r, keep = _linreg_specs(abi, k, getattr(abi, kind_name))
    assert abi.lib().fmcmc_validate(C.byref(m), C.byref(kk), C.byref(r)) == abi.OK, abi.last_error()


@pytest.mark.parametrize("kind_name", ["KERNEL_RAM", "KERNEL_ADAPT", "KERNEL_NORMAL"])
def test_validate_refuses_257_parameters(abi, kind_name):
    m, kk, r, keep = _linreg_specs(abi, 257, getattr(abi, kind_name))
    assert abi.lib().fmcmc_validate(C.byref(m), C.byref(kk), C.byref(r)) == abi.ERR_UNSUPPORTED
    assert "number of parameters k=257 outside [1, 256]" in abi.last_error()


def test_ordered_scheme_still_refused_above_64(abi):
    m, kk, r, keep = _linreg_specs(abi, 200, abi.KERNEL_NORMAL, scheme=abi.SCHEME_ORDERED)
    assert abi.lib().fmcmc_validate(C.byref(m), C.byref(kk), C.byref(r)) == abi.ERR_UNSUPPORTED
    assert "k = 200 > 64 parameters: supported are" in abi.last_error()
    kk.scheme = abi.SCHEME_JOINT
    assert abi.lib().fmcmc_validate(C.byref(m), C.byref(kk), C.byref(r)) == abi.OK


@pytest.mark.parametrize("p", [200, 256])
def test_gelman_finish_at_200_and_256_columns(abi, O, p):
    """fmcmc_gelman_finish (the host half of convergence_gelman) against the oracle's coda restatement."""
    rng = np.random.default_rng(p)
    m_, N = 6, 400
    x = rng.standard_normal((m_, N, p)) * (1 + rng.uniform(0, 1, (1, 1, p))) + rng.standard_normal((m_, 1, p)) * 0.4 + 3.0
    center = x[0, 0].copy()
    part = numpy_gelman_partial(x[:2], center) + numpy_gelman_partial(x[2:], center)
    assert part.size == abi.lib().fmcmc_gelman_partial_len(p)
    psrf = np.empty(p)
    mps = C.c_double()
    dp = C.POINTER(C.c_double)
    assert abi.lib().fmcmc_gelman_finish(part.ctypes.data_as(dp), p, N, psrf.ctypes.data_as(dp), C.byref(mps)) == abi.OK
    opsrf, ompsrf = O.gelman(x)
    assert np.allclose(psrf, opsrf, rtol=1e-9)
    assert abs(mps.value - ompsrf) < 1e-9 * ompsrf


def test_oracle_runs_256_parameters_on_worker_threads(O):
    """The oracle's frame grows as k^2 (about 2.7 MB at 256): kernel_ram and kernel_adapt at k = 256 on pool threads, as the
    GPU parity tests run it."""
    k, n = 256, 300
    rng = np.random.default_rng(256)
    X = rng.standard_normal((n, k - 2))
    beta = np.linspace(1.0, -1.0, k - 1)
    y = beta[0] + X @ beta[1:] + 2.0 * rng.standard_normal(n)
    init = np.r_[beta, 2.0][None, :] + 0.02 * rng.standard_normal((2, k))
    model = O.Model(O.FAM_LINREG, X, y)

    def one(kind):
        kern = O.Kernel(kind, k, warmup=5) if kind == O.K_ADAPT else O.Kernel(kind, k)
        return O.run(model, kern, init, nsteps=12, seed=5)
    with ThreadPoolExecutor(2) as ex:
        ram, adapt = ex.map(one, (O.K_RAM, O.K_ADAPT))
    for ro in (ram, adapt):
        assert np.array_equal(ro.status, [0, 0])
        assert ro.samples.shape == (2, 12, k) and np.isfinite(ro.samples).all()
        assert ro.accept_count.sum() > 0
