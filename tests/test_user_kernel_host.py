"""kernel_new() and the C-ABI of user-defined transition kernels, as far as they go without a GPU: the constructor's checks
with the reference's texts (R/kernel.R:291-300), the kernel object as a mutable environment, the new symbols and their ctypes
prototypes, and fmcmc_validate_user's messages."""
import ctypes as C

import numpy as np
import pytest

NEW_SYMBOLS = ("fmcmc_logpost_dev", "fmcmc_validate_user", "fmcmc_mcmc_run_user_dev")


@pytest.fixture(scope="module")
def abi():
    from fmcmc_amd import _abi, build
    if build.needs_build():
        build.build()
    _abi.lib()
    return _abi


def test_kernel_new_is_exported_and_returns_an_fmcmc_kernel():
    import fmcmc_amd
    assert "kernel_new" in fmcmc_amd.__all__
    kn = fmcmc_amd.kernel_new(lambda env: env.theta0)
    assert isinstance(kn, fmcmc_amd.fmcmc_kernel)
    assert kn.logratio is None and callable(kn.proposal)
    assert "kernel_new" in repr(kn)


@pytest.mark.parametrize("bad", [lambda: None, lambda a, b: a, lambda *a: a, lambda **kw: kw, 3, None, "proposal"])
def test_proposal_must_take_a_single_argument(bad):
    from fmcmc_amd import kernel_new
    with pytest.raises(ValueError) as e:
        kernel_new(bad)
    assert str(e.value) == "The `proposal` function should receive a single argument (an environment)."


@pytest.mark.parametrize("bad", [lambda: None, lambda a, b: a, 3, "logratio"])
def test_logratio_must_take_a_single_argument(bad):
    from fmcmc_amd import kernel_new
    with pytest.raises(ValueError) as e:
        kernel_new(lambda env: env.theta0, logratio=bad)
    assert str(e.value).startswith("The `logratio` function should receive a single argument (an environment)")


def test_callables_of_one_argument_are_accepted():
    from fmcmc_amd import kernel_new

    class Prop:
        def __call__(self, env):
            return env.theta0

    def named(env):
        return env.f1 - env.f0
    kn = kernel_new(Prop(), logratio=named)
    assert kn.logratio is named
    kernel_new(lambda env=None: env)   # (one formal, as length(formals(f)) counts it)


def test_state_attributes_round_trip():
    from fmcmc_amd import kernel_new
    sigma = np.array([[1.0, 0.2], [0.2, 1.0]])
    kn = kernel_new(lambda env: env.theta0, sigma_=sigma, ncalls=0, fixed=[False, True])
    assert kn.sigma_ is sigma and kn.ncalls == 0
    kn.ncalls += 5          # (what a callback does through env.kernel)
    kn.history = [1, 2]
    assert kn.ncalls == 5 and kn.history == [1, 2]
    kn._init(2)
    assert kn.k == 2 and kn.fixed.tolist() == [False, True] and kn.which_.tolist() == [0]
    assert kn.ncalls == 5 and kn.sigma_ is sigma      # initialisation leaves the user's objects alone
    with pytest.raises(ValueError, match="Incorrect length of -fixed-"):
        kernel_new(lambda env: env.theta0, fixed=[False, True, False])._init(2)


@pytest.mark.parametrize("name", ["proposal_", "k", "kind", "_state"])
def test_state_names_the_kernel_object_uses_are_refused(name):
    from fmcmc_amd import kernel_new
    if name == "proposal_":
        assert kernel_new(lambda env: env.theta0, **{name: 1}).proposal_ == 1
    else:
        with pytest.raises(ValueError, match="cannot name an object stored with the kernel"):
            kernel_new(lambda env: env.theta0, **{name: 1})


def test_mcmc_accepts_the_kernel_type_and_checks_fun_first():
    """MCMC()'s type checks are unchanged: a kernel_new() kernel passes the kernel check, an arbitrary closure as -fun- does not."""
    from fmcmc_amd import MCMC, kernel_new
    with pytest.raises(TypeError, match="-fun- must be one of"):
        MCMC(np.zeros(2), lambda th: 0.0, 10, kernel=kernel_new(lambda env: env.theta0))


def test_new_symbols_are_exported_with_prototypes(abi):
    L = abi.lib()
    for nm in NEW_SYMBOLS:
        assert nm in abi.EXPORTS
        f = getattr(L, nm)
        assert f.restype is C.c_int and f.argtypes is not None, nm
    assert len(L.fmcmc_logpost_dev.argtypes) == 5
    assert len(L.fmcmc_validate_user.argtypes) == 2
    assert len(L.fmcmc_mcmc_run_user_dev.argtypes) == 10
    assert L.fmcmc_mcmc_run_user_dev.argtypes[1:4] == [abi.LOGPOST_FN, abi.PROPOSAL_FN, abi.LOGRATIO_FN]
    assert L.fmcmc_abi_version() == abi.ABI_VERSION == 6


def test_step_env_layout(abi):
    """fmcmc_step_env of include/fmcmc_amd.h: five int64, k, then five pointers"""
    names = [f[0] for f in abi.StepEnv._fields_]
    assert names == ["i", "nsteps", "nchains", "chain_base", "step_base", "k", "theta0", "theta1", "f0", "f1", "status"]
    assert C.sizeof(abi.StepEnv) == 5 * 8 + 8 + 5 * 8 and abi.StepEnv.theta0.offset == 48


def _run(abi, nchains=2, nsteps=100, burnin=0, thin=1, rng_mode=0):
    return abi.Run(nchains, nsteps, burnin, thin, 1, 0, 0, rng_mode, 0, None, None)


@pytest.mark.parametrize("kw,text", [
    (dict(burnin=100), "-burnin- (100) cannot be >= than -nsteps- (100)."),
    (dict(thin=100), "-thin- (100) cannot be > than -nsteps- (100)."),
    (dict(thin=0), "-thin- should be >= 1."),
    (dict(nchains=0), "`nchains` must be an integer greater than 1."),
])
def test_validate_user_reproduces_the_run_messages(abi, kw, text):
    r = _run(abi, **kw)
    assert abi.lib().fmcmc_validate_user(C.byref(r), 3) == abi.ERR_ARG
    assert abi.last_error() == text


@pytest.mark.parametrize("k", [0, 257, -1])
def test_validate_user_refuses_k_outside_1_256(abi, k):
    r = _run(abi)
    assert abi.lib().fmcmc_validate_user(C.byref(r), k) == abi.ERR_UNSUPPORTED
    assert "outside [1, 256]" in abi.last_error()


@pytest.mark.parametrize("k", [1, 64, 65, 256])
def test_validate_user_accepts_a_good_call(abi, k):
    r = _run(abi)
    assert abi.lib().fmcmc_validate_user(C.byref(r), k) == abi.OK


def test_validate_user_wants_the_fed_uniforms(abi):
    r = _run(abi, rng_mode=abi.RNG_FED)
    assert abi.lib().fmcmc_validate_user(C.byref(r), 3) == abi.ERR_ARG
    assert "fed_logu" in abi.last_error()


def test_run_user_refuses_null_arguments_before_any_device_call(abi):
    L = abi.lib()
    r = _run(abi)
    st, out = abi.State(), abi.Out()
    prop = abi.PROPOSAL_FN(lambda e, o, s, u: 0)
    fun = abi.LOGPOST_FN(lambda t, c, k, o, s, u: 0)
    assert L.fmcmc_mcmc_run_user_dev(None, fun, abi.PROPOSAL_FN(), abi.LOGRATIO_FN(), None, 3, C.byref(r), C.byref(st),
                                     C.byref(out), None) == abi.ERR_ARG
    assert "proposal" in abi.last_error()
    assert L.fmcmc_mcmc_run_user_dev(None, abi.LOGPOST_FN(), prop, abi.LOGRATIO_FN(), None, 3, C.byref(r), C.byref(st),
                                     C.byref(out), None) == abi.ERR_ARG
    assert "log-posterior" in abi.last_error()
    assert L.fmcmc_mcmc_run_user_dev(None, fun, prop, abi.LOGRATIO_FN(), None, 3, C.byref(r), C.byref(st), C.byref(out),
                                     None) == abi.ERR_ARG
    assert "theta0" in abi.last_error()


def test_logpost_dev_refuses_a_bad_model_before_any_device_call(abi):
    L = abi.lib()
    buf = np.zeros(8)
    m = abi.Model(9, 0, 4, None, buf.ctypes.data, 1, 1, 0.0)
    assert L.fmcmc_logpost_dev(C.byref(m), buf.ctypes.data, 1, buf.ctypes.data, None) == abi.ERR_ARG
    assert "unknown log-posterior family" in abi.last_error()
    m = abi.Model(abi.FAM_GAUSSIAN_LINREG, 256, 4, buf.ctypes.data, buf.ctypes.data, 1, 1, 0.0)   # k = 258
    assert L.fmcmc_logpost_dev(C.byref(m), buf.ctypes.data, 1, buf.ctypes.data, None) == abi.ERR_UNSUPPORTED
    m = abi.Model(abi.FAM_IID_NORMAL, 0, 0, None, buf.ctypes.data, 1, 1, 0.0)
    assert L.fmcmc_logpost_dev(C.byref(m), buf.ctypes.data, 1, buf.ctypes.data, None) == abi.ERR_ARG
    assert "at least one observation" in abi.last_error()
