"""The host-pointer entry points (fmcmc_mcmc_run_host, fmcmc_mcmc_run_fun_host; staging: csrc/mh_host.hpp) through ctypes
with numpy host buffers, bitwise against the oracle: the families, kernels and streams that tests/test_gpu_api.py's two
host-entry tests (the linear model on the library's own stream) leave out, the callback path with a Python callback, and the
callback path's two ordinary error returns."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import synth_linreg
from test_gpu_parity import _bits_equal, jitter_init

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fmcmc_amd import engine
    return engine


def P(a):
    return a.ctypes.data if a is not None else None


def host_bufs(init, kf, nsteps, burnin=0, thin=1):
    """every fmcmc_state / fmcmc_out array of a host-pointer call, as numpy buffers (the layouts of include/fmcmc_amd.h)"""
    Cn, k = init.shape
    S = (nsteps - burnin) // thin
    B = SimpleNamespace(Cn=Cn, k=k, S=S, fresh=1, step_base=0)
    B.th = np.ascontiguousarray(init, dtype=np.float64).copy(); B.f0 = np.zeros(Cn); B.abs_iter = np.zeros(Cn, np.int64)
    B.Sig = np.zeros((Cn, kf, kf)); B.mp = np.zeros((Cn, kf)); B.hm = np.zeros(Cn, np.int32); B.ne = np.zeros(Cn, np.int32)
    B.cols = np.zeros((Cn, nsteps), np.int32)
    B.samples = np.empty((Cn, k, S)); B.lp = np.empty((Cn, S)); B.dr = np.empty((Cn, k, S))
    B.acc = np.zeros(Cn, np.int64); B.bits = np.zeros((Cn, (nsteps + 31) // 32), np.uint32)
    B.status = np.zeros(Cn, np.int32); B.sstep = np.zeros(Cn, np.int64); B.stheta = np.zeros((Cn, k))
    return B


def abi_kernel(abi, ok):
    return abi.Kernel(ok.kind, ok.k, P(ok.mu), P(ok.scale), P(ok.lb), P(ok.ub), P(ok.fixed), ok.scheme, ok.freq, ok.warmup, ok.bw,
                      ok.until, ok.eps, ok.arate, ok.Sd, P(ok.scheme_seq), 0 if ok.scheme_seq is None else ok.scheme_seq.size,
                      ok.nadapt, P(ok.constr), None, None, None, None, None, ok.ram_qfun, 0, ok.ram_df, ok.ram_eta_exp)


def abi_state_out(abi, B, random_scheme):
    st = abi.State(P(B.th), P(B.f0), P(B.abs_iter), P(B.Sig), P(B.mp), P(B.hm), P(B.ne), B.fresh, 0,
                   P(B.cols) if random_scheme else None, None, None, None)
    out = abi.Out(P(B.samples), P(B.lp), P(B.dr), P(B.acc), P(B.bits), P(B.status), P(B.sstep), P(B.stheta), 0)
    return st, out


def philox_stream_on_host(abi, ok, B, nsteps, seed, chain_base=0):
    """the canonical stream of the next call from fmcmc_rng_stream_dev, copied to host buffers"""
    import torch
    kz = 1 if (ok.kind in abi.SIMPLE_KERNELS and ok.scheme != abi.SCHEME_JOINT) else ok.kf
    if ok.kind == abi.KERNEL_RAM:
        df = {abi.RAM_QFUN_NORMAL: 0.0, abi.RAM_QFUN_T_DF: ok.ram_df}.get(ok.ram_qfun, float(ok.kf))
    else:
        df = -1.0 if ok.kind in (abi.KERNEL_UNIF, abi.KERNEL_UNIF_REFLECTIVE, abi.KERNEL_UMIRROR) else 0.0
    logu = torch.empty((B.Cn, nsteps), dtype=torch.float64, device="cuda:0")
    z = torch.empty((B.Cn, nsteps, kz), dtype=torch.float64, device="cuda:0")
    with torch.cuda.device(0):
        rc = abi.lib().fmcmc_rng_stream_dev(seed, B.step_base, chain_base, B.Cn, nsteps, kz, float(df), logu.data_ptr(), z.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    assert rc == abi.OK, abi.last_error()
    return np.ascontiguousarray(logu.cpu().numpy()), np.ascontiguousarray(z.cpu().numpy())


def abi_run(abi, ok, B, nsteps, burnin, thin, seed, fed):
    """(the fmcmc_run of the next call on B, what keeps its fed stream alive)"""
    if not fed:
        return abi.Run(B.Cn, nsteps, burnin, thin, seed, 0, B.step_base, abi.RNG_PHILOX, 0, None, None), None
    logu, z = philox_stream_on_host(abi, ok, B, nsteps, seed)
    return abi.Run(B.Cn, nsteps, burnin, thin, seed, 0, B.step_base, abi.RNG_FED, 0, P(logu), P(z)), (logu, z)


def assert_equals_oracle(O, ok, B, ro, ost, nsteps):
    """every field the staging moves: the outputs and the carried state"""
    assert np.array_equal(B.status, ro.status) and np.array_equal(B.sstep, ro.status_step)
    assert _bits_equal(B.samples, ro.samples_cks), "samples"
    assert _bits_equal(B.lp, ro.logpost), "logpost"
    assert _bits_equal(B.dr, ro.draws_cks), "draws"
    assert np.array_equal(B.bits, ro.accept_bits) and np.array_equal(B.acc, ro.accept_count)
    assert _bits_equal(B.th, ost.theta0) and _bits_equal(B.f0, ost.f0)
    if ok.kind in (O.K_ADAPT, O.K_RAM):
        assert np.array_equal(B.abs_iter, ost.abs_iter) and _bits_equal(B.Sig, ost.Sigma), "Sigma"
        assert np.array_equal(B.ne, ost.nerrors)
    if ok.kind == O.K_ADAPT:
        hm = ost.have_mean.astype(bool)
        assert np.array_equal(B.hm, ost.have_mean) and _bits_equal(B.mp[hm], ost.mean_prev[hm])
    if ok.scheme == O.SCHEME_RANDOM:
        assert np.array_equal(B.cols[:, 1:nsteps], ost.scheme_cols[:, 1:nsteps])


def run_host_both(O, fam, X, y, ok, init, nsteps, calls=1, burnin=0, thin=1, seed=77, fed=False, intercept=1, guard=1, prior_div=0.0):
    """`calls` consecutive fmcmc_mcmc_run_host calls with the carried state against the oracle's; returns the host buffers"""
    from fmcmc_amd import _abi as abi
    om = O.Model(fam, X, y, intercept=intercept, guard=guard, prior_div=prior_div)
    Xc = None if X is None else np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)
    yc = np.ascontiguousarray(y, dtype=np.float64)
    m = abi.Model(fam, 0 if X is None else Xc.shape[0], yc.size, P(Xc), P(yc), intercept, guard, prior_div)
    ost = O.ChainState(init, ok.kf)
    B = host_bufs(init, ok.kf, nsteps, burnin, thin)
    kk = abi_kernel(abi, ok)
    for _ in range(calls):
        ro = O.run(om, ok, nsteps=nsteps, burnin=burnin, thin=thin, seed=seed, state=ost)
        r, keep = abi_run(abi, ok, B, nsteps, burnin, thin, seed, fed)
        st, out = abi_state_out(abi, B, ok.scheme == O.SCHEME_RANDOM)
        rc = abi.lib().fmcmc_mcmc_run_host(C.byref(m), C.byref(kk), C.byref(r), C.byref(st), C.byref(out), 0)
        assert rc == abi.OK, abi.last_error()
        assert st.fresh == 0
        B.fresh, B.step_base = 0, B.step_base + nsteps
        assert_equals_oracle(O, ok, B, ro, ost, nsteps)
    return B


def synth_logistic(n, p, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(0.3 + X @ np.linspace(0.8, -0.6, p))))).astype(np.float64)
    return X, y


# ---------------------------------------------------------------------------------------------------------------------
# 1. fmcmc_mcmc_run_host on the other families and on a fed stream
# ---------------------------------------------------------------------------------------------------------------------
def test_run_host_logistic(E, O):
    X, y = synth_logistic(211, 2, 31)
    ok = O.Kernel(O.K_NORMAL_REFLECTIVE, 3, scale=0.1, lb=-5.0, ub=5.0, scheme="ordered")
    run_host_both(O, O.FAM_LOGISTIC, X, y, ok, jitter_init([0.0, 0.0, 0.0], 4, 2), 50, burnin=4, thin=3, prior_div=8.0)


def test_run_host_iid_normal_uploads_no_X_and_carries_kernel_ram(E, O):
    D = np.random.default_rng(1231).normal(2.6, 3, 173)
    init = np.abs(jitter_init([2.0, 3.0], 3, 9))
    run_host_both(O, O.FAM_IID_NORMAL, None, D, O.Kernel(O.K_RAM, 2), init, 60, calls=2)


def test_run_host_fed_stream_equals_the_librarys_own(E, O):
    X, y = synth_linreg(300, 2, 5)
    init = jitter_init([0.0, 0.0, 0.0, 4.0], 4, 3)
    ok = O.Kernel(O.K_RAM, 4)
    a = run_host_both(O, O.FAM_LINREG, X, y, ok, init, 60, calls=2)
    b = run_host_both(O, O.FAM_LINREG, X, y, ok, init, 60, calls=2, fed=True)
    # (every output, and the state kernel_ram carries: mean_prev / have_mean are kernel_adapt's, no kernel writes them here)
    for f in ("samples", "lp", "dr", "acc", "bits", "status", "sstep", "stheta", "th", "f0", "abs_iter", "Sig", "ne"):
        va, vb = getattr(a, f), getattr(b, f)
        assert _bits_equal(va, vb) if va.dtype == np.float64 else np.array_equal(va, vb), f


# ---------------------------------------------------------------------------------------------------------------------
# 2. fmcmc_mcmc_run_fun_host with a Python callback
# ---------------------------------------------------------------------------------------------------------------------
def logpost_callback(abi, om, hook=None):
    """abi.LOGPOST_FN over host buffers: f[c] = the oracle's canonical log-posterior of row c; hook(call number, f) -> return code"""
    n = [0]

    def cb(theta, nchains, k, f_out, stream, user):
        th = np.ctypeslib.as_array(C.cast(theta, C.POINTER(C.c_double)), shape=(nchains, k))
        f = np.ctypeslib.as_array(C.cast(f_out, C.POINTER(C.c_double)), shape=(nchains,))
        for c in range(nchains):
            f[c] = om.logpost(th[c])
        n[0] += 1
        return hook(n[0], f) if hook else 0
    return abi.LOGPOST_FN(cb)


def fun_host_call(abi, cb, ok, B, nsteps, burnin=0, thin=1, seed=77, fed=False):
    kk = abi_kernel(abi, ok)
    r, keep = abi_run(abi, ok, B, nsteps, burnin, thin, seed, fed)
    st, out = abi_state_out(abi, B, ok.scheme == abi.SCHEME_RANDOM)
    rc = abi.lib().fmcmc_mcmc_run_fun_host(C.byref(kk), C.byref(r), C.byref(st), C.byref(out), cb, None, 0)
    return rc, st


LINREG = synth_linreg(131, 2, 8)
BOUNDS = dict(lb=[-9, -9, -9, 0.1], ub=9.0)
FUN_CASES = {
    "normal_reflective_random": lambda O: (O.K_NORMAL_REFLECTIVE, dict(scale=0.05, scheme="random", **BOUNDS), False),
    "unif_explicit": lambda O: (O.K_UNIF, dict(min_=-0.1, max_=0.1, scheme=[2, 4, 1, 3]), False),
    "ram_bounded_band_fixed": lambda O: (O.K_RAM, dict(fixed=[False, True, False, False], constr=np.tril(np.triu(np.ones((4, 4)), -1), 1),
                                                       **BOUNDS), False),
    "adapt_fed": lambda O: (O.K_ADAPT, dict(warmup=10), True),
}


@pytest.mark.parametrize("case", list(FUN_CASES))
def test_run_fun_host_bitwise_against_the_oracle(E, O, case):
    from fmcmc_amd import _abi as abi
    kind, kw, fed = FUN_CASES[case](O)
    X, y = LINREG
    om = O.Model(O.FAM_LINREG, X, y)
    ok = O.Kernel(kind, 4, **kw)
    init = jitter_init([0.5, 0.5, 0.5, 4.0], 3, 4)
    ost = O.ChainState(init, ok.kf)
    B = host_bufs(init, ok.kf, 40, 3, 2)
    cb = logpost_callback(abi, om)
    for _ in range(2):
        ro = O.run(om, ok, nsteps=40, burnin=3, thin=2, seed=77, state=ost)
        rc, st = fun_host_call(abi, cb, ok, B, 40, 3, 2, fed=fed)
        assert rc == abi.OK, abi.last_error()
        assert abi.last_kernel() == "fun" and st.fresh == 0
        B.fresh, B.step_base = 0, B.step_base + 40
        assert_equals_oracle(O, ok, B, ro, ost, 40)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the callback path's ways out (ordinary error returns)
# ---------------------------------------------------------------------------------------------------------------------
def test_run_fun_host_callback_error_releases_the_stage(E, O):
    from fmcmc_amd import _abi as abi
    X, y = LINREG
    om = O.Model(O.FAM_LINREG, X, y)
    ok = O.Kernel(O.K_NORMAL, 4, scale=0.05)
    init = jitter_init([0.5, 0.5, 0.5, 4.0], 3, 4)
    B = host_bufs(init, ok.kf, 40)
    rc, st = fun_host_call(abi, logpost_callback(abi, om, lambda n, f: 7 if n == 3 else 0), ok, B, 40)
    assert rc == abi.ERR_FUN
    assert "returned 7 at loop step i = 3" in abi.last_error()
    assert st.fresh == 1
    B = host_bufs(init, ok.kf, 40)     # a good call in the same process
    ro = O.run(om, ok, init, nsteps=40, seed=77)
    rc, st = fun_host_call(abi, logpost_callback(abi, om), ok, B, 40)
    assert rc == abi.OK, abi.last_error()
    assert_equals_oracle(O, ok, B, ro, ro.state, 40)


def test_run_fun_host_nan_from_the_callback_is_a_chain_error(E, O):
    from fmcmc_amd import _abi as abi
    X, y = LINREG
    om = O.Model(O.FAM_LINREG, X, y)
    ok = O.Kernel(O.K_NORMAL, 4, scale=0.05)
    B = host_bufs(jitter_init([0.5, 0.5, 0.5, 4.0], 3, 4), ok.kf, 40)

    def nan_at_7(n, f):
        if n == 7:
            f[1] = np.nan
        return 0
    rc, st = fun_host_call(abi, logpost_callback(abi, om, nan_at_7), ok, B, 40)
    assert rc == abi.ERR_CHAIN
    assert B.status.tolist() == [0, 1, 0] and B.sstep[1] == 7
    assert abi.last_error() == ("fun(par) is undefined (NaN). (chain 1, status 1). Check either -fun- or the -lb- and -ub- parameters. "
                                "This error ocurred during step i = 7")
