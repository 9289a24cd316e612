"""One model on many datasets (fmcmc_mcmc_run_batch_*, MCMC_batch), the parts that need no GPU: the new C-ABI symbols,
fmcmc_validate_batch's acceptances, refusals and messages, the stride check of the run entries, model_batch's errors and the
shapes of `initial`."""
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


NEW = ["fmcmc_validate_batch", "fmcmc_mcmc_run_batch_dev", "fmcmc_mcmc_run_batch_host"]


def test_batch_entry_points_are_declared_and_exported(abi):
    names = declared_functions()
    assert set(NEW) <= set(names)
    assert set(NEW) <= set(abi.EXPORTS)
    L = abi.lib()
    assert all(hasattr(L, n) for n in NEW)
    assert abi.BATCH_STREAM_DATA == 1 and L.fmcmc_abi_version() == 6


def _validate_batch(abi, nmodels=3, nchains=6, **kw):
    m, kk, r, keep = _host_specs(abi, nchains=nchains, **kw)
    return abi.lib().fmcmc_validate_batch(C.byref(m), nmodels, C.byref(kk), C.byref(r)), m, kk, r, keep


def test_validate_batch_accepts_three_datasets_of_two_chains(abi):
    rc, *_ = _validate_batch(abi)
    assert rc == abi.OK, abi.last_error()


@pytest.mark.parametrize("kind,scheme", [(1, 0), (1, 1), (1, 2), (2, 0), (5, 1), (6, 0), (3, 0), (4, 0)])
@pytest.mark.parametrize("k,p", [(3, 1), (64, 62)])
def test_validate_batch_accepts_the_kernels_of_the_callback_path(abi, k, p, kind, scheme):
    rc, m, kk, r, keep = _validate_batch(abi, k=k, p=p, kind=kind, lb=[-1.0] * k, ub=[1.0] * k)
    kk.scheme = scheme
    assert abi.lib().fmcmc_validate_batch(C.byref(m), 3, C.byref(kk), C.byref(r)) == abi.OK, abi.last_error()


@pytest.mark.parametrize("kw,substr", [
    (dict(burnin=100), "-burnin- (100) cannot be >= than -nsteps- (100)."),
    (dict(thin=100), "-thin- (100) cannot be > than -nsteps- (100)."),
    (dict(thin=0), "-thin- should be >= 1."),
    (dict(nchains=0), "`nchains` must be an integer greater than 1."),
    (dict(k=4), "Incorrect length of -initial-"),
    (dict(fixed=[1, 1, 1]), "cannot be zero"),
])
def test_validate_batch_gives_validates_own_texts(abi, kw, substr):
    kw = dict(kw)
    rc, *_ = _validate_batch(abi, nchains=kw.pop("nchains", 6), **kw)
    assert rc == abi.ERR_ARG
    assert substr in abi.last_error()


def test_validate_batch_refuses_a_model_without_observations(abi):
    rc, m, kk, r, keep = _validate_batch(abi)
    m.n = 0
    assert abi.lib().fmcmc_validate_batch(C.byref(m), 3, C.byref(kk), C.byref(r)) == abi.ERR_ARG
    assert "at least one observation" in abi.last_error()


def test_validate_batch_refuses_more_than_a_wavefront_of_parameters(abi):
    rc, *_ = _validate_batch(abi, k=65, p=63)
    assert rc == abi.ERR_UNSUPPORTED
    assert "FMCMC_MAX_K_WAVE = 64" in abi.last_error()


@pytest.mark.parametrize("kind,bw,freq,substr", [(7, 0, 1, "mirror kernels"), (8, 0, 1, "mirror kernels"),
                                                 (3, 5, 1, "bw = 0 and freq = 1"), (3, 0, 2, "bw = 0 and freq = 1")])
def test_validate_batch_refuses_the_kernels_out_of_scope(abi, kind, bw, freq, substr):
    rc, m, kk, r, keep = _validate_batch(abi, kind=kind, lb=[-1.0] * 3, ub=[1.0] * 3)
    kk.bw, kk.freq, kk.warmup = bw, freq, 10
    assert abi.lib().fmcmc_validate_batch(C.byref(m), 3, C.byref(kk), C.byref(r)) == abi.ERR_UNSUPPORTED
    assert substr in abi.last_error()


@pytest.mark.parametrize("nmodels,nchains,substr", [(0, 6, "`nmodels` must be at least 1"), (-2, 6, "`nmodels` must be at least 1"),
                                                    (4, 6, "must be a multiple of `nmodels` (4)")])
def test_validate_batch_refuses_a_bad_split_into_datasets(abi, nmodels, nchains, substr):
    rc, *_ = _validate_batch(abi, nmodels=nmodels, nchains=nchains)
    assert rc == abi.ERR_ARG
    assert substr in abi.last_error()


@pytest.mark.parametrize("entry", ["fmcmc_mcmc_run_batch_dev", "fmcmc_mcmc_run_batch_host"])
@pytest.mark.parametrize("xs,ys", [(9, 10), (10, 9), (0, 10)])
def test_strides_smaller_than_a_dataset_are_refused_before_any_device_call(abi, entry, xs, ys):
    """(p = 1, n = 10: a dataset is 10 doubles of X and 10 of y)"""
    m, kk, r, keep = _host_specs(abi, nchains=6)
    st, out = abi.State(), abi.Out()
    rc = getattr(abi.lib(), entry)(C.byref(m), 3, xs, ys, C.byref(kk), C.byref(r), C.byref(st), C.byref(out), 0, None if entry.endswith("dev") else 0)
    assert rc == abi.ERR_ARG
    assert "smaller than a dataset" in abi.last_error()


def test_validate_fun_still_refuses_what_it_refused(abi):
    m, kk, r, keep = _host_specs(abi, kind=7, lb=[-1.0] * 3, ub=[1.0] * 3)
    assert abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)) == abi.ERR_UNSUPPORTED
    assert "mirror kernels" in abi.last_error()
    m, kk, r, keep = _host_specs(abi, kind=3)
    kk.bw, kk.warmup = 5, 10
    assert abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)) == abi.ERR_UNSUPPORTED
    m, kk, r, keep = _host_specs(abi, k=300)
    assert abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)) == abi.ERR_UNSUPPORTED
    # k = 65 stays in the callback path's scope, and in fmcmc_validate's for a joint kernel
    m, kk, r, keep = _host_specs(abi, k=65, p=63)
    assert abi.lib().fmcmc_validate_fun(C.byref(kk), C.byref(r)) == abi.OK
    assert abi.lib().fmcmc_validate(C.byref(m), C.byref(kk), C.byref(r)) == abi.OK


def _data(D=3, n=20, p=2, seed=0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((n, p)), rng.standard_normal(n)) for _ in range(D)]


def test_model_batch_holds_the_datasets():
    import fmcmc_amd as F
    b = F.model_batch(F.gaussian_linreg(X, y) for X, y in _data())
    assert isinstance(b, F.ModelBatch) and b.nmodels == len(b) == 3 and b.k == 4
    assert b[1].p == 2 and b[1] is b.models[1]


def test_model_batch_names_the_field_that_differs():
    import fmcmc_amd as F
    (X0, y0), (X1, y1), _ = _data()
    base = F.gaussian_linreg(X0, y0)
    for other, field in [(F.gaussian_linreg(X1[:-1], y1[:-1]), "-n-"), (F.gaussian_linreg(X1[:, :1], y1), "-p-"),
                         (F.gaussian_linreg(X1, y1, intercept=False), "-intercept-"), (F.gaussian_linreg(X1, y1, guard=False), "-guard-"),
                         (F.logistic(X1, y1 > 0), "-family-")]:
        with pytest.raises(ValueError, match=field):
            F.model_batch([base, other])
    with pytest.raises(ValueError, match="-prior_div-"):
        F.model_batch([F.logistic(X0, y0 > 0, prior_div=8.0), F.logistic(X1, y1 > 0, prior_div=0.0)])
    with pytest.raises(ValueError, match="empty"):
        F.model_batch([])
    with pytest.raises(TypeError, match="models\\[1\\]"):
        F.model_batch([base, F.batched_fun(lambda th: th.sum(1), 4)])


def test_the_shapes_of_initial():
    from fmcmc_amd.mcmc import batch_initial
    D, Cm, k = 3, 2, 4
    v = np.arange(k, dtype=float)
    a, names = batch_initial(v, D, Cm)
    assert a.shape == (D * Cm, k) and (a == v).all() and names == ["par1", "par2", "par3", "par4"]
    m = np.arange(Cm * k, dtype=float).reshape(Cm, k)
    a, _ = batch_initial(m, D, Cm)
    assert a.shape == (D * Cm, k) and all((a[d * Cm:(d + 1) * Cm] == m).all() for d in range(D))
    t = np.arange(D * Cm * k, dtype=float).reshape(D, Cm, k)
    a, _ = batch_initial(t, D, Cm)
    assert a.shape == (D * Cm, k) and (a[3] == t[1, 1]).all()
    a, names = batch_initial(dict(b0=1.0, b1=2.0), D, Cm)
    assert a.shape == (D * Cm, 2) and names == ["b0", "b1"]
    with pytest.raises(ValueError, match="number of chains per dataset"):
        batch_initial(np.zeros((3, k)), D, Cm)
    with pytest.raises(ValueError, match="three-way"):
        batch_initial(np.zeros((2, Cm, k)), D, Cm)
    with pytest.raises(ValueError, match="length zero"):
        batch_initial([], D, Cm)


def test_a_previous_result_continues_from_each_chains_last_row():
    """(host tensors stand in for the device buffers: McmcBatch only slices them)"""
    import torch
    import fmcmc_amd as F
    from fmcmc_amd.mcmc import batch_initial
    D, Cm, k, S = 2, 3, 4, 5
    s = torch.arange(D * Cm * k * S, dtype=torch.float64).reshape(D * Cm, k, S)
    dc = F.DeviceChains(s, None, None, np.arange(1, S + 1), 1, ["a", "b", "c", "d"], 0, D * Cm)
    dc.accept_count = torch.zeros(D * Cm, dtype=torch.int64)
    ans = F.McmcBatch(dc, D, Cm)
    assert len(ans) == D and ans[1].samples.shape == (Cm, k, S) and ans[1].chain_base == Cm and ans[-1].chain_base == Cm
    assert ans[1].samples.data_ptr() == s[Cm:].data_ptr()          # a slice, no copy
    a, names = batch_initial(ans, D, Cm)
    assert names == ["a", "b", "c", "d"] and torch.equal(a, s[:, :, -1])
    host = ans.to_host()
    assert len(host) == D and all(isinstance(h, F.McmcList) and len(h) == Cm for h in host)
    assert (host[1][2].data == s[Cm + 2].numpy().T).all()
    with pytest.raises(ValueError, match="2 datasets x 3 chains"):
        batch_initial(ans, 3, 2)


def test_mcmc_batch_refusals_before_any_device_work():
    import fmcmc_amd as F
    b = F.model_batch(F.gaussian_linreg(X, y) for X, y in _data())
    with pytest.raises(ValueError, match="conv_checker"):
        F.MCMC_batch(np.zeros(4), b, 100, conv_checker=F.convergence_gelman(50))
    with pytest.raises(ValueError, match="kernel_new"):
        F.MCMC_batch(np.zeros(4), b, 100, kernel=F.kernel_new(lambda env: env.theta0))
    with pytest.raises(TypeError, match="model_batch"):
        F.MCMC_batch(np.zeros(4), F.gaussian_linreg(*_data()[0]), 100)
    with pytest.raises(ValueError, match="Incorrect length of -initial-"):
        F.MCMC_batch(np.zeros(5), b, 100, nchains=2)
    with pytest.raises(ValueError, match="-burnin-"):
        F.MCMC_batch(np.zeros(4), b, 100, burnin=100)
