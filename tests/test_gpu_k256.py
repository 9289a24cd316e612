"""128 < k <= 256 parameters (FMCMC_MAX_K 256) and the HBM form of mh_sweep_bigk ("big-k-hbm"): the chain's matrices in its own
Sigma square instead of LDS where they do not fit (kernel_adapt from 134, kernel_ram from 184 free parameters).  Everything
bitwise against the oracle: samples, draws, log-posteriors, acceptance, the carried state (Sigma, abs_iter, mean_prev) over
consecutive calls, chain statuses."""
import numpy as np
import pytest

from conftest import set_knob, synth_linreg
from test_gpu_parity import jitter_init, run_both

pytestmark = pytest.mark.gpu

# the LDS form's last sizes (free parameters): mh_bigk.hpp, bigk_lds_doubles against 160 KiB
LDS_LAST = {"adapt": 133, "ram": 183}


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fmcmc_amd import engine
    return engine


def _linreg(k, seed, n=None):
    p = k - 2
    beta = np.linspace(1.0, -1.0, p + 1)
    X, y = synth_linreg(n or 300 + k, p, seed, beta=beta, sigma=2.0)
    init = jitter_init(list(beta) + [2.0], 3, seed + 1)
    init[:, -1] = np.abs(init[:, -1])
    return X, y, init


def _expected(kind_name, kf):
    last = LDS_LAST.get(kind_name.split("_")[0])
    return "big-k-hbm" if last is not None and kf > last else "big-k"


@pytest.mark.parametrize("k", [150, 200, 256])
@pytest.mark.parametrize("kind_name", ["ram", "ram_bounded", "adapt", "normal_reflective", "unif"])
def test_up_to_256_parameters(E, O, k, kind_name):
    from fmcmc_amd import _abi as abi
    X, y, init = _linreg(k, 9000 + k)
    fixed = [False] * k
    fixed[5] = (k == 200)                        # one case with a fixed parameter (kf = k - 1) per kernel
    kf = k - int(fixed[5])
    if kind_name == "ram":
        run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=40, calls=2, fixed=fixed)
    elif kind_name == "ram_bounded":
        run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=30, calls=2, lb=-1.5, ub=2.5, fixed=fixed)
    elif kind_name == "adapt":
        run_both(E, O, O.FAM_LINREG, X, y, O.K_ADAPT, k, init, nsteps=30, calls=2, warmup=10, fixed=fixed)
    elif kind_name == "normal_reflective":
        run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL_REFLECTIVE, k, init, nsteps=50, burnin=4, thin=3, calls=2, scale=0.01,
                 lb=-3.0, ub=4.0, fixed=fixed)
    else:
        run_both(E, O, O.FAM_LINREG, X, y, O.K_UNIF, k, init, nsteps=50, calls=2, min_=-0.01, max_=0.012, fixed=fixed)
    assert abi.last_kernel() == _expected(kind_name, kf)


@pytest.mark.parametrize("kind_name,k", [("adapt", 133), ("adapt", 134), ("ram", 183), ("ram", 184)])
def test_lds_and_hbm_thresholds(E, O, kind_name, k):
    from fmcmc_amd import _abi as abi
    X, y, init = _linreg(k, 7000 + k)
    if kind_name == "adapt":
        run_both(E, O, O.FAM_LINREG, X, y, O.K_ADAPT, k, init, nsteps=30, warmup=8)
    else:
        run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=30)
    assert abi.last_kernel() == ("big-k" if k <= LDS_LAST[kind_name] else "big-k-hbm")


@pytest.mark.parametrize("k", [70, 100])
def test_forced_hbm_form_equals_the_lds_form(E, O, monkeypatch, k):
    """Knob bigkhbm=1: the HBM form where the LDS form runs by default -- both give the oracle's bits, hence each other's."""
    from fmcmc_amd import _abi as abi
    X, y, init = _linreg(k, 5000 + k)
    fixed = [False] * k
    fixed[2] = (k == 100)
    set_knob(monkeypatch, "bigkhbm", 1)
    run_both(E, O, O.FAM_LINREG, X, y, O.K_ADAPT, k, init, nsteps=40, calls=2, warmup=10, fixed=fixed)
    assert abi.last_kernel() == "big-k-hbm"
    run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=40, calls=2, fixed=fixed)
    assert abi.last_kernel() == "big-k-hbm"
    constr = np.ones((k, k))
    constr[k // 2:, :10] = 0.0                   # (kernel_ram's constr: Sigma <<- constr * Sigma after every update)
    run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=30, lb=-1.5, ub=2.5, constr=constr)
    assert abi.last_kernel() == "big-k-hbm"
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, k, init, nsteps=40, scale=0.01)
    assert abi.last_kernel() == "big-k-hbm"
    monkeypatch.delenv("FMCMC_AMD_DEBUG")
    run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=40, calls=2, fixed=fixed)
    assert abi.last_kernel() == "big-k"


def test_constr_on_the_lds_form(E, O):
    """kernel_ram's constr with the packed triangles in LDS (the forced HBM form has it above), with and without bounds."""
    from fmcmc_amd import _abi as abi
    k = 70
    X, y, init = _linreg(k, 5070, n=200)
    constr = np.ones((k, k))
    constr[k // 2:, :10] = 0.0
    for kw in (dict(), dict(lb=-1.5, ub=2.5)):
        run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=30, constr=constr, **kw)
        assert abi.last_kernel() == "big-k"


# ---- the edges of the row owner's arithmetic at the fewest rows beyond a wavefront, k = 65; 3 chains, n = 200
def _form(monkeypatch, form):
    if form == "big-k-hbm":
        set_knob(monkeypatch, "bigkhbm", 1)


def _status_as_the_oracle(rg, ro):
    assert np.array_equal(rg.status_step.cpu().numpy(), ro.status_step)
    bad = ro.status != 0
    assert np.array_equal(rg.status_theta.cpu().numpy()[bad].view(np.uint64), np.ascontiguousarray(ro.status_theta[bad]).view(np.uint64))


NOT_PD_CASES = {"eps_negative": dict(eps=-1e-4), "warmup_0": dict(warmup=0)}


def not_pd_inputs(case):
    X, y, init = _linreg(65, 6500, n=200)
    return X, y, init, 12, NOT_PD_CASES[case]


def not_pd_in_the_oracle(case, ro):
    """every chain of eps < 0 (the first pivot is negative: step 2) and at least one of warmup = 0 ends NOT_PD: not vacuous"""
    bad = ro.status == 3
    assert bad.all() if case == "eps_negative" else bad.any()
    if case == "eps_negative":
        assert (ro.status_step == 2).all()


@pytest.mark.parametrize("form", ["big-k", "big-k-hbm"])
@pytest.mark.parametrize("case", list(NOT_PD_CASES))
def test_not_positive_definite_is_the_oracles_status(E, O, monkeypatch, case, form):
    """FMCMC_CHAIN_NOT_PD: the uniform early exit from the Cholesky's column loop, between its barriers"""
    from fmcmc_amd import _abi as abi
    X, y, init, nsteps, kw = not_pd_inputs(case)
    _form(monkeypatch, form)
    rg, ro = run_both(E, O, O.FAM_LINREG, X, y, O.K_ADAPT, 65, init, nsteps=nsteps, precheck=lambda ro: not_pd_in_the_oracle(case, ro), **kw)
    assert abi.last_kernel() == form
    _status_as_the_oracle(rg, ro)


EDGE_KERNELS = {"ram": ("K_RAM", 80, dict()), "ram_bounded": ("K_RAM", 80, dict(lb=-1.5, ub=2.5)), "adapt": ("K_ADAPT", 40, dict(warmup=5))}


def edge_inputs(kind_name, kf):
    """kf = 1: a scan of zero levels and a 1 x 1 factor (one free coefficient); kf = 64 < k: one fixed parameter"""
    X, y, init = _linreg(65, 6600 + kf, n=200)
    kind, nsteps, kw = EDGE_KERNELS[kind_name]
    fixed = [j != 3 for j in range(65)] if kf == 1 else [j == 5 for j in range(65)]
    return X, y, init, kind, nsteps, dict(kw, fixed=fixed)


def edge_in_the_oracle(ro, nsteps):
    """at least one accepted and one rejected step, every chain alive"""
    assert (ro.status == 0).all()
    assert 0 < ro.accept_count.sum() < ro.accept_count.size * (nsteps - 1)


@pytest.mark.parametrize("form", ["big-k", "big-k-hbm"])
@pytest.mark.parametrize("kf", [1, 64])
@pytest.mark.parametrize("kind_name", list(EDGE_KERNELS))
def test_fewest_rows_beyond_a_wavefront(E, O, monkeypatch, kind_name, kf, form):
    from fmcmc_amd import _abi as abi
    X, y, init, kind, nsteps, kw = edge_inputs(kind_name, kf)
    kind = getattr(O, kind)
    _form(monkeypatch, form)
    rg, ro = run_both(E, O, O.FAM_LINREG, X, y, kind, 65, init, nsteps=nsteps, precheck=lambda ro: edge_in_the_oracle(ro, nsteps), **kw)
    assert abi.last_kernel() == form
    _status_as_the_oracle(rg, ro)


def test_logistic_regression_with_200_parameters(E, O):
    """The all-family evaluation (g table, scaled coefficient copies, data-only sums) beside the HBM form."""
    from fmcmc_amd import _abi as abi
    rng = np.random.default_rng(200)
    n, p = 600, 199
    X = rng.standard_normal((n, p)) * 0.2
    beta = rng.uniform(-0.5, 0.5, p + 1)
    y = (rng.uniform(size=n) < 1 / (1 + np.exp(-(beta[0] + X @ beta[1:])))).astype(np.float64)
    init = jitter_init(beta, 3, 201)
    run_both(E, O, O.FAM_LOGISTIC, X, y, O.K_NORMAL, p + 1, init, nsteps=40, calls=2, prior_div=8.0, scale=0.01)
    assert abi.last_kernel() == "big-k"
    run_both(E, O, O.FAM_LOGISTIC, X, y, O.K_RAM, p + 1, init, nsteps=30, calls=2, prior_div=8.0)
    assert abi.last_kernel() == "big-k-hbm"


def test_300_chains_at_200_parameters(E, O):
    """More chains than CUs: the HBM form's workgroups in consecutive rounds, each XCD's chains sharing its L2."""
    from fmcmc_amd import _abi as abi
    k = 200
    X, y, _ = _linreg(k, 300, n=400)
    init = jitter_init(list(np.linspace(1.0, -1.0, k - 1)) + [2.0], 300, 301)
    init[:, -1] = np.abs(init[:, -1])
    run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=30, calls=2, threads=8)
    assert abi.last_kernel() == "big-k-hbm"


@pytest.mark.parametrize("kind_name,k", [("ram", 200), ("normal", 150)])
def test_nan_log_posterior_status_above_128(E, O, kind_name, k):
    """The unguarded linear model (README.md:356-361): sigma below zero -> NaN -> chain status 1 at the oracle's step, with the
    oracle's theta; the other chains go on."""
    from fmcmc_amd import _abi as abi
    X, y, init = _linreg(k, 4000 + k)
    init[:, -1] = [0.004, 2.0, 0.003]
    if kind_name == "ram":
        rg, ro = run_both(E, O, O.FAM_LINREG, X, y, O.K_RAM, k, init, nsteps=60, guard=False, eps=0.01)
    else:
        rg, ro = run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, k, init, nsteps=60, guard=False, scale=0.01)
    assert abi.last_kernel() == ("big-k-hbm" if kind_name == "ram" else "big-k")
    assert (ro.status == 1).any() and (ro.status == 0).any()
    assert np.array_equal(rg.status_step.cpu().numpy(), ro.status_step)
    bad = ro.status != 0
    assert np.array_equal(rg.status_theta.cpu().numpy()[bad].view(np.uint64), np.ascontiguousarray(ro.status_theta[bad]).view(np.uint64))


def test_mcmc_with_200_parameters_kernel_adapt_and_the_gelman_checker(E, O):
    """MCMC(..., kernel_adapt(), conv_checker = convergence_gelman()) at k = 200: the chains on the HBM form, the checker's
    window statistics from the host-side torch path -- R-hat history and samples as the oracle's.  (A window of fewer
    distinct rows than parameters has a singular within-chain covariance: gelman.diag fails there, the library skips the
    check with a warning and the oracle records NaN.)"""
    import fmcmc_amd as f
    from fmcmc_amd import _abi as abi
    k, nsteps, freq = 200, 800, 400
    X, y = synth_linreg(500, k - 2, 12, beta=np.linspace(1.0, -1.0, k - 1), sigma=2.0)
    init = np.tile(np.r_[np.linspace(1.0, -1.0, k - 1), 2.0], (3, 1)) + 0.02 * np.random.default_rng(4).standard_normal((3, k))
    init[:, -1] = np.abs(init[:, -1])
    chk = f.convergence_gelman(freq, threshold=1.5)
    ans = f.MCMC(init, f.gaussian_linreg(X, y), nsteps, seed=7, nchains=3, kernel=f.kernel_adapt(warmup=20), conv_checker=chk)
    assert abi.last_kernel() == "big-k-hbm"
    ro = O.mcmc_with_conv_checker(O.Model(O.FAM_LINREG, X, y), O.Kernel(O.K_ADAPT, k, warmup=20), init, nsteps, 3, freq, seed=7,
                                  threshold=1.5)
    oh = [h for h in ro.history if np.isfinite(h[1])]
    assert [h[0] for h in chk.history] == [h[0] for h in oh] and len(oh) >= 1
    assert np.allclose([h[1] for h in chk.history], [h[1] for h in oh], rtol=1e-7)
    assert np.array_equal(np.ascontiguousarray(ans.as_array()).view(np.uint64), np.ascontiguousarray(ro.samples).view(np.uint64))
