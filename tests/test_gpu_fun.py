"""User-defined log-posteriors through a batched callback (batched_fun -> fmcmc_mcmc_run_fun_dev, mh_fun.hpp) on the GPU.

With `fun` = the oracle's own canonical log-posterior, evaluated row by row on the host, every output is bitwise the oracle's
and the family path's: samples, draws, logpost, acceptance, statuses and the carried state.  A model outside the families
(the multivariate-normal mean of the reference's benchmark, k = 100, n = 500) is replayed step by step from its outputs."""
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


def host_fun(om, counter=None):
    """fn(theta [C, k] on the device) = the oracle's canonical logpost of every row, as a device tensor"""
    import torch

    def fn(th):
        if counter is not None:
            counter.append(th.shape[0])
        rows = th.cpu().numpy()
        return torch.tensor([om.logpost(r) for r in rows], dtype=torch.float64, device=th.device)
    return fn


def _model(k, seed):
    if k == 2:   # iid Normal(mu, sigma)
        rng = np.random.default_rng(seed)
        return 3, None, 2.0 + 1.5 * rng.standard_normal(200), np.array([[2.0, 1.5]])
    p = k - 2
    beta = np.linspace(1.0, -1.0, p + 1)
    X, y = synth_linreg(120 + 2 * k, p, seed, beta=beta, sigma=2.0)
    return 1, X, y, np.array([list(beta) + [2.0]])


def fun_inputs(k, nchains, seed=77):
    """the model and the initial values run_fun_both works on"""
    fam, X, y, base = _model(k, 100 + k)
    init = jitter_init(base[0], nchains, seed + k)
    init[:, -1] = np.abs(init[:, -1]) + 0.5
    return fam, X, y, init


def run_fun_both(E, O, k, kind, nchains=4, nsteps=60, calls=2, burnin=0, thin=1, seed=77, chain_base=0, shards=1, precheck=None, **kw):
    """`calls` consecutive calls of the callback path against the oracle (and the first against the family path), bitwise.
    precheck(ro): what a test asserts of the oracle's result alone, before the GPU runs."""
    import torch
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.models import batched_fun
    fam, X, y, init = fun_inputs(k, nchains, seed)
    om = O.Model(fam, X, y)
    ok = O.Kernel(kind, k, **kw)
    spec = lambda: E.KernelSpec(kind, k, ok.mu, ok.scale, ok.lb, ok.ub, ok.fixed, scheme=ok.scheme, freq=ok.freq,
                                warmup=ok.warmup, until=ok.until, eps=ok.eps, arate=ok.arate, scheme_seq=ok.scheme_seq,
                                constr=ok.constr, ram_qfun=ok.ram_qfun, ram_df=ok.ram_df, ram_eta_exp=ok.ram_eta_exp)
    gf = E.DeviceFun(batched_fun(host_fun(om), k))
    cuts = np.linspace(0, nchains, shards + 1).astype(int)
    parts = [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]
    gk = spec()
    gsts = [E.ChainState(init[a:b], ok.kf) for a, b in parts]
    ost = O.ChainState(init, ok.kf)
    for call in range(calls):
        ro = O.run(om, ok, nsteps=nsteps, burnin=burnin, thin=thin, seed=seed, chain_base=chain_base, state=ost)
        if precheck is not None:
            precheck(ro)
        for (a, b), gst in zip(parts, gsts):
            rg = E.sweep(gf, gk, gst, nsteps, burnin=burnin, thin=thin, seed=seed, chain_base=chain_base + a, check=False)
            torch.cuda.synchronize()
            assert abi.last_kernel() == ("fun" if k <= 64 else "fun-wg")
            sl = slice(a, b)
            assert np.array_equal(rg.status.cpu().numpy(), ro.status[sl])
            assert np.array_equal(rg.status_step.cpu().numpy(), ro.status_step[sl])
            bad = ro.status[sl] != 0
            assert _bits_equal(rg.status_theta.cpu().numpy()[bad], ro.status_theta[sl][bad]), "status_theta"
            assert np.array_equal(rg.accept_bits.cpu().numpy().view(np.uint32), ro.accept_bits[sl]), "accept bitmap"
            assert np.array_equal(rg.accept_count.cpu().numpy(), ro.accept_count[sl])
            good = ro.status[sl] == 0
            assert _bits_equal(rg.samples.cpu().numpy()[good], ro.samples_cks[sl][good]), "samples"
            assert _bits_equal(rg.draws.cpu().numpy()[good], ro.draws_cks[sl][good]), "draws"
            assert _bits_equal(rg.logpost.cpu().numpy()[good], ro.logpost[sl][good]), "logpost"
            assert _bits_equal(gst.theta0.cpu().numpy(), ost.theta0[sl])
            assert _bits_equal(gst.f0.cpu().numpy()[good], ost.f0[sl][good])
            if kind in (O.K_ADAPT, O.K_RAM):
                assert np.array_equal(gst.abs_iter.cpu().numpy(), ost.abs_iter[sl])
                assert _bits_equal(gst.Sigma.cpu().numpy(), ost.Sigma[sl]), "Sigma"
                assert np.array_equal(gst.nerrors.cpu().numpy(), ost.nerrors[sl])
            if kind == O.K_ADAPT:
                assert np.array_equal(gst.have_mean.cpu().numpy(), ost.have_mean[sl])
                hm = ost.have_mean[sl].astype(bool)
                assert _bits_equal(gst.mean_prev.cpu().numpy()[hm], ost.mean_prev[sl][hm])
            if ok.scheme == O.SCHEME_RANDOM:
                assert np.array_equal(gst.scheme_cols.cpu().numpy()[:, 1:nsteps], ost.scheme_cols[sl, 1:nsteps])
            family = not (k > 64 and kind not in (O.K_ADAPT, O.K_RAM) and ok.scheme != O.SCHEME_JOINT)   # (what it runs)
            if call == 0 and shards == 1 and family:   # the family path on the same call: the same bits
                fst = E.ChainState(init[a:b], ok.kf)
                rf = E.sweep(E.DeviceModel(fam, X, y), spec(), fst, nsteps, burnin=burnin, thin=thin, seed=seed,
                             chain_base=chain_base + a, check=False)
                torch.cuda.synchronize()
                fg = rf.status.cpu().numpy() == 0
                assert _bits_equal(rf.samples.cpu().numpy()[fg], ro.samples_cks[sl][fg]), "family path"
    return ro


K_SMALL = [3, 5, 64]
CASES = [
    ("normal", dict(scale=0.05)),
    ("normal_ordered", dict(scale=0.1, scheme=1)),
    ("normal_random", dict(scale=0.1, scheme=2)),
    ("normal_explicit", dict(scale=0.1, scheme=3)),
    ("normal_reflective", dict(scale=0.05, lb=-2.0, ub=3.0)),
    ("unif", dict(min_=-0.05, max_=0.06)),
    ("unif_reflective_ordered", dict(min_=-0.1, max_=0.1, lb=-2.0, ub=3.0, scheme=1)),
    ("adapt", dict(warmup=10)),
    ("ram", dict()),
    ("ram_bounded_constr", dict(lb=-2.0, ub=3.0, constr=True)),
    ("ram_normal_qfun_freq", dict(ram_qfun=1, freq=2, warmup=5, until=40)),
    ("ram_tdf", dict(ram_qfun=2, ram_df=3.5, ram_eta_exp=0.8)),
]


def _kind_kw(O, name, k, kw):
    kw = dict(kw)
    kind = {"normal": O.K_NORMAL, "unif": O.K_UNIF, "adapt": O.K_ADAPT, "ram": O.K_RAM}[name.split("_")[0]]
    if "reflective" in name:
        kind = O.K_NORMAL_REFLECTIVE if kind == O.K_NORMAL else O.K_UNIF_REFLECTIVE
    sch = kw.pop("scheme", 0)
    if sch:   # (the oracle's Kernel takes R's form: a name, or the 1-based sequence of an explicit plan)
        kw["scheme"] = {1: "ordered", 2: "random", 3: list(range(k, 0, -1))}[sch]
    if kw.pop("constr", False):
        kw["constr"] = np.tril(np.ones((k, k)))
    return kind, kw


@pytest.mark.parametrize("k", K_SMALL)
@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_bitwise_against_the_oracle(E, O, name, kw, k):
    kind, kw = _kind_kw(O, name, k, kw)
    run_fun_both(E, O, k, kind, nsteps=60 if k < 64 else 30, **kw)


@pytest.mark.parametrize("k", [65, 130, 256])
@pytest.mark.parametrize("name,kw", [c for c in CASES if c[0] in ("normal", "normal_ordered", "unif_reflective_ordered",
                                                                  "adapt", "ram", "ram_bounded_constr")],
                         ids=["normal", "normal_ordered", "unif_reflective_ordered", "adapt", "ram", "ram_bounded_constr"])
def test_bitwise_above_a_wavefront(E, O, name, kw, k):
    kind, kw = _kind_kw(O, name, k, kw)
    if kind == O.K_NORMAL and "scheme" not in kw and k == 130:
        kw["fixed"] = [j == 7 for j in range(k)]
    run_fun_both(E, O, k, kind, nchains=3, nsteps=25, **kw)


NOT_PD_CASES = {"eps_negative": dict(eps=-1e-4), "warmup_0": dict(warmup=0)}


def not_pd_in_the_oracle(case, ro):
    """every chain of eps < 0 (the first pivot is negative: step 2) and at least one of warmup = 0 ends NOT_PD: not vacuous"""
    bad = ro.status == 3
    assert bad.all() and (ro.status_step == 2).all() if case == "eps_negative" else bad.any()


@pytest.mark.parametrize("k", [5, 64, 65])
@pytest.mark.parametrize("case", list(NOT_PD_CASES))
def test_not_positive_definite_is_the_oracles_status(E, O, case, k):
    """FMCMC_CHAIN_NOT_PD from the LDL^T factor ("fun", k = 5 and 64) and from the row owner's Cholesky ("fun-wg", k = 65: the
    uniform early exit between its barriers); the form (fmcmc_last_kernel), status, status_step and status_theta are
    run_fun_both's assertions"""
    run_fun_both(E, O, k, O.K_ADAPT, nchains=3, nsteps=12, calls=1, precheck=lambda ro: not_pd_in_the_oracle(case, ro), **NOT_PD_CASES[case])


# the fewest rows beyond a wavefront, k = 65: one free parameter (a scan of zero levels, a 1 x 1 factor) and 64 of them
EDGE_KERNELS = {"ram": ("K_RAM", 80, dict()), "ram_bounded": ("K_RAM", 80, dict(lb=-2.0, ub=3.0)), "adapt": ("K_ADAPT", 40, dict(warmup=5))}
EDGE_SEED = 87   # (of the seeds 77 .. 91, one at which the oracle rejects a step in each of the six cases)


def edge_case(kind_name, kf):
    kind, nsteps, kw = EDGE_KERNELS[kind_name]
    return kind, nsteps, dict(kw, fixed=[j != 3 for j in range(65)] if kf == 1 else [j == 5 for j in range(65)])


def edge_in_the_oracle(ro, nsteps):
    """at least one accepted and one rejected step, every chain alive"""
    assert (ro.status == 0).all()
    assert 0 < ro.accept_count.sum() < ro.accept_count.size * (nsteps - 1)


@pytest.mark.parametrize("kf", [1, 64])
@pytest.mark.parametrize("kind_name", list(EDGE_KERNELS))
def test_fewest_rows_beyond_a_wavefront(E, O, kind_name, kf):
    kind, nsteps, kw = edge_case(kind_name, kf)
    kind = getattr(O, kind)
    run_fun_both(E, O, 65, kind, nchains=3, nsteps=nsteps, calls=1, seed=EDGE_SEED, precheck=lambda ro: edge_in_the_oracle(ro, nsteps), **kw)


@pytest.mark.parametrize("kind_name", ["normal", "adapt", "ram_bounded"])
def test_fixed_parameters_thinning_and_iid_normal(E, O, kind_name):
    kind = {"normal": O.K_NORMAL, "adapt": O.K_ADAPT, "ram_bounded": O.K_RAM}[kind_name]
    kw = dict(fixed=[False, True, False, False, False])
    if kind_name == "ram_bounded":
        kw.update(lb=-2.0, ub=3.0)
    if kind_name == "adapt":
        kw.update(warmup=8)
    run_fun_both(E, O, 5, kind, nsteps=80, burnin=10, thin=3, **kw)
    run_fun_both(E, O, 2, O.K_NORMAL, nsteps=100, scale=0.1)


@pytest.mark.parametrize("k", [5, 130])
def test_chain_base_split_into_two_shards(E, O, k):
    run_fun_both(E, O, k, O.K_RAM, nchains=6, nsteps=30, shards=2, lb=-2.0, ub=3.0)


@pytest.mark.parametrize("kind_name,per_step", [("normal", 1), ("ram", 1), ("ram_bounded", 2), ("adapt", 1)])
def test_call_counts(E, O, kind_name, per_step):
    import fmcmc_amd as F
    from fmcmc_amd.models import batched_fun
    om = O.Model(1, *synth_linreg(200, 1, 3))
    calls = []
    kern = {"normal": lambda: F.kernel_normal(scale=0.05), "ram": lambda: F.kernel_ram(),
            "ram_bounded": lambda: F.kernel_ram(lb=-10.0, ub=10.0), "adapt": lambda: F.kernel_adapt(warmup=5)}[kind_name]()
    nsteps = 50
    F.MCMC(np.array([3.0, 2.0, 4.0]), batched_fun(host_fun(om, calls), 3), nsteps, nchains=3, seed=5, kernel=kern)
    assert len(calls) == 1 + per_step * (nsteps - 1)
    assert set(calls) == {3}


def _mvn(n=500, k=100, seed=11):
    import torch
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((n, k)) + np.linspace(-1, 1, k)[None, :]
    Yt = torch.tensor(Y, dtype=torch.float64, device="cuda")

    def fn(th):   # sum_i log N(y_i | mu, I) up to a constant (playground/benchmarks.Rmd: the mean of a 100-dimension normal)
        return -0.5 * ((Yt[None, :, :] - th[:, None, :]) ** 2).sum(dim=(1, 2))
    return Y, fn


def test_a_model_outside_the_families_kernel_normal_replayed(E):
    """k = 100, n = 500, fn in pure torch: every draw, accept bit and logpost replayed from the recorded outputs"""
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    Y, fn = _mvn()
    k, C, nsteps, scale, seed = 100, 8, 300, 0.004, 31
    ybar = Y.mean(0)
    init = ybar[None, :] + 0.02 * np.random.default_rng(1).standard_normal((C, k))
    f = F.batched_fun(fn, k)
    kern = F.kernel_normal(scale=scale)
    dc = F.MCMC(init, f, nsteps, nchains=C, seed=seed, kernel=kern, _return_device=True)
    assert abi.last_kernel() == "fun-wg"
    S = dc.samples.cpu().numpy()      # [C][k][nsteps]
    D = dc.draws.cpu().numpy()
    L = dc.logpost.cpu().numpy()
    # the variates of the call (step_base 0): fmcmc_rng_stream_dev
    st = E.ChainState(init, k)
    logu, z = E.rng_stream(st, kern._spec, nsteps, seed=seed)
    logu, z = logu.cpu().numpy(), z.cpu().numpy()
    for c in range(C):
        f0 = L[c, 0]
        assert _bits_equal(S[c, :, 0], init[c]) and _bits_equal(D[c, :, 0], init[c])
        for i in range(2, nsteps + 1):
            prop = S[c, :, i - 2] + (0.0 + scale * z[c, i - 1, :])
            assert _bits_equal(D[c, :, i - 1], prop), (c, i)
            f1 = L[c, i - 1]
            acc = logu[c, i - 1] < f1 - f0
            assert _bits_equal(S[c, :, i - 1], prop if acc else S[c, :, i - 2]), (c, i)
            if acc:
                f0 = f1
    ref = fn(torch.tensor(D.transpose(0, 2, 1).reshape(-1, k), device="cuda")).cpu().numpy().reshape(C, nsteps)
    assert np.allclose(L, ref, rtol=1e-12, atol=0)


def test_a_model_outside_the_families_kernel_ram(E):
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    Y, fn = _mvn()
    k, C = 100, 8
    ybar = Y.mean(0)
    init = ybar[None, :] + 0.05 * np.random.default_rng(2).standard_normal((C, k))
    ans = F.MCMC(init, F.batched_fun(fn, k), 1500, nchains=C, seed=3, kernel=F.kernel_ram(warmup=100), burnin=500)
    assert abi.last_kernel() == "fun-wg"
    arr = ans.as_array()              # [C][S][k]
    assert np.isfinite(arr).all()
    # the posterior of mu is N(ybar, I / n): sd 0.045 per coordinate
    assert np.abs(arr.mean(axis=(0, 1)) - ybar).max() < 0.1


def test_nan_from_fn_gives_chain_status_1(E, O):
    import torch
    from fmcmc_amd.models import batched_fun
    om = O.Model(1, *synth_linreg(200, 1, 4))
    calls = []

    def fn(th):
        f = host_fun(om)(th)
        calls.append(th.clone())
        if len(calls) == 7:
            f[1] = float("nan")
        return f
    init = np.array([[3.0, 2.0, 4.0]] * 3) + 0.01 * np.arange(9).reshape(3, 3)
    ok = O.Kernel(O.K_NORMAL, 3, scale=0.05)
    gk = E.KernelSpec(O.K_NORMAL, 3, ok.mu, ok.scale, ok.lb, ok.ub, ok.fixed)
    st = E.ChainState(init, 3)
    rg = E.sweep(E.DeviceFun(batched_fun(fn, 3)), gk, st, 20, seed=2, check=False)
    torch.cuda.synchronize()
    assert rg.status.cpu().numpy().tolist() == [0, 1, 0]
    assert int(rg.status_step[1]) == 7
    assert _bits_equal(rg.status_theta[1].cpu().numpy(), calls[6][1].cpu().numpy())
    with pytest.raises(RuntimeError, match="fun\\(par\\) is undefined"):
        E.raise_on_chain_error(rg)


def test_an_exception_in_fn_is_raised_again_and_the_device_stays_usable(E):
    import torch
    import fmcmc_amd as F
    n = []

    def bad(th):
        n.append(1)
        if len(n) == 4:
            raise KeyError("boom at call 4")
        return -(th ** 2).sum(1)
    with pytest.raises(KeyError, match="boom at call 4"):
        F.MCMC(np.zeros((4, 3)), F.batched_fun(bad, 3), 100, nchains=4, seed=1)
    ans = F.MCMC(np.zeros((4, 3)), F.batched_fun(lambda th: -(th ** 2).sum(1), 3), 100, nchains=4, seed=1)
    assert np.isfinite(ans.as_array()).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("bad", ["shape", "dtype", "type"])
def test_a_wrong_return_raises_value_error(E, bad):
    import torch
    import fmcmc_amd as F
    fn = {"shape": lambda th: th.sum(1, keepdim=True), "dtype": lambda th: th.sum(1).float(),
          "type": lambda th: th.sum(1).cpu().numpy()}[bad]
    with pytest.raises(ValueError, match="batched_fun"):
        F.MCMC(np.zeros((2, 3)), F.batched_fun(fn, 3), 50, nchains=2, seed=1)
    torch.cuda.synchronize()


def test_auto_stop_matches_the_family_path(E, O):
    """convergence_gelman through batched_fun stops at the same bulk as the family path, with the same R-hat history"""
    import fmcmc_amd as F
    X, y = synth_linreg(300, 1, 8)
    om = O.Model(1, X, y)
    init = np.array([[3.0, 2.0, 4.0]] * 4) + 0.2 * np.random.default_rng(3).standard_normal((4, 3))
    res = []
    for fun in (F.gaussian_linreg(X, y), F.batched_fun(host_fun(om), 3)):
        chk = F.convergence_gelman(200, threshold=1.2)
        ans = F.MCMC(init, fun, 2000, nchains=4, seed=9, kernel=F.kernel_ram(), conv_checker=chk)
        res.append((ans.as_array(), list(chk.history)))
    assert res[0][0].shape == res[1][0].shape
    assert _bits_equal(res[0][0], res[1][0])
    (a, b) = (res[0][1], res[1][1])
    assert len(a) == len(b) >= 1
    for (ea, va, pa), (eb, vb, pb) in zip(a, b):
        assert ea == eb and _bits_equal(va, vb) and _bits_equal(pa, pb)
