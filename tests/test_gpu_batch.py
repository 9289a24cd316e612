"""One model on many datasets in one launch (engine.sweep_batch -> fmcmc_mcmc_run_batch_dev, mh_batch.hpp; MCMC_batch) on the GPU.

Every case is bitwise the oracle's: the oracle is run once per dataset with the chains' global ids (chain_base + d Cm) and its
results are laid side by side; samples, draws, logpost, accept bitmap and counts, statuses, status_step, status_theta, theta0,
f0, abs_iter, Sigma, mean_prev, have_mean, nerrors and scheme_cols are compared, after each of the consecutive calls.  The
oracle of a case runs once and serves both data forms ("batch-lds", "batch-stream")."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth_linreg
from test_gpu_fun import CASES, _kind_kw
from test_gpu_host_entries import P, abi_kernel, abi_state_out, host_bufs, synth_logistic
from test_gpu_parity import _bits_equal, jitter_init

pytestmark = pytest.mark.gpu

LINREG, LOGISTIC, IID = 1, 2, 3
FORMS = {False: "batch-lds", True: "batch-stream"}


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fmcmc_amd import engine
    return engine


def linreg_data(D, n, p, seed):
    """D datasets of one linear model and the point the chains start around"""
    beta = np.linspace(1.0, -1.0, p + 1)
    sets = [synth_linreg(n, p, seed + 31 * d, beta=beta, sigma=2.0) for d in range(D)]
    return np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]), np.array(list(beta) + [2.0])


def start_points(base, nch, seed, sigma_last=True):
    init = jitter_init(base, nch, seed)
    if sigma_last:
        init[:, -1] = np.abs(init[:, -1]) + 0.5
    return init


class Case:
    """A batch, a kernel and the oracle's results of `calls` consecutive calls, dataset by dataset"""

    def __init__(self, O, fam, Xs, ys, kind, init, Cm, nsteps, calls=1, burnin=0, thin=1, seed=77, chain_base=0, model_kw=None, **kw):
        self.fam, self.Xs, self.ys, self.Cm, self.D = fam, Xs, np.asarray(ys), Cm, len(ys)
        self.nsteps, self.calls, self.burnin, self.thin, self.seed, self.chain_base = nsteps, calls, burnin, thin, seed, chain_base
        self.model_kw = dict(model_kw or {})
        self.init = np.ascontiguousarray(init, dtype=np.float64)
        assert self.init.shape[0] == self.D * Cm
        k = self.init.shape[1]
        self.ok = ok = O.Kernel(kind, k, **kw)
        self.O = O
        oms = [O.Model(fam, None if Xs is None else Xs[d], ys[d], **self.model_kw) for d in range(self.D)]
        osts = [O.ChainState(self.init[d * Cm:(d + 1) * Cm], ok.kf) for d in range(self.D)]
        self.refs = []
        for _ in range(calls):
            ros = [O.run(oms[d], ok, nsteps=nsteps, burnin=burnin, thin=thin, seed=seed, chain_base=chain_base + d * Cm, state=osts[d])
                   for d in range(self.D)]
            cat = lambda f, src: np.concatenate([f(s) for s in src])
            ref = dict(status=cat(lambda r: r.status, ros), status_step=cat(lambda r: r.status_step, ros),
                       status_theta=cat(lambda r: r.status_theta, ros), accept_bits=cat(lambda r: r.accept_bits, ros),
                       accept_count=cat(lambda r: r.accept_count, ros), samples=cat(lambda r: r.samples_cks, ros),
                       draws=cat(lambda r: r.draws_cks, ros), logpost=cat(lambda r: r.logpost, ros),
                       theta0=cat(lambda s: s.theta0, osts), f0=cat(lambda s: s.f0, osts), abs_iter=cat(lambda s: s.abs_iter, osts),
                       Sigma=cat(lambda s: s.Sigma, osts), nerrors=cat(lambda s: s.nerrors, osts),
                       have_mean=cat(lambda s: s.have_mean, osts), mean_prev=cat(lambda s: s.mean_prev, osts))
            if ok.scheme == O.SCHEME_RANDOM:
                ref["scheme_cols"] = cat(lambda s: s.scheme_cols, osts)
            self.refs.append(ref)

    def spec(self, E):
        ok = self.ok
        return E.KernelSpec(ok.kind, ok.k, ok.mu, ok.scale, ok.lb, ok.ub, ok.fixed, scheme=ok.scheme, freq=ok.freq, warmup=ok.warmup,
                            until=ok.until, eps=ok.eps, arate=ok.arate, scheme_seq=ok.scheme_seq, constr=ok.constr,
                            ram_qfun=ok.ram_qfun, ram_df=ok.ram_df, ram_eta_exp=ok.ram_eta_exp)

    def batch(self, E, datasets=None, ys=None):
        ds = slice(None) if datasets is None else datasets
        ys = self.ys if ys is None else ys
        return E.DeviceModelBatch(self.fam, None if self.Xs is None else self.Xs[ds], ys[ds], **self.model_kw)

    def assert_call(self, rg, gst, call, chains=slice(None)):
        """the outputs of one device call and the state it left against the oracle's, for the chains `chains` of the case"""
        O, ok, ref = self.O, self.ok, {f: v[chains] for f, v in self.refs[call].items()}
        cpu = lambda t: t.cpu().numpy()
        assert np.array_equal(cpu(rg.status), ref["status"]), "status"
        assert np.array_equal(cpu(rg.status_step), ref["status_step"]), "status_step"
        bad, good = ref["status"] != 0, ref["status"] == 0
        assert _bits_equal(cpu(rg.status_theta)[bad], ref["status_theta"][bad]), "status_theta"
        assert np.array_equal(cpu(rg.accept_bits).view(np.uint32), ref["accept_bits"]), "accept bitmap"
        assert np.array_equal(cpu(rg.accept_count), ref["accept_count"]), "accept counts"
        assert _bits_equal(cpu(rg.samples)[good], ref["samples"][good]), "samples"
        assert _bits_equal(cpu(rg.draws)[good], ref["draws"][good]), "draws"
        assert _bits_equal(cpu(rg.logpost)[good], ref["logpost"][good]), "logpost"
        assert _bits_equal(cpu(gst.theta0), ref["theta0"]), "theta0"
        assert _bits_equal(cpu(gst.f0)[good], ref["f0"][good]), "f0"
        if ok.kind in (O.K_ADAPT, O.K_RAM):
            assert np.array_equal(cpu(gst.abs_iter), ref["abs_iter"]), "abs_iter"
            assert _bits_equal(cpu(gst.Sigma), ref["Sigma"]), "Sigma"
            assert np.array_equal(cpu(gst.nerrors), ref["nerrors"]), "nerrors"
        if ok.kind == O.K_ADAPT:
            assert np.array_equal(cpu(gst.have_mean), ref["have_mean"]), "have_mean"
            hm = ref["have_mean"].astype(bool)
            assert _bits_equal(cpu(gst.mean_prev)[hm], ref["mean_prev"][hm]), "mean_prev"
        if ok.scheme == O.SCHEME_RANDOM:
            assert np.array_equal(cpu(gst.scheme_cols)[:, 1:self.nsteps], ref["scheme_cols"][:, 1:self.nsteps]), "scheme_cols"

    def check(self, E, stream_data=False, form=None, fed=False):
        """`calls` consecutive sweep_batch calls with the carried state, each against the oracle's"""
        import torch
        from fmcmc_amd import _abi as abi
        batch, gk = self.batch(E), self.spec(E)
        gst = E.ChainState(self.init, self.ok.kf)
        rg = None
        for call in range(self.calls):
            fkw = {}
            if fed:
                logu, z = E.rng_stream(gst, gk, self.nsteps, seed=self.seed, chain_base=self.chain_base)
                fkw = dict(fed_logu=logu, fed_z=z)
            rg = E.sweep_batch(batch, gk, gst, self.nsteps, burnin=self.burnin, thin=self.thin, seed=self.seed,
                               chain_base=self.chain_base, check=False, stream_data=stream_data, **fkw)
            torch.cuda.synchronize()
            assert abi.last_kernel() == (form or FORMS[stream_data])
            self.assert_call(rg, gst, call)
        return rg, gst


def linreg_case(O, kind, D=3, Cm=2, p=3, n=130, nsteps=40, seed=77, data_seed=5, **kw):
    Xs, ys, base = linreg_data(D, n, p, data_seed)
    return Case(O, LINREG, Xs, ys, kind, start_points(base, D * Cm, seed + p), Cm, nsteps, seed=seed, **kw)


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_every_kernel_in_both_data_forms(E, O, name, kw):
    """D = 3 datasets x 2 chains, linreg p = 3 (k = 5), n = 130, two calls with the carried state"""
    kind, kw = _kind_kw(O, name, 5, kw)
    case = linreg_case(O, kind, calls=2, **kw)
    for stream_data in (False, True):
        case.check(E, stream_data)


@pytest.mark.parametrize("n", [1, 63, 511, 512, 513, 1025])
@pytest.mark.parametrize("name", ["normal", "ram"])
def test_lane_edges_of_the_canonical_sum(E, O, name, n):
    """fewer observations than a wavefront, than the 512 lanes, exactly 512, one and 513 more; n = 1025, p = 3 is in LDS"""
    kind, kw = _kind_kw(O, name, 5, dict(CASES)[name])
    case = linreg_case(O, kind, D=2, Cm=1, n=n, nsteps=30, **kw)
    for stream_data in (False, True):
        case.check(E, stream_data)


def test_a_dataset_beyond_the_lds_streams_without_the_flag(E, O):
    """linreg p = 7, n = 2600: 8 x 2600 doubles = 166 400 B do not fit the 160 KB of a CU"""
    case = linreg_case(O, O.K_NORMAL, D=2, Cm=1, p=7, n=2600, nsteps=25, scale=0.02)
    case.check(E, stream_data=False, form="batch-stream")


@pytest.mark.parametrize("name", ["adapt", "ram"])
def test_sixty_four_parameters(E, O, name):
    """k = 64: linreg p = 62 with an intercept, n = 100 -- every lane of the owners' wavefront holds a row"""
    kind, kw = _kind_kw(O, name, 64, dict(CASES)[name])
    case = linreg_case(O, kind, D=2, Cm=1, p=62, n=100, nsteps=25, calls=2, **kw)
    for stream_data in (False, True):
        case.check(E, stream_data)


def test_two_parameters_through_iid_normal(E, O):
    rng = np.random.default_rng(3)
    ys = 2.0 + 1.5 * rng.standard_normal((3, 200))
    case = Case(O, IID, None, ys, O.K_NORMAL, start_points([2.0, 1.5], 6, 9), 2, 60, calls=2, scale=0.1)
    for stream_data in (False, True):
        case.check(E, stream_data)


@pytest.mark.parametrize("prior_div", [8.0, 0.0])
@pytest.mark.parametrize("name", ["normal_reflective", "adapt"])
def test_logistic(E, O, name, prior_div):
    """p = 4, n = 300, D = 3: the data-only sums of every dataset, the prior and the flat prior"""
    kind, kw = _kind_kw(O, name, 5, dict(CASES)[name])
    sets = [synth_logistic(300, 4, 40 + d) for d in range(3)]
    Xs, ys = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    init = start_points([0.3, 0.8, 0.3, -0.1, -0.6], 6, 12, sigma_last=False)
    case = Case(O, LOGISTIC, Xs, ys, kind, init, 2, 40, calls=2, model_kw=dict(intercept=1, guard=0, prior_div=prior_div), **kw)
    for stream_data in (False, True):
        case.check(E, stream_data)


def test_a_fixed_parameter_burnin_and_thinning(E, O):
    case = linreg_case(O, O.K_RAM, nsteps=50, calls=2, burnin=7, thin=3, fixed=[False, True, False, False, False], lb=-2.0, ub=3.0)
    case.check(E)
    case = linreg_case(O, O.K_ADAPT, nsteps=50, calls=2, burnin=7, thin=3, fixed=[False, True, False, False, False], warmup=8)
    case.check(E, stream_data=True)


def test_chain_base_and_shards_of_whole_datasets(E, O):
    """chain_base = 1000; one call over 4 datasets == two calls over datasets {0, 1} and {2, 3}, chain_base advanced by 2 Cm"""
    import torch
    Cm = 2
    case = linreg_case(O, O.K_RAM, D=4, Cm=Cm, nsteps=30, chain_base=1000, lb=-2.0, ub=3.0)
    whole, _ = case.check(E)
    gk = case.spec(E)
    for h, ds in enumerate((slice(0, 2), slice(2, 4))):
        chains = slice(ds.start * Cm, ds.stop * Cm)
        gst = E.ChainState(case.init[chains], case.ok.kf)
        rg = E.sweep_batch(case.batch(E, ds), gk, gst, case.nsteps, seed=case.seed, chain_base=1000 + 2 * Cm * h, check=False)
        torch.cuda.synchronize()
        case.assert_call(rg, gst, 0, chains)
        assert _bits_equal(rg.samples.cpu().numpy(), whole.samples[chains].cpu().numpy())


def test_one_dataset_is_the_family_path(E, O):
    import torch
    case = linreg_case(O, O.K_NORMAL, D=1, Cm=4, nsteps=40, scale=0.05)
    rg, _ = case.check(E)
    fst = E.ChainState(case.init, case.ok.kf)
    rf = E.sweep(E.DeviceModel(LINREG, case.Xs[0], case.ys[0]), case.spec(E), fst, case.nsteps, seed=case.seed, check=False)
    torch.cuda.synchronize()
    assert _bits_equal(rf.samples.cpu().numpy(), rg.samples.cpu().numpy())


def test_three_chains_per_dataset(E, O):
    case = linreg_case(O, O.K_ADAPT, D=2, Cm=3, nsteps=40, calls=2, warmup=10)
    case.check(E)


def test_datasets_do_not_leak(E, O):
    """another y for dataset 1 leaves every output of dataset 0's chains as it was"""
    import torch
    Cm = 2
    case = linreg_case(O, O.K_RAM, D=2, Cm=Cm, nsteps=40)
    a, sa = case.check(E)
    ys = case.ys.copy()
    ys[1] = ys[1][::-1] * 3.0 + 1.0
    gst = E.ChainState(case.init, case.ok.kf)
    b = E.sweep_batch(case.batch(E, ys=ys), case.spec(E), gst, case.nsteps, seed=case.seed, check=False)
    torch.cuda.synchronize()
    own = slice(0, Cm)
    for f in ("samples", "draws", "logpost", "status_theta"):
        assert _bits_equal(getattr(a, f)[own].cpu().numpy(), getattr(b, f)[own].cpu().numpy()), f
    for f in ("accept_bits", "accept_count", "status", "status_step"):
        assert torch.equal(getattr(a, f)[own], getattr(b, f)[own]), f
    for f in ("theta0", "f0", "Sigma"):
        assert _bits_equal(getattr(sa, f)[own].cpu().numpy(), getattr(gst, f)[own].cpu().numpy()), f
    assert not _bits_equal(a.samples[Cm:].cpu().numpy(), b.samples[Cm:].cpu().numpy())   # (dataset 1 did change)


def bad_dataset_case(O):
    Xs, ys, base = linreg_data(3, 130, 3, 5)
    ys[1, 17] = np.nan
    return Case(O, LINREG, Xs, ys, O.K_NORMAL, start_points(base, 6, 80), 2, 30, model_kw=dict(guard=0), scale=0.05)


def test_a_bad_dataset_stops_its_chains_only(E, O):
    """guard = 0 and a NaN in dataset 1's y: its chains end with the oracle's status 1, status_step and status_theta, the
    other datasets' chains finish with the oracle's bits"""
    case = bad_dataset_case(O)
    st = case.refs[0]["status"]
    assert st.tolist() == [0, 0, 1, 1, 0, 0]
    for stream_data in (False, True):
        rg, _ = case.check(E, stream_data)
    with pytest.raises(RuntimeError, match=r"fun\(par\) is undefined.*\(chain 2\)"):
        E.raise_on_chain_error(rg)


def test_mcmc_batch_raises_on_a_bad_dataset_naming_the_global_chain(E, O):
    import fmcmc_amd as F
    case = bad_dataset_case(O)
    b = F.model_batch(F.gaussian_linreg(case.Xs[d], case.ys[d], guard=False) for d in range(3))
    with pytest.raises(RuntimeError, match=r"fun\(par\) is undefined.*\(chain 2\)"):
        F.MCMC_batch(case.init.reshape(3, 2, 5), b, 30, nchains=2, seed=case.seed, kernel=F.kernel_normal(scale=0.05))


def test_fed_variates(E, O):
    """fed_logu / fed_z from engine.rng_stream: the bits of the library's own stream, through both calls"""
    case = linreg_case(O, O.K_RAM, nsteps=30, calls=2, chain_base=40, lb=-2.0, ub=3.0)
    case.check(E, fed=True)
    case = linreg_case(O, O.K_NORMAL, nsteps=30, chain_base=40, scale=0.1, scheme="ordered")
    case.check(E, stream_data=True, fed=True)


@pytest.mark.parametrize("name", ["adapt", "normal_random"])
def test_the_host_entry_equals_the_device_entry(E, O, name):
    """fmcmc_mcmc_run_batch_host through ctypes from numpy arrays, two calls, with strides wider than a dataset"""
    from fmcmc_amd import _abi as abi
    kind, kw = _kind_kw(O, name, 5, dict(CASES)[name])
    case = linreg_case(O, kind, nsteps=30, calls=2, chain_base=6, **kw)
    dev, dst = case.check(E)
    D, n, p = case.D, case.ys.shape[1], case.Xs.shape[2]
    xs, ys_ = p * n + 5, n + 3
    Xh, yh = np.full((D, xs), np.nan), np.full((D, ys_), np.nan)
    Xh[:, :p * n] = case.Xs.transpose(0, 2, 1).reshape(D, p * n)
    yh[:, :n] = case.ys
    m = abi.Model(LINREG, p, n, P(Xh), P(yh), 1, 1, 0.0)
    B = host_bufs(case.init, case.ok.kf, case.nsteps)
    kk = abi_kernel(abi, case.ok)
    for call in range(case.calls):
        r = abi.Run(B.Cn, case.nsteps, 0, 1, case.seed, case.chain_base, B.step_base, abi.RNG_PHILOX, 0, None, None)
        st, out = abi_state_out(abi, B, case.ok.scheme == O.SCHEME_RANDOM)
        rc = abi.lib().fmcmc_mcmc_run_batch_host(C.byref(m), D, xs, ys_, C.byref(kk), C.byref(r), C.byref(st), C.byref(out), 0, 0)
        assert rc == abi.OK, abi.last_error()
        assert st.fresh == 0
        B.fresh, B.step_base = 0, B.step_base + case.nsteps
        ref = case.refs[call]
        assert np.array_equal(B.status, ref["status"]) and np.array_equal(B.bits, ref["accept_bits"]) and np.array_equal(B.acc, ref["accept_count"])
        assert _bits_equal(B.samples, ref["samples"]) and _bits_equal(B.dr, ref["draws"]) and _bits_equal(B.lp, ref["logpost"])
        assert _bits_equal(B.th, ref["theta0"]) and _bits_equal(B.f0, ref["f0"])
    assert _bits_equal(B.samples, dev.samples.cpu().numpy()) and _bits_equal(B.th, dst.theta0.cpu().numpy())
    if kind == O.K_ADAPT:
        assert _bits_equal(B.Sig, dst.Sigma.cpu().numpy()) and np.array_equal(B.abs_iter, dst.abs_iter.cpu().numpy())


def test_mcmc_batch_end_to_end(E, O):
    import torch
    import fmcmc_amd as F
    D, Cm, nsteps = 3, 4, 60
    case = linreg_case(O, O.K_RAM, D=D, Cm=Cm, nsteps=nsteps, calls=2)
    b = F.model_batch(F.gaussian_linreg(case.Xs[d], case.ys[d]) for d in range(D))
    kern = F.kernel_ram()
    ans = F.MCMC_batch(case.init.reshape(D, Cm, 5), b, nsteps, nchains=Cm, seed=case.seed, kernel=kern)
    assert isinstance(ans, F.McmcBatch) and len(ans) == D
    assert tuple(ans.chains.samples.shape) == (D * Cm, 5, nsteps)
    assert _bits_equal(ans.chains.samples.cpu().numpy(), case.refs[0]["samples"])
    for d in range(D):
        dc = ans[d]
        assert tuple(dc.samples.shape) == (Cm, 5, nsteps) and tuple(dc.logpost.shape) == (Cm, nsteps) and dc.chain_base == d * Cm
        assert dc.samples.data_ptr() == ans.chains.samples[d * Cm:].data_ptr()      # a slice, no copy
        own = F.DeviceChains(dc.samples.clone(), None, None, dc.iters, dc.thin, dc.names, 0, Cm)
        g, h = F.gelman_diag(dc), F.gelman_diag(own)
        assert _bits_equal(g.psrf, h.psrf) and g.mpsrf == h.mpsrf and np.isfinite(g.psrf).all()
        s = F.summary(dc)
        assert s is not None
    host = ans.to_host()
    assert len(host) == D and all(len(h) == Cm and h[0].data.shape == (nsteps, 5) for h in host)
    assert _bits_equal(host[1][2].data, case.refs[0]["samples"][Cm + 2].T)
    # the second call continues every chain from its last row with the kernel object's carried state
    ans2 = F.MCMC_batch(ans, b, nsteps, nchains=Cm, seed=case.seed, kernel=kern)
    assert _bits_equal(ans2.chains.samples.cpu().numpy(), case.refs[1]["samples"])
    with pytest.raises(ValueError, match="conv_checker"):
        F.MCMC_batch(ans, b, nsteps, nchains=Cm, seed=case.seed, kernel=kern, conv_checker=F.convergence_gelman(20))
    torch.cuda.synchronize()
