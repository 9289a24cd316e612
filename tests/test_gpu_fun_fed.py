"""The callback path (batched_fun -> fmcmc_mcmc_run_fun_dev) with host-fed variates (fmcmc_run.rng_mode = FED), on another
stream than torch's current one, and on device="cuda".

 * fed R's own Mersenne-Twister stream, with `fun` = the oracle's R-math log-posterior, it retraces what fmcmc PRINTS for the
   README's linear regression (G1, and the kernel_normal / kernel_ram continuation of G4; tests/golden/readme_goldens.json);
 * fed the canonical stream of a PHILOX call (fmcmc_rng_stream_dev) and that call's update plan, scheme = "random" included, it
   repeats the PHILOX call bit for bit."""
import json
import os

import numpy as np
import pytest

from conftest import synth_linreg
from test_gpu_fun import host_fun
from test_gpu_parity import _bits_equal

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "readme_goldens.json")))


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fmcmc_amd import engine
    return engine


def sig(x, d):
    return float("%.*g" % (d, x))


def fed_stream(g, nsteps, kz, ram_df=None):
    """R's draw order for one chain (R/mcmc.R:726 then the kernel's draws per step)."""
    logu = np.log(g.runif(nsteps))
    z = np.zeros((nsteps, kz))
    for i in range(1, nsteps):   # rows 1.. hold the variates of loop steps 2..
        z[i] = g.rt(kz, ram_df) if ram_df else g.rnorm(kz)
    return logu, z


def r_fun(om):
    """fn(theta) = the oracle's R-math log-posterior (math_mode = R: R's own dnorm sums) of every row"""
    import torch
    from oracle import oracle as O

    def fn(th):
        return torch.tensor([om.logpost(r, math_mode=O.MATH_R) for r in th.cpu().numpy()], dtype=torch.float64,
                            device=th.device)
    return fn


def test_readme_g1_on_rs_stream_through_the_callback(E, O, readme_data):
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    X, y = readme_data
    om = O.Model(O.FAM_LINREG, X, y)
    gf = E.DeviceFun(F.batched_fun(r_fun(om), 3))
    big = E.DBL_MAX
    g = O.RRng(1215)

    def run(kind, scale, init, ram=False):
        logu, z = fed_stream(g, 5000, 3, ram_df=3.0 if ram else None)
        gk = E.KernelSpec(kind, 3, np.zeros(3), np.full(3, scale), np.full(3, -big), np.full(3, big),
                          np.zeros(3, np.uint8), warmup=0)
        st = E.ChainState(np.asarray(init, dtype=np.float64)[None, :], 3)
        r = E.sweep(gf, gk, st, 5000, fed_logu=torch.as_tensor(logu[None, :]).cuda().contiguous(),
                    fed_z=torch.as_tensor(z[None, :, :]).cuda().contiguous())
        torch.cuda.synchronize()
        assert abi.last_kernel() == "fun"
        return r, st

    # README.md:156-201 (G1)
    r1, _ = run(abi.KERNEL_NORMAL, 1.0, [0, 0, O.r_sd(y)])
    s = r1.samples.cpu().numpy()[0].T
    assert [sig(v, 4) for v in s.mean(0)] == G["G1"]["mean"]
    assert [sig(v, 4) for v in s.std(0, ddof=1)] == [sig(v, 4) for v in G["G1"]["sd"]]
    q = np.quantile(s[:, 0], [.025, .25, .5, .75, .975])
    assert [sig(v, 4) for v in q] == G["G1"]["q_par1"]
    assert list(O.accept_steps(r1.accept_bits.cpu().numpy().view(np.uint32)[0])) == [
        3, 5, 8, 10, 14, 32, 67, 544, 786, 834, 1598, 2764, 3693, 3826, 4039, 4514, 4613, 4776, 4898, 4916, 4950]
    # README.md:209-246 (G4): kernel_normal(scale=.05) from the last row, then kernel_ram() on R's rt(k, k) variates
    r2, _ = run(abi.KERNEL_NORMAL, 0.05, s[-1])
    s2 = r2.samples.cpu().numpy()[0].T
    assert int(r2.accept_count[0]) == 3641
    r3, st3 = run(abi.KERNEL_RAM, 1.0, s2[-1], ram=True)
    assert int(r3.accept_count[0]) == 1761
    assert sig(1761 / 4999, 7) == G["G4"]["ram_accept_rate"]
    assert np.allclose(st3.Sigma.cpu().numpy()[0], [[0.18001104, 0, 0], [0.01481571, 0.17576006, 0],
                                                    [0.00806067, -0.00281060, 0.11951173]], atol=5e-9)
    # the same G1 call through MCMC(fed = ...): the same chain
    fed = lambda C_, nsteps, kz, kernel: tuple(a[None] for a in fed_stream(O.RRng(1215), nsteps, kz))
    ans = F.MCMC([0.0, 0.0, O.r_sd(y)], F.batched_fun(r_fun(om), 3), 5000, seed=0, kernel=F.kernel_normal(scale=1.0),
                 fed=fed)
    assert _bits_equal(ans.data, s)


@pytest.mark.parametrize("name", ["normal_random", "unif_reflective", "adapt", "ram_bounded"])
def test_fed_canonical_stream_repeats_the_philox_call(E, O, name):
    import torch
    from fmcmc_amd.models import batched_fun
    X, y = synth_linreg(300, 3, 21)
    om = O.Model(O.FAM_LINREG, X, y)
    kind, kw = {"normal_random": (O.K_NORMAL, dict(scale=0.1, scheme="random")),
                "unif_reflective": (O.K_UNIF_REFLECTIVE, dict(min_=-0.05, max_=0.05, lb=-4.0, ub=6.0)),
                "adapt": (O.K_ADAPT, dict(warmup=10)),
                "ram_bounded": (O.K_RAM, dict(lb=-4.0, ub=6.0))}[name]
    ok = O.Kernel(kind, 5, **kw)
    gk = E.KernelSpec(kind, 5, ok.mu, ok.scale, ok.lb, ok.ub, ok.fixed, scheme=ok.scheme, warmup=ok.warmup)
    init = np.array([3.0, 2.0, -1.0, 0.5, 4.0])[None, :] + 0.05 * np.random.default_rng(2).standard_normal((4, 5))
    gf = E.DeviceFun(batched_fun(host_fun(om), 5))
    nsteps, seed = 80, 99
    st1 = E.ChainState(init, ok.kf)
    st2 = E.ChainState(init, ok.kf)
    logu, z = E.rng_stream(st2, gk, nsteps, seed=seed)          # (before the calls: step_base 0)
    r1 = E.sweep(gf, gk, st1, nsteps, seed=seed, check=False)
    if st1.scheme_cols is not None:
        st2.scheme_cols = st1.scheme_cols.clone()                # FED: the plan is read, not drawn
    r2 = E.sweep(gf, gk, st2, nsteps, seed=seed + 1, fed_logu=logu, fed_z=z, check=False)
    torch.cuda.synchronize()
    for a, b in ((r1.samples, r2.samples), (r1.draws, r2.draws), (r1.logpost, r2.logpost), (st1.theta0, st2.theta0),
                 (st1.Sigma, st2.Sigma)):
        assert _bits_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(r1.accept_bits.cpu().numpy(), r2.accept_bits.cpu().numpy())
    # and the PHILOX call is the oracle's
    ro = O.run(om, ok, init, nsteps=nsteps, seed=seed)
    assert _bits_equal(r1.samples.cpu().numpy(), ro.samples_cks)


def test_fn_runs_on_the_engine_stream(E, O):
    """sweep(stream = s) with s not torch's current stream: fn sees s as its current stream, the call equals the one on the
    current stream bit for bit"""
    import torch
    from fmcmc_amd.models import batched_fun
    X, y = synth_linreg(400, 1, 5)
    om = O.Model(O.FAM_LINREG, X, y)
    seen = []
    inner = host_fun(om)

    def fn(th):
        seen.append(torch.cuda.current_stream().cuda_stream)
        return inner(th)
    ok = O.Kernel(O.K_RAM, 3)
    init = np.array([[3.0, 2.0, 4.0]] * 3) + 0.1 * np.arange(9).reshape(3, 3)
    out, n0 = [], []
    side = torch.cuda.Stream()
    for stream in (None, side):
        n0.append(len(seen))
        st = E.ChainState(init, 3)
        gk = E.KernelSpec(O.K_RAM, 3, ok.mu, ok.scale, ok.lb, ok.ub, ok.fixed)
        r = E.sweep(E.DeviceFun(batched_fun(fn, 3)), gk, st, 60, seed=4, stream=stream)
        (side if stream is not None else torch.cuda.current_stream()).synchronize()
        out.append((r.samples.cpu().numpy(), st.Sigma.cpu().numpy()))
    assert n0[1] == 60 and set(seen[n0[1]:]) == {side.cuda_stream}
    assert _bits_equal(out[0][0], out[1][0]) and _bits_equal(out[0][1], out[1][1])


def test_device_cuda_without_an_index(E):
    import fmcmc_amd as F
    fun = F.batched_fun(lambda th: -(th * th).sum(1), 3)
    ans = F.MCMC(np.zeros((2, 3)), fun, 50, nchains=2, seed=3, device="cuda")
    ref = F.MCMC(np.zeros((2, 3)), fun, 50, nchains=2, seed=3)
    assert _bits_equal(ans.as_array(), ref.as_array())
