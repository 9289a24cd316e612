"""The look-ahead pass of mh_sweep_mfma's owner waves with its shortened replay (csrc/mh_sigtree.hpp, round 7): the increments of
all levels from one multiply and add in the lanes that hold the variates, the decisions of a lane as one left-aligned mask, no replay
at all for a fixed sigma.  The pass stays with the owner wave in front of barrier 1 and keeps its period of six steps: moving it to the
late waves' barrier window and splitting the exposed owner phase were measured and dropped (profiles/r07_owner_window.md), so the
run lengths, phases and launch ends below are laid around that period.  Every case is the oracle's bits (run_both: samples, draws,
log-posteriors, accept bitmap, counts, state), on a handful of chains that stay on the headline kernel with knob lat=0 at n = 600,
p = 3.  The last case holds the BIG twins, which take the tree from nine observation slots up since the same round."""
import numpy as np
import pytest

from conftest import synth_linreg, set_knob
from test_gpu_parity import E, run_both, jitter_init  # noqa: F401  (E: the module's engine fixture)
from test_gpu_mfma_lookahead import decisions, TREE_STEPS

pytestmark = pytest.mark.gpu

PERIOD = TREE_STEPS         # steps between two look-ahead passes
N, P, K = 600, 3, 5


@pytest.fixture(autouse=True)
def _headline_kernel(monkeypatch):
    set_knob(monkeypatch, "lat", "0")


@pytest.fixture(scope="module")
def data():
    X, y = synth_linreg(N, P, 20260701)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def _init(y, chains, sigma0=None):
    init = jitter_init([0, 0, 0, 0, float(np.std(y))], chains, 47)
    init[:, -1] = np.abs(init[:, -1]) if sigma0 is None else sigma0
    return init


def patterns_by_phase(dec, period=PERIOD, look=TREE_STEPS - 1):
    """seen[r, pat]: `look` consecutive decisions, the first at a step s with s % period == r, that read pat (first decision in the
    top bit).  A table is entered by the decision of the step it was built in, and left `look` decisions later."""
    C, T = dec.shape
    pat = np.zeros((C, T - look + 1), dtype=np.int64)
    for j in range(look):
        pat = 2 * pat + dec[:, j:T - look + 1 + j]
    step = np.arange(1, T - look + 2)                 # the step of the first decision of a window
    seen = np.zeros((period, 1 << look), dtype=bool)
    for r in range(period):
        seen[r, np.unique(pat[:, step % period == r])] = True
    return seen


def _is_mfma(name="mfma"):
    from fmcmc_amd import _abi as abi
    assert abi.last_kernel() == name, abi.last_kernel()


@pytest.mark.parametrize("nsteps", [1, 2, 3] + list(range(PERIOD - 1, 2 * PERIOD + 2)))
def test_run_lengths(E, O, data, nsteps):
    """Launches that end right behind the first step and at every place of the first two tables (period - 1 .. 2 period + 1: the
    rows a pass reads ahead stop at the chain's last variate); the second call starts from a pass of its own."""
    X, y = data
    if nsteps == 1:
        # no CALL is one step long: thin < nsteps is a condition of the interface, the oracle's and the engine's alike (the shortest
        # launches are the two steps below and the two-step continuation window of test_step_windows)
        from fmcmc_amd import _abi as abi
        with pytest.raises(ValueError, match="cannot be > than -nsteps-"):
            ok = O.Kernel(O.K_NORMAL, K, scale=0.08)
            O.run(O.Model(O.FAM_LINREG, X, y), ok, nsteps=1, seed=1215, state=O.ChainState(_init(y, 7), ok.kf))
        big = E.DBL_MAX
        gk = E.KernelSpec(abi.KERNEL_NORMAL, K, np.zeros(K), np.full(K, 0.08), np.full(K, -big), np.full(K, big), np.zeros(K, np.uint8))
        with pytest.raises(ValueError, match="cannot be > than -nsteps-"):
            E.sweep(E.DeviceModel(abi.FAM_GAUSSIAN_LINREG, X, y), gk, E.ChainState(_init(y, 7), K), 1, seed=1215)
        return
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, _init(y, 7), nsteps=nsteps, calls=2, scale=0.08)
    _is_mfma()


@pytest.mark.parametrize("chains", [1, 4, 5, 7])
def test_workgroup_fill(E, O, data, chains):
    """A full workgroup, and workgroups with one, three and no missing owners."""
    X, y = data
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, _init(y, chains), nsteps=40, burnin=3, thin=2, scale=0.08)
    _is_mfma()


def test_every_decision_pattern_at_every_phase(E, O, data):
    """3000 steps at an acceptance between 0.3 and 0.7: the ORACLE's bitmap holds each of the 32 patterns of five consecutive decisions
    at each of the six phases of the pass period (and of a period of five, which a pass that leaves its root to the step before it
    would have), so whatever steps the passes fall on, every lane's replay -- every path of every depth -- is looked up.  A
    condition on the input, asserted before the device runs."""
    X, y = data
    nsteps = 3000

    def precheck(ro):
        assert (ro.status == 0).all()
        rate = ro.accept_count.sum() / (ro.status.size * (nsteps - 1.0))
        assert 0.3 < rate < 0.7, rate
        for period in (PERIOD, PERIOD - 1):
            seen = patterns_by_phase(decisions(ro.accept_bits, nsteps), period)
            assert seen.shape == (period, 32)
            assert seen.all(), "period %d: patterns missing at (phase, pattern): %s" % (period, np.argwhere(~seen).tolist())

    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, _init(y, 7), nsteps=nsteps, scale=0.08, precheck=precheck)
    _is_mfma()


@pytest.mark.parametrize("nsteps", [33, 64, 65])
def test_rows_and_bit_words(E, O, data, nsteps):
    """thin = 3 behind a burn-in of 7 with samples, draws, log-posteriors and the bitmap; the calls end one step behind, on and one
    step behind the next boundary of a 32-bit word of the bitmap."""
    X, y = data
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, _init(y, 7), nsteps=nsteps, burnin=7, thin=3, calls=2, scale=0.08)
    _is_mfma()


@pytest.mark.parametrize("fixed", [[False, True, False, False, False], [False, False, False, False, True]], ids=["beta", "sigma"])
def test_fixed_parameters(E, O, data, fixed):
    """A fixed beta, and a fixed sigma: the pass then skips its replay, every node is the sigma of the state."""
    X, y = data
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, _init(y, 7), nsteps=200, calls=2, scale=0.08, fixed=fixed)
    _is_mfma()


@pytest.mark.parametrize("guard", [False, True])
def test_rare_branch_on_step_one_and_later(E, O, data, guard):
    """Chain 2 starts at sigma = 0 and chain 5 at sigma = -0.5, the others move sigma with scale 1 around 0.03: the rare branch decides
    step 1 of every chain, comes back within a few steps, and a fresh pass follows each time.  Status, the step it reports and the
    neighbours of the failed chains (inside run_both: their samples, draws and state) are the oracle's."""
    X, y = data
    init = _init(y, 7, sigma0=0.03)
    init[2, -1] = 0.0
    init[5, -1] = -0.5
    rg, ro = run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, init, nsteps=120, guard=guard, scale=1.0)
    _is_mfma()
    assert np.array_equal(rg.status_step.cpu().numpy(), ro.status_step)
    if guard:      # log-posteriors that are not finite count as -inf: such proposals are rejected and no chain fails
        assert (ro.status == 0).all()
        return
    assert ro.status[5] != 0 and ro.status_step[5] == 2, "sigma < 0 at the start fails the chain at once"
    assert (ro.status_step[ro.status != 0] > 2).any() and (ro.status == 0).any(), "a later failure, and a chain that goes on"
    # sigma moves with scale 2 around ~4: the chains fail one after the other, dozens of steps apart, next to chains that go on
    rg, ro = run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, _init(y, 7), nsteps=400, guard=False, scale=[0.08, 0.08, 0.08, 0.08, 2.0])
    assert np.array_equal(rg.status_step.cpu().numpy(), ro.status_step)
    assert (ro.status == 1).any() and np.unique(ro.status_step).size >= 4


@pytest.mark.parametrize("window", ["32", "96"])
def test_step_windows(E, O, data, monkeypatch, window):
    """The same call cut into step windows: every launch starts from a pass of its own."""
    set_knob(monkeypatch, "window", window)
    X, y = data
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, _init(y, 7), nsteps=230, burnin=7, thin=3, calls=2, scale=0.08)
    _is_mfma()
    # one step more than window 0 holds: the second launch re-evaluates the state it starts from and decides ONE step
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, K, _init(y, 7), nsteps=int(window) + 2, calls=2, scale=0.08)
    _is_mfma()


def test_second_sweep_into_a_history(E, data):
    """A second sweep on the carried state that writes behind the first into one preallocated history gives the bits of two
    separately allocated calls (which run_both holds to the oracle above)."""
    import torch
    from fmcmc_amd import _abi as abi
    X, y = data
    init = _init(y, 7)
    gm = E.DeviceModel(abi.FAM_GAUSSIAN_LINREG, X, y)
    big = E.DBL_MAX
    gk = E.KernelSpec(abi.KERNEL_NORMAL, K, np.zeros(K), np.full(K, 0.08), np.full(K, -big), np.full(K, big), np.zeros(K, np.uint8))
    sa, sb = E.ChainState(init, K), E.ChainState(init, K)
    a1 = E.sweep(gm, gk, sa, 64, burnin=7, thin=3, seed=9)
    a2 = E.sweep(gm, gk, sa, 41, thin=3, seed=9)
    _is_mfma()
    n1, n2 = a1.samples.shape[2], a2.samples.shape[2]
    cap = n1 + n2 + 3
    f64 = dict(dtype=torch.float64, device="cuda")
    hs, hl, hd = torch.full((7, K, cap), -7.0, **f64), torch.full((7, cap), -7.0, **f64), torch.full((7, K, cap), -7.0, **f64)
    E.sweep(gm, gk, sb, 64, burnin=7, thin=3, seed=9, into=(hs, hl, hd), row0=0)
    E.sweep(gm, gk, sb, 41, thin=3, seed=9, into=(hs, hl, hd), row0=n1)
    torch.cuda.synchronize()

    def bits(t):
        return np.ascontiguousarray(t.cpu().numpy()).view(np.uint64)

    for h, a, b in ((hs, a1.samples, a2.samples), (hd, a1.draws, a2.draws), (hl, a1.logpost, a2.logpost)):
        assert np.array_equal(bits(h[..., :n1]), bits(a)) and np.array_equal(bits(h[..., n1:n1 + n2]), bits(b))
        assert (h[..., n1 + n2:] == -7.0).all()
    assert np.array_equal(bits(sb.theta0), bits(sa.theta0)) and np.array_equal(bits(sb.f0), bits(sa.f0))


@pytest.mark.parametrize("kind,n,p,steps", [("reflective", N, P, 300), ("normal", 3000, 5, 200), ("normal", 11000, 3, 200)],
                         ids=["reflective", "two-groups", "streamed"])
def test_instantiations_outside_the_gate(E, O, monkeypatch, kind, n, p, steps):
    """KIND 2, two operand groups and the streamed form keep the per-step sigma block and run no pass: still the oracle's bits."""
    set_knob(monkeypatch, "shard", "0")     # (few chains on long data would take the long-data form)
    X, y = synth_linreg(n, p, 13 * n + p)
    init = jitter_init([0] * (p + 1) + [float(np.std(y))], 5, 43)
    init[:, -1] = np.abs(init[:, -1])
    if kind == "reflective":
        run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL_REFLECTIVE, p + 2, init, nsteps=steps, scale=0.3,
                 lb=[-5] * (p + 1) + [0.1], ub=[5] * (p + 1) + [5.0], guard=False)
    else:
        run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, p + 2, init, nsteps=steps, scale=0.02)
    _is_mfma("mfma-streamed" if n > 10240 else "mfma")


def test_big_offsets_form_with_the_tree(E, O):
    """The BIG instantiations (64-bit chain bases: 4 GiB of samples or more) run the pass from nine observation slots up.  A history of
    15.4 million rows for 7 chains x 5 parameters is 4.3 GB of samples, so a call of 300 steps that writes into it takes the BIG form
    at n = 4200 (nine slots): its rows, log-posteriors, bitmap and state are the oracle's.  (Twenty slots at 1.2e5 steps against the
    general kernel: test_gpu_parity.py, a call longer than 4 GiB of samples.)"""
    import torch
    from fmcmc_amd import _abi as abi
    n, chains, nsteps = 4200, 7, 300
    X, y = synth_linreg(n, P, 20260702)
    init = _init(y, chains)
    ok = O.Kernel(O.K_NORMAL, K, scale=0.03)
    ost = O.ChainState(init, ok.kf)
    ro = O.run(O.Model(O.FAM_LINREG, X, y), ok, nsteps=nsteps, seed=1215, state=ost)
    assert (ro.status == 0).all() and 0.2 < ro.accept_count.sum() / (chains * (nsteps - 1.0)) < 0.8
    cap = (1 << 32) // (chains * K * 8) + 1000
    assert chains * K * cap * 8 >= 1 << 32 and K * cap * 8 < 1 << 32          # the dispatcher's condition for BIG, and its limit
    hs = torch.empty((chains, K, cap), dtype=torch.float64, device="cuda")
    hl = torch.empty((chains, cap), dtype=torch.float64, device="cuda")
    row0 = cap - nsteps - 7                                                   # rows near the end of every chain's block
    gk = E.KernelSpec(abi.KERNEL_NORMAL, K, ok.mu, ok.scale, ok.lb, ok.ub, ok.fixed)
    gst = E.ChainState(init, ok.kf)
    rg = E.sweep(E.DeviceModel(abi.FAM_GAUSSIAN_LINREG, X, y), gk, gst, nsteps, seed=1215, check=False, into=(hs, hl, None), row0=row0)
    torch.cuda.synchronize()
    _is_mfma()

    def bits(a):
        return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)

    assert np.array_equal(rg.status.cpu().numpy(), ro.status)
    assert np.array_equal(rg.accept_bits.cpu().numpy().view(np.uint32), ro.accept_bits)
    assert np.array_equal(bits(hs[:, :, row0:row0 + nsteps].cpu().numpy()), bits(ro.samples_cks))
    assert np.array_equal(bits(hl[:, row0:row0 + nsteps].cpu().numpy()), bits(ro.logpost))
    assert np.array_equal(bits(gst.theta0.cpu().numpy()), bits(ost.theta0)) and np.array_equal(bits(gst.f0.cpu().numpy()), bits(ost.f0))
