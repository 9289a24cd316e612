"""The look-ahead tree of mh_sweep_mfma's owner waves (csrc/mh_sigtree.hpp): one pass in six steps prepares the sigma-only half of
the closed form for the 63 sigmas the next six proposals can carry, a step looks up the node its decisions led to.  Every case
is the oracle's bits (run_both); a handful of chains stays on the headline kernel with knob lat=0.  The kernel uses the tree in its
one-group resident normal / uniform instantiations (mh_mfma.hpp, TREE); the reflective, two-group and streamed cases below hold the
instantiations that keep the per-step block to the same bits, and pin the tree's replay of reflect1 if it is switched on for them."""
import numpy as np
import pytest

from conftest import synth_linreg, set_knob
from test_gpu_parity import E, run_both, jitter_init  # noqa: F401  (E: the module's engine fixture)

pytestmark = pytest.mark.gpu

TREE_STEPS = 6          # steps one pass covers (ST_DEPTH)
SMALL = dict(n=600, p=3, chains=7)          # two observation slots; 7 chains: a partly filled second workgroup


@pytest.fixture(autouse=True)
def _headline_kernel(monkeypatch):
    set_knob(monkeypatch, "lat", "0")


def _small(seed=20260601, chains=SMALL["chains"], sigma0=None):
    X, y = synth_linreg(SMALL["n"], SMALL["p"], seed)
    init = jitter_init([0, 0, 0, 0, float(np.std(y))], chains, 41)
    init[:, -1] = np.abs(init[:, -1]) if sigma0 is None else sigma0
    return X, y, init


def _is_mfma(name="mfma"):
    from fmcmc_amd import _abi as abi
    assert abi.last_kernel() == name, abi.last_kernel()


def decisions(accept_bits, nsteps):
    """[chains, nsteps] 0 / 1: column i - 1 is the decision of step i (bit (i - 1) & 31 of word (i - 1) >> 5)"""
    w = np.asarray(accept_bits, dtype=np.uint32)
    i = np.arange(nsteps)
    return ((w[:, i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(np.int64)


def patterns_by_phase(dec):
    """seen[r, pat]: five consecutive decisions, the first at a step s with s % 6 == r, that read pat (first decision in the top bit)"""
    C, T = dec.shape
    look = TREE_STEPS - 1
    pat = np.zeros((C, T - look + 1), dtype=np.int64)
    for j in range(look):
        pat = 2 * pat + dec[:, j:T - look + 1 + j]
    step = np.arange(1, T - look + 2)                 # the step of the first decision of a window
    seen = np.zeros((TREE_STEPS, 1 << look), dtype=bool)
    for r in range(TREE_STEPS):
        seen[r, np.unique(pat[:, step % TREE_STEPS == r])] = True
    return seen


def test_every_node_is_consulted(E, O):
    """3000 steps at an acceptance near one half: the ORACLE's accept bitmap holds each of the 32 patterns of five consecutive
    decisions at each of the six phases step mod 6, so whatever step a pass falls on, every one of its 63 nodes is looked up (a
    node at depth d is a prefix of d decisions behind a pass).  That is a condition on the input, checked before the GPU runs."""
    X, y, init = _small()
    nsteps = 3000

    def precheck(ro):
        assert (ro.status == 0).all()
        rate = ro.accept_count.sum() / (ro.status.size * (nsteps - 1.0))
        assert 0.3 < rate < 0.7, rate
        seen = patterns_by_phase(decisions(ro.accept_bits, nsteps))
        assert seen.all(), "patterns missing at (phase, pattern): %s" % np.argwhere(~seen).tolist()

    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, 5, init, nsteps=nsteps, scale=0.08, precheck=precheck)
    _is_mfma()


@pytest.mark.parametrize("nsteps", [2, 6, 7, 8, 12, 13])
def test_calls_that_end_inside_a_tree(E, O, nsteps):
    """The rows a pass reads ahead stop at the last row of the chain's block (the last chain's rows ahead would lie behind the
    stream), and a second call starts from a pass of its own."""
    X, y, init = _small()
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, 5, init, nsteps=nsteps, calls=2, scale=0.08)
    _is_mfma()


@pytest.mark.parametrize("window", ["32", "96"])
def test_step_windows_start_from_a_pass(E, O, monkeypatch, window):
    """Step windows of 32 (no multiple of six) and 96 steps: every launch rebuilds; burn-in and thinning that divide neither."""
    set_knob(monkeypatch, "window", window)
    X, y, init = _small()
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, 5, init, nsteps=230, burnin=7, thin=3, calls=2, scale=0.08)
    _is_mfma()


def test_proposal_families(E, O):
    """Each lane of a pass replays the owner's propose(): the reflective kernel (sigma between bounds it meets often), the uniform
    kernel, no intercept, sigma itself fixed and another parameter fixed."""
    X, y, init = _small()
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL_REFLECTIVE, 5, init, nsteps=300, scale=0.3,
             lb=[-5, -5, -5, -5, 0.1], ub=[5, 5, 5, 5, 5.0], guard=False)
    _is_mfma()
    s0 = float(np.std(y))       # bounds of sigma one proposal scale around the start: most proposals of sigma reflect, some twice
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL_REFLECTIVE, 5, init, nsteps=300, scale=0.3,
             lb=[-5, -5, -5, -5, s0 - 0.3], ub=[5, 5, 5, 5, s0 + 0.3], guard=False)
    _is_mfma()
    run_both(E, O, O.FAM_LINREG, X, y, O.K_UNIF, 5, init, nsteps=300, min_=-0.1, max_=0.12)
    _is_mfma()
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, 4, init[:, 1:], nsteps=200, scale=0.08, intercept=False)
    _is_mfma()
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, 5, init, nsteps=200, scale=0.08, fixed=[False, False, False, False, True])
    _is_mfma()
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, 5, init, nsteps=200, scale=0.08, fixed=[False, True, False, False, False])
    _is_mfma()


@pytest.mark.parametrize("guard", [False, True])
def test_rare_branch_in_the_middle_of_a_table(E, O, guard):
    """sigma starts at 0.03 and moves with scale 1: proposals below zero within a few steps.  Without the guard chains fail with a
    NaN and freeze (a pass every step from there on); with it the steps of log-posterior -inf are rejected and the chain goes on."""
    X, y, init = _small(sigma0=0.03)
    _, ro = run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, 5, init, nsteps=120, guard=guard, scale=1.0)
    _is_mfma()
    if guard:
        assert (ro.status == 0).all()
    else:
        assert (ro.status == 1).any()


@pytest.mark.parametrize("n,p,steps", [(3000, 5, 90), (12000, 3, 60), (9729, 3, 60), (10240, 3, 60)],
                         ids=["two-groups", "streamed", "n9729", "n10240"])
def test_other_instantiations(E, O, monkeypatch, n, p, steps):
    """Two operand groups (p = 5), the streamed form (n = 12000) and the first and the last n of the headline's 20 slots."""
    set_knob(monkeypatch, "shard", "0")     # (few chains on long data would take the long-data form)
    X, y = synth_linreg(n, p, 11 * n + p)
    init = jitter_init([0] * (p + 1) + [float(np.std(y))], 5, 43)
    init[:, -1] = np.abs(init[:, -1])
    run_both(E, O, O.FAM_LINREG, X, y, O.K_NORMAL, p + 2, init, nsteps=steps, scale=0.02)
    _is_mfma("mfma-streamed" if n > 10240 else "mfma")
