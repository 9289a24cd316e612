"""Every device entry point is held to its caller's stream (include/fmcmc_amd.h: "the call only enqueues kernels on hip_stream";
engine.py: `stream=`, or torch's current stream).  On an idle default stream a launch, memset or copy that strays to another stream
still gives the right bits, and so does a buffer prepared on a stream the kernel does not wait for: the rest of the suite cannot see
either.  Here every call runs next to a timed gate.

The gate: a stream kept busy for GATE_MS by torch.cuda._sleep (cycles per millisecond calibrated once per module), and an event
recorded behind it.  The gate "was closed when the call returned" if that event's query() is still false.  It ends by itself: a
test that dies leaves nothing spinning.  torch's side streams do not wait for the legacy null stream, so stray work there runs
while the gate is closed -- on side streams that do not share a hardware queue with it: side_streams() finds two such streams once
per module (two streams on one queue run in turn, and a gate on one would hold the other's stray work back as well).

Every case first runs its call ungated on the default stream -- that warms the code object and is the reference -- then again on
fresh, identical inputs next to a gate; every output tensor and every carried state tensor must hold the reference's bits.

 A. the library's work stays on its stream.  The call goes to a side stream (torch's current one, or passed as `stream=` /
    hip_stream).  Before it, every device input holds a decoy (same shape, finite values: decoy()); on the side stream, in this
    order: the gate, copy_ of the true inputs, fill_(nan) of every buffer the test owns, the call.  A piece of the call that ran
    elsewhere read decoys or had its output overwritten by the NaN fill.  For the entry points documented as enqueue-only the gate
    must still be closed at return ("no synchronise").
 B. the Python layer's own preparation is ordered before the engine's stream: the gate is on torch's current stream, the call
    gets an idle `stream=side` (on which the same call ran once before, so that it starts at once).  No NaN or zero fill of an
    output may land after the sweep wrote it, no copy of an input after the kernel read it.
 C. check=True sees the stream: a failing chain is reported although its status is written behind a gate.
 D. two different calls on two side streams overlap and equal their serial results.

The rows, lags and ranks of the diagnostics are HOST arrays of the C ABI (read during the call): there is no device decoy for them.

Entry points that are documented to synchronise (they skip the closed-gate assertion only):
  fmcmc_mcmc_run_fun_dev   "`fun` is called once for row 1 (f0), then once per loop step"; fmcmc_logpost_fn: "Work is enqueued on
                           hip_stream, or the function synchronises before returning" -- a host callback per step.
  fmcmc_mcmc_run_user_dev  fmcmc_proposal_fn / fmcmc_logratio_fn: "Called on the calling host thread, once per loop step each.  Work
                           is enqueued on hip_stream, or the function synchronises before returning."
  fmcmc_mcmc_run_dev with NULL h_* mirrors   "with NULLs it reads the few bytes back from the device and synchronises the stream
                           first."
  the Python wrappers of the diagnostics (summary(), gelman_diag(), ...): they return host numbers, and refuse non-finite rows from
                           a count they read back.
"""
import ctypes as C
import gc
import time
import warnings

import numpy as np
import pytest

import diag_dev
import gelman_dev
from conftest import set_knob
from test_gpu_parity import E  # noqa: F401  (the module's engine fixture)
from test_gpu_route import SHAPES

pytestmark = pytest.mark.gpu

LINREG, LOGISTIC, IID = 1, 2, 3
NORMAL, ADAPT, RAM, UNIF = 1, 3, 4, 5
DBL_MAX = float(np.finfo(np.float64).max)
SEED = 7
NAN = float("nan")

# ---- the gate ------------------------------------------------------------------------------------------------------------------------
# The gate has to outlast the host's enqueueing of a call.  ENQUEUE_MS is the largest warm host-side duration (median of five,
# time.perf_counter around the call, default stream, the commit before this file) over the enqueue-only calls of this module, as
# measured on an MI355X; the gate gets ten times that, and never more than a second.  Measured: 0.165 ms, the `logistic-sharded`
# sweep (the sweeps take 0.08 to 0.17 ms, sweep_batch 0.09 to 0.14 ms, fmcmc_summary_dev 0.09 ms, fmcmc_heidel_dev 0.06 ms, every
# other diagnostic, fmcmc_logpost_dev and fmcmc_rng_stream_dev under 0.03 ms); the gate is 1.65 ms.  The 122 cases of the file
# take 11 to 16 s on an MI355X.
ENQUEUE_MS = 0.165
GATE_MS = min(10.0 * ENQUEUE_MS, 1000.0)
GATE_TOO_SHORT = "gate too short: open when the call returned (%.2f ms of host time; the gate took %.2f ms, %.1f ms were asked for)"

_cycles_per_ms = []


def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond, from two events around a warm sleep; measured once per module"""
    import torch
    if not _cycles_per_ms:
        torch.cuda._sleep(1 << 20)
        torch.cuda.synchronize()
        n = 1 << 24
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        _cycles_per_ms.append(n / a.elapsed_time(b))
    return _cycles_per_ms[0]


class Gate:
    """`stream` is busy for `ms` from now on; closed() until the event behind the sleep has happened"""

    def __init__(self, stream, ms=None):
        import torch
        self.ms = GATE_MS if ms is None else ms
        cycles = int(self.ms * cycles_per_ms())
        self.start, self.opened = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.start.record()
            torch.cuda._sleep(cycles)
            self.opened.record()

    def closed(self):
        return not self.opened.query()

    def too_short(self, host_ms):
        """the failure message; call it after the stream was synchronised"""
        return GATE_TOO_SHORT % (host_ms, self.start.elapsed_time(self.opened), self.ms)


def quiet_host():
    """before a gate is set up: a collection of the interpreter's own now, so that none falls into the gate's milliseconds"""
    import torch
    gc.collect()
    torch.cuda.synchronize()


def runs_beside(gated, other):
    """does work on the stream `other` run while the stream `gated` is busy?  The runtime folds its streams onto a few hardware
    queues, and two streams that share a queue run in turn: a gate on one of them holds the other back as well, and stray work
    would wait for the gate like everything else."""
    import torch
    quiet_host()
    gate, done = Gate(gated), torch.cuda.Event()
    done.record(other)
    beside = False
    while gate.closed() and not beside:
        beside = done.query()
    torch.cuda.synchronize()
    return beside


_side_streams = []


def side_streams():
    """Two side streams for the module: each runs beside the null stream, either way round, and beside the other (runs_beside).
    Found once among a few streams of torch's pool."""
    import torch
    if not _side_streams:
        null, pool = torch.cuda.default_stream(), [torch.cuda.Stream() for _ in range(8)]
        a = next((s for s in pool if runs_beside(s, null) and runs_beside(null, s)), None)
        b = next((s for s in pool if s is not a and a is not None and runs_beside(s, null) and runs_beside(null, s)
                  and runs_beside(a, s) and runs_beside(s, a)), None)
        if a is None or b is None:
            warnings.warn("no two side streams that run beside the null stream and each other: a gate proves less on this device")
            a, b = (pool[0] if a is None else a), next(s for s in pool if s is not a)
        _side_streams[:] = [a, b]
    return _side_streams


def decoy(t):
    """Same shape, finite, other values, and nothing a kernel could trip over: floats are scaled by factors in (0.5, 0.9) from a
    seed of their own (signs stay, bounds stay ordered, zeros become small positive numbers), integers and masks are rotated by
    one place (indices stay valid, counts stay)."""
    import torch
    if t.is_floating_point():
        g = torch.Generator().manual_seed(20260 + t.numel())
        f = (0.5 + 0.4 * torch.rand(tuple(t.shape), generator=g, dtype=torch.float64)).to(t.device)
        return torch.where(t == 0, 0.37 * f, t * f)
    return torch.roll(t, 1, dims=-1)


def sptr(stream):
    import torch
    return C.c_void_p((torch.cuda.current_stream() if stream is None else stream).cuda_stream)


def snapshot(named):
    import torch
    out = {}
    for name, v in named.items():
        if v is not None:
            out[name] = v.detach().contiguous().cpu().numpy().copy() if torch.is_tensor(v) else np.ascontiguousarray(v)
    return out


def assert_same_bits(ref, got, what):
    assert sorted(ref) == sorted(got), (what, sorted(ref), sorted(got))
    bad = [n for n in ref if ref[n].shape != got[n].shape or ref[n].dtype != got[n].dtype or ref[n].tobytes() != got[n].tobytes()]
    first = ""
    if bad and ref[bad[0]].shape == got[bad[0]].shape and ref[bad[0]].dtype.kind in "fiu":
        r, g = ref[bad[0]].ravel(), got[bad[0]].ravel()
        at = np.nonzero(r.view(np.uint8).reshape(r.size, -1) != g.view(np.uint8).reshape(g.size, -1))[0]
        first = "; %s differs in %d of %d elements, the first at %d: %r, the reference has %r" % (
            bad[0], np.unique(at).size, r.size, at[0], g[at[0]], r[at[0]])
    assert not bad, "%s: other bits than the ungated run on the default stream in %s%s" % (what, bad, first)


def reference(case):
    """the ungated run on the default stream"""
    import torch
    case.call(None)
    torch.cuda.synchronize()
    return snapshot(case.results())


def gated_a(case, mode, enqueue_only):
    """Direction A on a fresh case.  mode "current": the side stream is torch's current stream; "passed": it is handed to the
    call.  Returns with nothing pending; the gate is judged after the streams were synchronised."""
    import torch
    side = side_streams()[0]
    inputs = case.inputs()
    true = [t.clone() for t in inputs]
    for t in inputs:
        t.copy_(decoy(t))
    quiet_host()
    gate = Gate(side)
    closed, host_ms = None, 0.0
    try:
        with torch.cuda.stream(side):
            for t, v in zip(inputs, true):
                t.copy_(v)
            for b in case.owned():
                b.fill_(NAN)
            if mode == "current":
                t0 = time.perf_counter()
                case.call(None)
                host_ms = 1e3 * (time.perf_counter() - t0)
                closed = gate.closed()
        if mode == "passed":
            t0 = time.perf_counter()
            case.call(side)
            host_ms = 1e3 * (time.perf_counter() - t0)
            closed = gate.closed()
    finally:
        side.synchronize()
        torch.cuda.synchronize()
    if enqueue_only:
        assert closed, gate.too_short(host_ms)


def scribble(nbytes):
    """NaNs into the blocks the caching allocator just took back, so that a temporary read too early does not find the reference
    run's values"""
    import torch
    junk = [torch.full((max(nbytes // 8, 1),), NAN, dtype=torch.float64, device="cuda") for _ in range(32)]
    del junk


def gated_b(case, side):
    """Direction B on a fresh case: the gate on torch's current stream, the call on the idle stream `side`"""
    import torch
    quiet_host()
    Gate(torch.cuda.current_stream())
    try:
        case.call(side)
    finally:
        side.synchronize()
        torch.cuda.synchronize()


# ---- the calls ---------------------------------------------------------------------------------------------------------------------
STATE = ("theta0", "f0", "abs_iter", "Sigma", "mean_prev", "have_mean", "nerrors", "mirror_mu", "mirror_scale", "obs_arate", "scheme_cols")
OUT = ("samples", "logpost", "draws", "accept_count", "accept_bits", "status", "status_step", "status_theta")


def spec_tensors(gk):
    return [t for t in (gk.mu, gk.scale, gk.lb, gk.ub, gk.fixed, gk.scheme_seq, gk.constr) if t is not None]


def state_tensors(st):
    return [getattr(st, n) for n in STATE if getattr(st, n) is not None]


def sweep_results(res, st, ran=None):
    """every output of a call and the state it carried on (call it after the streams were synchronised).  logpost and draws are
    torch.empty: their rows count for the chains that ran (ran: a bool tensor, None = all) and did not fail, f0 for the latter;
    mean_prev is defined where have_mean says so (a fresh chain's is whatever the kernel held: the suite compares it nowhere else)."""
    good = res.status == 0
    wrote = good if ran is None else good & ran
    named = {n: getattr(res, n) for n in OUT}
    named["logpost"], named["draws"] = res.logpost[wrote], res.draws[wrote]
    named.update({"state." + n: getattr(st, n) for n in STATE})
    named["state.f0"], named["state.mean_prev"] = st.f0[good], st.mean_prev[st.have_mean != 0]
    return named


def route_data(fam, p, n, chains):
    """the inputs of a row of test_gpu_route.SHAPES"""
    rng = np.random.default_rng(1000 * p + chains)
    X = rng.standard_normal((n, p))
    beta = rng.uniform(-1.0, 1.0, p + 1)
    eta = beta[0] + X @ beta[1:]
    y = eta + 2.0 * rng.standard_normal(n) if fam == LINREG else (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    k = p + 1 + (1 if fam == LINREG else 0)
    init = np.concatenate([beta, [2.0]] if fam == LINREG else [beta])[None, :] + 0.01 * rng.standard_normal((chains, k))
    return X, y, k, init


class Sweep:
    """engine.sweep on a family (fmcmc_mcmc_run_dev).  fed: the variates come from engine.rng_stream, enqueued in front of the
    sweep on the same stream.  null_mirrors: the fmcmc_kernel goes through ctypes without its h_* host mirrors, so the entry reads
    fixed / lb / ub back from the device; one parameter is fixed, another in the decoy."""

    def __init__(self, E, fam, p, n, kind, chains, opts, nsteps=32, fed=False, null_mirrors=False, guard=True, init=None, scale=0.01):
        X, y, k, init0 = route_data(fam, p, n, chains)
        self.E, self.nsteps, self.fed = E, nsteps, fed
        self.gm = E.DeviceModel(fam, X, y, guard=guard)
        fixed = np.zeros(k, np.uint8)
        if null_mirrors:
            fixed[1] = 1
        self.gk = E.KernelSpec(kind, k, np.zeros(k), np.full(k, scale), np.full(k, -DBL_MAX), np.full(k, DBL_MAX), fixed, **opts)
        if null_mirrors:
            with_mirrors = self.gk.c

            def without():
                ck = with_mirrors()
                ck.h_fixed = ck.h_lb = ck.h_ub = ck.h_scale = ck.h_scheme_seq = None
                return ck
            self.gk.c = without
        self.st = E.ChainState(init0 if init is None else init, self.gk.kf)
        self.res = None

    def inputs(self):
        return [self.gm.Xc, self.gm.y] + spec_tensors(self.gk) + state_tensors(self.st)

    def owned(self):
        return []

    def call(self, stream, check=False):
        kw = {}
        if self.fed:
            self.logu, self.z = self.E.rng_stream(self.st, self.gk, self.nsteps, seed=SEED, stream=stream)
            kw = dict(fed_logu=self.logu, fed_z=self.z)
        self.res = self.E.sweep(self.gm, self.gk, self.st, self.nsteps, seed=SEED, check=check, stream=stream, **kw)

    def results(self):
        return sweep_results(self.res, self.st)


class Batch:
    """engine.sweep_batch (fmcmc_mcmc_run_batch_sel_dev): D = 3 datasets x 2 chains"""
    D, CM = 3, 2

    def __init__(self, E, fam, p, n, kind, nsteps=40, stream_data=False, mask=None, opts=None):
        import torch
        D, Cm = self.D, self.CM
        sets = [route_data(fam, p, n, 10 * Cm + d) for d in range(D)]
        k = sets[0][2]
        init = np.concatenate([s[3][:Cm] for s in sets])
        self.E, self.nsteps, self.stream_data = E, nsteps, stream_data
        self.gb = E.DeviceModelBatch(fam, np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]))
        self.gk = E.KernelSpec(kind, k, np.zeros(k), np.full(k, 0.05), np.full(k, -DBL_MAX), np.full(k, DBL_MAX), np.zeros(k, np.uint8),
                               **(opts or {}))
        self.st = E.ChainState(init, self.gk.kf)
        self.active = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.int32)).cuda()
        self.ran = None if mask is None else torch.as_tensor(np.repeat(mask, Cm).astype(bool)).cuda()
        self.res = None

    def inputs(self):
        return [self.gb.Xc, self.gb.y] + spec_tensors(self.gk) + state_tensors(self.st) + ([] if self.active is None else [self.active])

    def owned(self):
        return []

    def call(self, stream):
        self.res = self.E.sweep_batch(self.gb, self.gk, self.st, self.nsteps, seed=SEED, check=False, stream=stream,
                                      stream_data=self.stream_data, active=self.active)

    def results(self):
        return sweep_results(self.res, self.st, self.ran)


class Callback:
    """k = 3, 3 chains, 30 steps.  what = "fun": engine.sweep on a DeviceFun (fmcmc_mcmc_run_fun_dev); "user-fun" / "user-model":
    engine.sweep_user (fmcmc_mcmc_run_user_dev) with the model evaluated by the callback / by the engine.  The callbacks read
    device tensors of their own (the centre of the callback's log-density, the proposal's mu and scale): gated inputs too."""

    def __init__(self, E, what):
        import torch
        from fmcmc_amd import kernel_new
        from fmcmc_amd.models import batched_fun
        k, chains = 3, 3
        self.E, self.what, self.nsteps = E, what, 30
        X, y, _, init = route_data(LINREG, 1, 100, chains)
        self.extra = []
        if what == "user-model":
            self.model = E.DeviceModel(LINREG, X, y)
            self.extra += [self.model.Xc, self.model.y]
        else:
            centre = torch.as_tensor(np.array([0.5, -0.25, 2.0])).cuda()
            self.extra.append(centre)
            self.model = E.DeviceFun(batched_fun(lambda th: -0.5 * ((th - centre) * (th - centre)).sum(1), k))
        if what == "fun":
            self.gk = E.KernelSpec(NORMAL, k, np.zeros(k), np.full(k, 0.1), np.full(k, -DBL_MAX), np.full(k, DBL_MAX), np.zeros(k, np.uint8))
            self.extra += spec_tensors(self.gk)
        else:
            mu, scale = torch.as_tensor(np.full(k, 0.01)).cuda(), torch.as_tensor(np.full(k, 0.1)).cuda()
            self.extra += [mu, scale]
            self.gk = kernel_new(lambda env: env.theta0 + (mu + scale * env.rnorm(env.k)))
        self.st = E.ChainState(init, k)
        self.res = None

    def inputs(self):
        return self.extra + state_tensors(self.st)

    def owned(self):
        return []

    def call(self, stream):
        run = self.E.sweep if self.what == "fun" else self.E.sweep_user
        self.res = run(self.model, self.gk, self.st, self.nsteps, seed=SEED, check=False, stream=stream)

    def results(self):
        return sweep_results(self.res, self.st)


class Logpost:
    """DeviceModel.logpost (fmcmc_logpost_dev) at n = 513, 7 chains; sliced: theta is a column slice of a wider tensor; shift:
    other points (added to the slopes and the location, not to sigma)"""

    def __init__(self, E, fam, sliced=False, shift=0.0):
        import torch
        p = {LINREG: 3, LOGISTIC: 4, IID: 0}[fam]
        rng = np.random.default_rng(513 + fam)
        if fam == IID:
            X, y, k, base = None, 2.0 + 1.5 * rng.standard_normal(513), 2, np.array([2.0, 1.5])
        else:
            X, y, k, init = route_data(fam, p, 513, 7)
            base = init[0]
        self.gm = E.DeviceModel(fam, X, y)
        wide = np.tile(np.r_[9.0, base, 9.0, 9.0], (7, 1)) + 0.05 * rng.standard_normal((7, k + 3))
        wide[:, 1] += shift
        self.wide = torch.as_tensor(wide).cuda()
        self.theta = self.wide[:, 1:k + 1] if sliced else self.wide[:, 1:k + 1].contiguous()
        self.out = torch.full((7,), NAN, dtype=torch.float64, device="cuda")
        self.nbytes = 7 * k * 8

    def inputs(self):
        return [t for t in (self.gm.Xc, self.gm.y, self.wide, None if self.theta._base is self.wide else self.theta) if t is not None]

    def owned(self):
        return [self.out]

    def call(self, stream):
        self.gm.logpost(self.theta, out=self.out, stream=stream)

    def results(self):
        return {"out": self.out}


class RngRaw:
    """fmcmc_rng_stream_dev: df = 0 normal, -1 uniform, 3 Student-t variates"""

    def __init__(self, E, df, kz):
        import torch
        self.args = (99, 7, 3, 5, 33, kz, float(df))
        self.logu = torch.full((5, 33), NAN, dtype=torch.float64, device="cuda")
        self.z = torch.full((5, 33, kz), NAN, dtype=torch.float64, device="cuda")

    def inputs(self):
        return []

    def owned(self):
        return [self.logu, self.z]

    def call(self, stream):
        from fmcmc_amd import _abi as abi
        rc = abi.lib().fmcmc_rng_stream_dev(*self.args, self.logu.data_ptr(), self.z.data_ptr(), sptr(stream))
        assert rc == abi.OK, abi.last_error()

    def results(self):
        return {"logu": self.logu, "z": self.z}


class RngStream:
    """engine.rng_stream for the state and the kernel of the `mfma` shape"""

    def __init__(self, E):
        self.E, self.s = E, Sweep(E, *MFMA[:6])

    def call(self, stream):
        self.logu, self.z = self.E.rng_stream(self.s.st, self.s.gk, 32, seed=SEED, stream=stream)

    def results(self):
        return {"logu": self.logu, "z": self.z}


class Raw:
    """a raw call that tests/diag_dev.py or tests/gelman_dev.py prepared: what their `run` hook is given"""

    def __init__(self, inputs, buffers, call):
        self._inputs, self._owned, self._call, self.rc = inputs, buffers, call, None

    def inputs(self):
        return self._inputs

    def owned(self):
        return self._owned

    def call(self, stream):
        self.rc = self._call(sptr(stream))

    def results(self):
        return {}


def gated_raw(inputs, buffers, call):
    """the `run` hook of the raw calls: direction A, the stream handed over as hip_stream, enqueue-only"""
    raw = Raw(inputs, buffers, call)
    gated_a(raw, "passed", True)
    return raw.rc


BY_FORM = {s[-1]: s for s in SHAPES}
MFMA, LAT1 = BY_FORM["mfma"], BY_FORM["lat1"]
# name -> (knobs, factory(E)) of the sweeps through fmcmc_mcmc_run_dev that only enqueue
SWEEPS = {form: (s[6], (lambda s: lambda E: Sweep(E, *s[:6]))(s)) for form, s in BY_FORM.items()}
SWEEPS["mfma-window32"] = (dict(MFMA[6], window=32), lambda E: Sweep(E, *MFMA[:6], nsteps=100))
SWEEPS["mfma-fed"] = (MFMA[6], lambda E: Sweep(E, *MFMA[:6], fed=True))
ADAPT_OPTS = dict(warmup=5, Sd=2.38 ** 2 / 5)
BATCHES = {
    "linreg-lds": lambda E: Batch(E, LINREG, 3, 130, NORMAL),
    "linreg-stream": lambda E: Batch(E, LINREG, 3, 130, NORMAL, stream_data=True),
    "linreg-lds-mask": lambda E: Batch(E, LINREG, 3, 130, NORMAL, mask=[1, 0, 1]),
    "linreg-stream-mask": lambda E: Batch(E, LINREG, 3, 130, NORMAL, stream_data=True, mask=[1, 0, 1]),
    "logistic": lambda E: Batch(E, LOGISTIC, 4, 300, NORMAL),
    "linreg-adapt": lambda E: Batch(E, LINREG, 3, 130, ADAPT, opts=ADAPT_OPTS),
}
RNGS = {"%s-kz%d" % (name, kz): (lambda df, kz: lambda E: RngRaw(E, df, kz))(df, kz)
        for name, df in (("normal", 0.0), ("uniform", -1.0), ("t", 3.0)) for kz in (1, 5)}
LOGPOSTS = {"linreg": lambda E: Logpost(E, LINREG), "logistic": lambda E: Logpost(E, LOGISTIC), "iid": lambda E: Logpost(E, IID)}
MODES = ["current", "passed"]


def knobs_on(monkeypatch, knobs):
    for key, value in knobs.items():
        set_knob(monkeypatch, key, value)


def direction_a(make, E, mode, enqueue_only=True, form=None):
    import torch
    from fmcmc_amd import _abi as abi
    ref_case = make(E)
    ref = reference(ref_case)
    if form is not None and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert abi.last_kernel() == form
    case = make(E)
    gated_a(case, mode, enqueue_only)
    assert_same_bits(ref, snapshot(case.results()), "direction A (%s stream)" % mode)


# ---- A. the library's work stays on its stream ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SWEEPS))
def test_a_run_dev(E, monkeypatch, name, mode):
    """every form of test_gpu_route.SHAPES (prep kernels, stream fill, barrier memset, the cooperative and the long-data forms);
    `mfma` in step windows of 32 (several launches, fill_window_stream) and fed from engine.rng_stream"""
    knobs, make = SWEEPS[name]
    knobs_on(monkeypatch, knobs)
    direction_a(make, E, mode, form=name if name in BY_FORM else "mfma")


@pytest.mark.parametrize("mode", MODES)
def test_a_run_dev_null_mirrors(E, monkeypatch, mode):
    """kernel_host_view reads fixed / lb / ub back: on the call's stream, behind the copy of the true values"""
    knobs_on(monkeypatch, MFMA[6])
    direction_a(lambda E: Sweep(E, *MFMA[:6], null_mirrors=True), E, mode, enqueue_only=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(BATCHES))
def test_a_run_batch_sel_dev(E, name, mode):
    direction_a(BATCHES[name], E, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("what", ["fun", "user-fun", "user-model"])
def test_a_callbacks(E, what, mode):
    direction_a(lambda E: Callback(E, what), E, mode, enqueue_only=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(LOGPOSTS))
def test_a_logpost_dev(E, name, mode):
    direction_a(LOGPOSTS[name], E, mode)


@pytest.mark.parametrize("name", list(RNGS))
def test_a_rng_stream_dev(E, name):
    direction_a(RNGS[name], E, "passed")


def hpd_case(N, run=None):
    from fmcmc_amd.summary import hpd_gap
    L, p = diag_dev._lib(), len(diag_dev.COLS)
    work, out = diag_dev.device_call("fmcmc_hpd_dev", diag_dev.make_series(N, 5000 + N), N, (hpd_gap(N, 0.95),),
                                     (L.fmcmc_hpd_work_len(diag_dev.CHAINS, p), diag_dev.SERIES * 4), run)
    return {"work": gelman_dev._bits(work), "out": gelman_dev._bits(out)}


def autocov_case(N, run=None):
    L, p = diag_dev._lib(), len(diag_dev.COLS)
    lags = np.array([0, 1, 5, 10, 50], dtype=np.int64)
    work, out = diag_dev.device_call("fmcmc_autocov_dev", diag_dev.make_series(N, 6000 + N), N,
                                     (lags.ctypes.data_as(C.POINTER(C.c_int64)), int(lags.size)),
                                     (diag_dev.SERIES, L.fmcmc_autocov_out_len(diag_dev.CHAINS, p, lags.size)), run)
    return {"work": gelman_dev._bits(work), "out": gelman_dev._bits(out)}


def gelman_case(p, N, run=None):
    """p = 3: the columns (2, 0, 3) of k = 4; p = 65, the narrowest width beyond 64: a shuffled 65 of 68"""
    k = 4 if p == 3 else p + 3
    S = diag_dev.ROW0 + N + 3
    x = gelman_dev.make_chains(diag_dev.CHAINS, k, S, 70000 + p + N)
    cols = np.asarray(diag_dev.COLS if p == 3 else np.random.default_rng(p).permutation(k)[:p], dtype=np.int32)
    work, part = gelman_dev.device_partial(x, cols, diag_dev.ROW0, N, run=run)
    return {"work": gelman_dev._bits(work).ravel(), "partial": gelman_dev._bits(part)}


def groups_case(entry, N, mask=None, run=None):
    """fmcmc_gelman_groups_dev / fmcmc_summary_groups_dev on 3 groups x 2 chains, k = 4, the columns (2, 0, 3); mask: `active`"""
    import torch
    from fmcmc_amd import _abi as abi
    L, G, Cm, p, ROW0 = abi.lib(), 3, 2, len(diag_dev.COLS), diag_dev.ROW0
    x = np.concatenate([diag_dev.make_series(N, 7000 + N), diag_dev.make_series(N, 8000 + N)])
    xd = torch.as_tensor(x).cuda()
    cd = torch.as_tensor(np.asarray(diag_dev.COLS, dtype=np.int32)).cuda()
    ad = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.int32)).cuda()
    probs = np.asarray(diag_dev.PROBS, dtype=np.float64)
    if entry == "fmcmc_gelman_groups_dev":
        mid, lens = (), (L.fmcmc_gelman_groups_work_len(G, Cm, p), G * (L.fmcmc_gelman_partial_len(p) + 2))
    else:
        mid = (probs.ctypes.data_as(C.POINTER(C.c_double)), int(probs.size))
        lens = (L.fmcmc_summary_groups_work_len(G, Cm, p, probs.size), G * Cm * p * 4, G * L.fmcmc_summary_pooled_len(p, probs.size))
    bufs = [torch.full((int(n) + gelman_dev.GUARD,), NAN, dtype=torch.float64, device="cuda") for n in lens]
    call = lambda stream: getattr(L, entry)(xd.data_ptr(), G, Cm, x.shape[1], x.shape[2], ROW0, N, cd.data_ptr(), p,
                                            None if ad is None else ad.data_ptr(), *mid, *[b.data_ptr() for b in bufs], stream)
    rc = call(None) if run is None else run([xd, cd] + ([] if ad is None else [ad]), bufs, call)
    assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    return {"buffer%d" % i: b.cpu().numpy().view(np.uint64) for i, b in enumerate(bufs)}


LENGTHS = (1025, 19457)      # the second takes the re-read path of the selects: more passes
DIAGS = {}
for _N in LENGTHS:
    DIAGS.update({
        "summary_N%d" % _N: (diag_dev.summary_case, (_N,)),
        "summary_groups_N%d" % _N: (groups_case, ("fmcmc_summary_groups_dev", _N)),
        "summary_groups_mask_N%d" % _N: (groups_case, ("fmcmc_summary_groups_dev", _N, [1, 0, 1])),
        "heidel_N%d" % _N: (diag_dev.heidel_case, (_N,)),
        "chain_order_N%d" % _N: (diag_dev.order_case, (_N, 16)),
        "raftery_N%d" % _N: (diag_dev.raftery_case, (_N, 0.025, 1, 16)),
        "hpd_N%d" % _N: (hpd_case, (_N,)),
        "autocov_N%d" % _N: (autocov_case, (_N,)),
        "gelman_p3_N%d" % _N: (gelman_case, (3, _N)),
        "gelman_p65_N%d" % _N: (gelman_case, (65, _N)),
        "gelman_groups_N%d" % _N: (groups_case, ("fmcmc_gelman_groups_dev", _N)),
        "gelman_groups_mask_N%d" % _N: (groups_case, ("fmcmc_gelman_groups_dev", _N, [1, 0, 1])),
    })


def same_case_bits(ref, got, what):
    assert_same_bits({n: np.asarray(v) for n, v in ref.items()}, {n: np.asarray(v) for n, v in got.items()}, what)


@pytest.mark.parametrize("name", list(DIAGS))
def test_a_diagnostics(E, name):
    """the raw calls of the device diagnostics (cross-correlation is fmcmc_gelman_partial_dev over all rows)"""
    fn, args = DIAGS[name]
    ref = fn(*args)
    same_case_bits(ref, fn(*args, run=gated_raw), "direction A (hip_stream)")


def leaves(obj, path="", out=None):
    """every array and number a result object holds, by the path that leads to it"""
    import torch
    out = {} if out is None else out
    if isinstance(obj, np.ndarray) and obj.dtype == object:
        obj = obj.tolist()
    if isinstance(obj, np.ndarray) or torch.is_tensor(obj):
        out[path] = obj
    elif obj is None or isinstance(obj, (bool, int, float, str, np.generic)):
        out[path] = np.asarray(repr(obj))
    elif isinstance(obj, dict):
        for key in sorted(obj, key=str):
            leaves(obj[key], "%s.%s" % (path, key), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            leaves(v, "%s[%d]" % (path, i), out)
    elif hasattr(obj, "__dict__") and not callable(obj):
        leaves(vars(obj), path, out)
    else:
        out[path] = np.asarray(type(obj).__name__)
    return out


class Wrapper:
    """a diagnostic of fmcmc_amd/summary.py on DeviceChains of 3 (batch: 3 x 2) chains, k = 4, 1025 rows: _samples is the gated input"""

    def __init__(self, E, fn, batch=False):
        import torch
        from fmcmc_amd.mcmc import DeviceChains, McmcBatch
        x = diag_dev.make_series(1025, 31)
        if batch:
            x = np.concatenate([x, diag_dev.make_series(1025, 32)])
        self.smp = torch.as_tensor(x).cuda()
        dc = DeviceChains(self.smp, None, None, np.arange(1, x.shape[2] + 1), 1, None, 0, x.shape[0])
        self.arg, self.fn, self.out = McmcBatch(dc, 3, 2) if batch else dc, fn, None

    def inputs(self):
        return [self.smp]

    def owned(self):
        return []

    def call(self, stream):
        assert stream is None     # (the wrappers take torch's current stream)
        self.out = self.fn(self.arg)

    def results(self):
        return leaves(self.out)


WRAPPERS = {
    "summary": lambda x: x.summary(), "effective_size": lambda x: x.effective_size(), "geweke": lambda x: x.geweke(),
    "gelman_diag": lambda x: x.gelman_diag(), "heidel": lambda x: x.heidel(), "raftery_diag": lambda x: x.raftery_diag(),
    "chain_quantiles": lambda x: x.chain_quantiles(), "hpd_interval": lambda x: x.hpd_interval(),
    "autocorr_diag": lambda x: x.autocorr_diag(), "crosscorr": lambda x: x.crosscorr(),
}


@pytest.mark.parametrize("name", list(WRAPPERS) + ["batch_summary"])
def test_a_python_diagnostics(E, name):
    """under `with torch.cuda.stream(side)`: the wrappers enqueue on torch's current stream and read back on it"""
    make = (lambda E: Wrapper(E, lambda b: b.summary(), batch=True)) if name == "batch_summary" else (lambda E: Wrapper(E, WRAPPERS[name]))
    direction_a(make, E, "current", enqueue_only=False)


def test_a_mcmc_with_a_checker(E):
    """MCMC(..., conv_checker = convergence_gelman()) of 2 chains x 200 steps inside a side-stream context behind a gate equals
    the same call outside it"""
    import torch
    import fmcmc_amd as f
    X, y, _, init = route_data(LINREG, 1, 300, 2)

    def run():
        chk = f.convergence_gelman(100, threshold=1.0001)
        ans = f.MCMC(init, f.gaussian_linreg(X, y), 200, seed=99, nchains=2, kernel=f.kernel_normal(scale=0.05), conv_checker=chk)
        return leaves({"samples": ans.as_array(), "iters": np.asarray(ans.iters), "history": [list(h) for h in chk.history]})

    ref = snapshot(run())
    side = side_streams()[0]
    quiet_host()
    Gate(side)
    try:
        with torch.cuda.stream(side):
            got = run()
    finally:
        side.synchronize()
        torch.cuda.synchronize()
    assert_same_bits(ref, snapshot(got), "MCMC under torch.cuda.stream(side)")


# ---- B. Python-side preparation is ordered before the engine's stream -------------------------------------------------------------------
def direction_b(make, E):
    """(a run of the call on the side stream comes first: the stream's queue and the scratch the library allocates in stream order
    exist by then, so the gated call is on the device well within the gate's time, where a late fill or copy shows)"""
    import torch
    ref_case = make(E)
    ref = reference(ref_case)
    side = side_streams()[0]
    make(E).call(side)
    side.synchronize()
    torch.cuda.synchronize()
    scribble(getattr(ref_case, "nbytes", 512))
    case = make(E)
    gated_b(case, side)
    assert_same_bits(ref, snapshot(case.results()), "direction B (gate on torch's current stream, stream=side)")


B_CASES = {
    "sweep-mfma": (MFMA[6], SWEEPS["mfma"][1]),
    "sweep-lat1": (LAT1[6], SWEEPS["lat1"][1]),
    "sweep_batch": ({}, BATCHES["linreg-lds"]),
    "sweep_batch-mask": ({}, BATCHES["linreg-lds-mask"]),
    "sweep_user-model": ({}, lambda E: Callback(E, "user-model")),
    "sweep_user-fun": ({}, lambda E: Callback(E, "user-fun")),
    "sweep-fun": ({}, lambda E: Callback(E, "fun")),
    "rng_stream": (MFMA[6], lambda E: RngStream(E)),
}


@pytest.mark.parametrize("name", list(B_CASES))
def test_b_prepared_before_the_stream(E, monkeypatch, name):
    knobs, make = B_CASES[name]
    knobs_on(monkeypatch, knobs)
    direction_b(make, E)


@pytest.mark.parametrize("fam", [LINREG, LOGISTIC], ids=["linreg", "logistic"])
def test_b_logpost_of_a_column_slice(E, fam):
    """DeviceModel.logpost copies a non-contiguous theta on torch's current stream: the side stream has to wait for that copy.
    The temporary comes from the caching allocator, which may hand out the block an earlier call's copy lay in -- so the runs that
    warm the code object and the side stream are made at OTHER points, and the reference run comes last: a copy read too early
    holds those points, the NaNs of scribble(), or anything but the points of this call."""
    import torch
    side = side_streams()[0]
    for stream in (None, side):
        warm = Logpost(E, fam, sliced=True, shift=1.0)
        warm.call(stream)
    side.synchronize()
    torch.cuda.synchronize()
    scribble(warm.nbytes)
    case = Logpost(E, fam, sliced=True)
    gated_b(case, side)
    got = snapshot(case.results())
    assert np.isfinite(got["out"]).all()
    assert_same_bits(reference(Logpost(E, fam, sliced=True)), got, "direction B (gate on torch's current stream, stream=side)")


# ---- C. the check must see the stream ---------------------------------------------------------------------------------------------------
def failing_sweep(E):
    """the failing call of test_gpu_parity.test_nan_logpost_is_reported: n = 300, p = 1, 2 chains, sigma0 = 0.05, scale 1, no guard"""
    from conftest import synth_linreg
    X, y = synth_linreg(300, 1, 2)
    s = Sweep(E, LINREG, 1, 300, NORMAL, 2, {}, nsteps=200, guard=False, init=np.array([[0, 0, 0.05]] * 2), scale=1.0)
    s.gm = E.DeviceModel(LINREG, X, y, guard=False)
    return X, y, s


def test_c_check_sees_the_stream(E, O, monkeypatch):
    import torch
    set_knob(monkeypatch, "lat", "0")
    X, y, s = failing_sweep(E)
    ro = O.run(O.Model(O.FAM_LINREG, X, y, guard=False), O.Kernel(O.K_NORMAL, 3, scale=1.0), np.array([[0, 0, 0.05]] * 2), nsteps=200,
               seed=SEED)
    assert (ro.status == 1).any()
    s.call(None)                                    # warm
    torch.cuda.synchronize()
    assert np.array_equal(s.res.status.cpu().numpy(), ro.status)
    with pytest.raises(RuntimeError, match="undefined"):      # (the path of the check is warm too: it reads within the gate's time)
        failing_sweep(E)[2].call(None, check=True)
    # check=True: raises although the status is written behind the gate
    _, _, s = failing_sweep(E)
    side = side_streams()[0]
    quiet_host()
    Gate(side)
    try:
        with pytest.raises(RuntimeError, match="undefined"):
            s.call(side, check=True)
    finally:
        side.synchronize()
        torch.cuda.synchronize()
    # check=False: returns with the gate closed
    _, _, s = failing_sweep(E)
    quiet_host()
    gate = Gate(side)
    t0 = time.perf_counter()
    s.call(side, check=False)
    host_ms = 1e3 * (time.perf_counter() - t0)
    closed = gate.closed()
    side.synchronize()
    torch.cuda.synchronize()
    assert closed, gate.too_short(host_ms)
    assert np.array_equal(s.res.status.cpu().numpy(), ro.status)


# ---- D. two calls at once ---------------------------------------------------------------------------------------------------------------
def overlapped(a, b):
    """a and b, each behind a gate on a side stream of its own, both enqueued before either gate opens"""
    import torch
    sa, sb = side_streams()
    quiet_host()
    ga, gb = Gate(sa), Gate(sb)
    t0 = time.perf_counter()
    try:
        a.call(sa)
        b.call(sb)
        host_ms = 1e3 * (time.perf_counter() - t0)
        closed = ga.closed(), gb.closed()
    finally:
        sa.synchronize()
        sb.synchronize()
        torch.cuda.synchronize()
    assert closed[0], ga.too_short(host_ms)
    assert closed[1], gb.too_short(host_ms)


def test_d_mfma_with_lat1(E, monkeypatch):
    """(the knob lat=0 of the `mfma` shape would hold for both calls: the second shape is `lat1` under its own knobs, so each
    pair of runs, serial and overlapped, is made under the knobs of its shape -- the knobs are read when a call is planned)"""
    refs = []
    for shape in (MFMA, LAT1):
        with monkeypatch.context() as m:
            knobs_on(m, shape[6])
            refs.append(reference(Sweep(E, *shape[:6])))
    a, b = Sweep(E, *MFMA[:6]), Sweep(E, *LAT1[:6])

    class Planned:
        """a.call under the knobs of its shape"""

        def __init__(self, case, knobs):
            self.case, self.knobs = case, knobs

        def call(self, stream):
            with monkeypatch.context() as m:
                knobs_on(m, self.knobs)
                self.case.call(stream)

    overlapped(Planned(a, MFMA[6]), Planned(b, LAT1[6]))
    assert_same_bits(refs[0], snapshot(a.results()), "mfma next to lat1")
    assert_same_bits(refs[1], snapshot(b.results()), "lat1 next to mfma")


def test_d_batch_with_summary(E):
    ref_b, ref_s = reference(BATCHES["linreg-lds"](E)), diag_dev.summary_case(1025)
    b = BATCHES["linreg-lds"](E)
    got_s = diag_dev.summary_case(1025, run=lambda i, o, c: _overlap_raw(b, Raw(i, o, c)))
    assert_same_bits(ref_b, snapshot(b.results()), "batch-lds next to fmcmc_summary_dev")
    same_case_bits(ref_s, got_s, "fmcmc_summary_dev next to batch-lds")


def _overlap_raw(a, raw):
    overlapped(a, raw)
    return raw.rc


def test_d_gelman_with_raftery(E):
    ref_g, ref_r = gelman_case(3, 1025), diag_dev.raftery_case(1025, 0.025, 1, 16)
    got = {}

    def outer(i, o, c):
        g = Raw(i, o, c)
        got["raftery"] = diag_dev.raftery_case(1025, 0.025, 1, 16, run=lambda i2, o2, c2: _overlap_raw(g, Raw(i2, o2, c2)))
        return g.rc

    got["gelman"] = gelman_case(3, 1025, run=outer)
    same_case_bits(ref_g, got["gelman"], "fmcmc_gelman_partial_dev next to fmcmc_raftery_dev")
    same_case_bits(ref_r, got["raftery"], "fmcmc_raftery_dev next to fmcmc_gelman_partial_dev")
