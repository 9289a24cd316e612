"""Device-level front end of the HIP engine: torch tensors are only used as HBM buffers whose
data_ptr() goes through the C-ABI (include/fmcmc_amd.h, fmcmc_mcmc_run_dev).  One call ==
one MCMC_without_conv_checker over all local chains (R/mcmc.R:485-838)."""
import ctypes as C

import numpy as np
import torch

from . import _abi as abi

DBL_MAX = float(np.finfo(np.float64).max)


def _dev(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError("fmcmc_amd needs an AMD GPU (HIP device); there is no CPU fallback.")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _t(a, dtype, device):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(device).contiguous()


def _call_stream(stream, dev, made=()):
    """The stream of a call: `stream`, or torch's current stream of `dev`.  The one rule of every `stream=` of this module: with
    stream = s the call starts behind torch's current stream as it stands at the call (s.wait_stream(current): what the caller
    and this module prepared there -- inputs, NaN and zero fills of the outputs, contiguous copies -- is done before the first
    launch), its results are ordered on s, and check=True waits for s.  made: tensors this module allocated on the current stream
    for the call; they are recorded on s, so that the caching allocator does not hand their memory out again on the current stream
    while s still works on them.  Nothing happens when s is the current stream.  Call it after the last preparation."""
    cur = torch.cuda.current_stream(dev)
    if stream is None or stream == cur:
        return cur
    stream.wait_stream(cur)
    for t in made:
        if t is not None:
            t.record_stream(stream)
    return stream


class DeviceModel:
    """Shared read-only data of a log-posterior family, resident in HBM (fmcmc_model)."""

    def __init__(self, family, X, y, intercept=True, guard=True, prior_div=0.0, device=None):
        self.device = _dev(device)
        if torch.is_tensor(y):
            y = y.to(self.device, torch.float64).contiguous()
        else:
            y = _t(np.asarray(y, dtype=np.float64), torch.float64, self.device)
        n = y.shape[0]
        if X is None:
            Xc, p = None, 0
        else:
            if torch.is_tensor(X):
                X = X.to(self.device, torch.float64)
                if X.ndim == 1:
                    X = X[:, None]
                Xc = X.t().contiguous()  # [p][n] == column-major n x p
            else:
                X = np.asarray(X, dtype=np.float64)
                if X.ndim == 1:
                    X = X[:, None]
                Xc = _t(X.T, torch.float64, self.device)
            p = Xc.shape[0]
            if Xc.shape[1] != n:
                raise ValueError("X has %d rows but y has %d" % (Xc.shape[1], n))
            if p == 0:
                Xc = None
        self.family, self.Xc, self.y, self.n, self.p = family, Xc, y, int(n), int(p)
        self.intercept, self.guard, self.prior_div = int(bool(intercept)), int(bool(guard)), float(prior_div)

    @property
    def k(self):
        if self.family == abi.FAM_GAUSSIAN_LINREG:
            return self.intercept + self.p + 1
        if self.family == abi.FAM_LOGISTIC:
            return self.intercept + self.p
        return 2

    def c(self):
        return abi.Model(self.family, self.p, self.n, self.Xc.data_ptr() if self.Xc is not None else None,
                         self.y.data_ptr(), self.intercept, self.guard, self.prior_div)

    def logpost(self, theta, out=None, stream=None):
        """The family's canonical log-posterior of every row of theta [C, k] (a float64 tensor on this device) -> [C]
        (fmcmc_logpost_dev): the value the sweeps evaluate, bit for bit, enqueued on `stream` (torch's current one; the rule of
        _call_stream: the call starts behind torch's current stream, a non-contiguous theta is copied there first)."""
        if not torch.is_tensor(theta) or theta.dtype != torch.float64 or theta.ndim != 2 or theta.shape[1] != self.k or \
                not _on(theta, self.device):
            raise ValueError("DeviceModel.logpost: theta must be a float64 tensor of shape [C, %d] on %s; got %s" % (
                self.k, self.device, _describe(theta)))
        made = []
        if not theta.is_contiguous():
            theta = theta.contiguous()
            made.append(theta)
        if out is None:
            out = torch.empty(theta.shape[0], dtype=torch.float64, device=self.device)
            made.append(out)
        if theta.shape[0] == 0:
            return out
        stream = _call_stream(stream, self.device, made)
        cm = self.c()
        with torch.cuda.device(self.device):
            rc = abi.lib().fmcmc_logpost_dev(C.byref(cm), theta.data_ptr(), theta.shape[0], out.data_ptr(),
                                             C.c_void_p(stream.cuda_stream))
        if rc in (abi.ERR_ARG, abi.ERR_UNSUPPORTED):
            raise ValueError(abi.last_error())
        if rc != abi.OK:
            raise RuntimeError("fmcmc_logpost_dev failed (%d): %s" % (rc, abi.last_error()))
        return out


class DeviceModelBatch:
    """D datasets of one family and one shape, resident in HBM as X [D][p][n] and y [D][n] (fmcmc_mcmc_run_batch_dev):
    Xs [D, n, p] (or [D, n], or None when p = 0), ys [D, n]."""

    def __init__(self, family, Xs, ys, intercept=True, guard=True, prior_div=0.0, device=None):
        self.device = _dev(device)
        ys = np.asarray(ys, dtype=np.float64)
        if ys.ndim != 2 or ys.shape[0] < 1:
            raise ValueError("ys must be [D, n] with D >= 1; got shape %s" % (ys.shape,))
        D, n = ys.shape
        if Xs is None:
            Xc, p = None, 0
        else:
            Xs = np.asarray(Xs, dtype=np.float64)
            if Xs.ndim == 2:
                Xs = Xs[:, :, None]
            if Xs.ndim != 3 or Xs.shape[0] != D or Xs.shape[1] != n:
                raise ValueError("Xs must be [D, n, p] = [%d, %d, p]; got shape %s" % (D, n, Xs.shape))
            p = Xs.shape[2]
            Xc = _t(Xs.transpose(0, 2, 1), torch.float64, self.device) if p else None   # [D][p][n]
        self.family, self.Xc, self.y, self.n, self.p, self.nmodels = family, Xc, _t(ys, torch.float64, self.device), int(n), int(p), int(D)
        self.intercept, self.guard, self.prior_div = int(bool(intercept)), int(bool(guard)), float(prior_div)

    k = DeviceModel.k

    def c(self):
        """fmcmc_model of dataset 0 (the shape of all of them)"""
        return abi.Model(self.family, self.p, self.n, self.Xc.data_ptr() if self.Xc is not None else None,
                         self.y.data_ptr(), self.intercept, self.guard, self.prior_div)

    x_stride = property(lambda self: self.p * self.n)
    y_stride = property(lambda self: self.n)


class DeviceFun:
    """A batched user-defined log-posterior (models.BatchedFun) bound to a device: what sweep() hands to
    fmcmc_mcmc_run_fun_dev instead of a family's fmcmc_model."""

    def __init__(self, fun, device=None):
        dev = _dev(device)
        # (an indexed device: what the tensors fn returns report as theirs, device="cuda" included)
        self.device = dev if dev.index is not None else torch.device(dev.type, torch.cuda.current_device())
        self.fun, self.k = fun, fun.k


class _DevArray:
    """A device buffer of the engine as a torch tensor, without a copy (__cuda_array_interface__, no stream: no sync)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2,
                                         "strides": None}


def _describe(t):
    return ("%s %s on %s" % (t.dtype, tuple(t.shape), t.device)) if torch.is_tensor(t) else type(t).__name__


def _on(t, dev):
    """is the tensor on `dev` (an un-indexed "cuda" names every GPU's tensors)"""
    return t.device.type == dev.type and (dev.index is None or t.device.index == dev.index)


class _Views:
    """The engine's device buffers as torch tensors, one per (address, shape) of a call."""

    def __init__(self, dev):
        self.dev, self.made = dev, {}

    def __call__(self, ptr, shape):
        key = (ptr, shape)
        if key not in self.made:
            self.made[key] = torch.as_tensor(_DevArray(ptr, shape), device=self.dev)
        return self.made[key]


def _logpost_trampoline(model, stream, view, caught):
    """model.fun.fn as a fmcmc_logpost_fn: an exception raised in fn is kept in `caught` and the trampoline returns non-zero
    (the engine abandons the call, FMCMC_ERR_FUN).  fn runs with the engine's stream as torch's current stream, so its work is
    ordered with the engine's launches whatever stream the call got."""
    dev, fn = model.device, model.fun.fn

    def trampoline(theta_p, nchains, k, out_p, stream_p, user):
        try:
            with torch.cuda.stream(stream):
                th = view(theta_p, (nchains, k))
                f = fn(th)
                if not torch.is_tensor(f) or f.dtype != torch.float64 or f.device != dev or tuple(f.shape) != (nchains,):
                    raise ValueError("batched_fun: fn(theta) must return a float64 tensor of shape [%d] on %s; got %s" % (
                        nchains, dev, _describe(f)))
                view(out_p, (nchains,)).copy_(f)
            return 0
        except BaseException as e:   # (nothing may unwind through the C frames)
            caught.append(e)
            return 1

    return abi.LOGPOST_FN(trampoline)


def _run_fun_dev(model, ck, crun, cs, cout, stream):
    """fmcmc_mcmc_run_fun_dev with model.fun.fn behind a ctypes trampoline; an exception raised in fn is raised again here,
    after the C call has returned."""
    L = abi.lib()
    dev = model.device
    caught = []
    cb = _logpost_trampoline(model, stream, _Views(dev), caught)
    with torch.cuda.device(dev):
        rc = L.fmcmc_mcmc_run_fun_dev(C.byref(ck), C.byref(crun), C.byref(cs), C.byref(cout), cb, None,
                                      C.c_void_p(stream.cuda_stream))
    if caught:
        raise caught[0]
    return rc


class KernelSpec:
    """Expanded (recycled) kernel parameters on the device (fmcmc_kernel)."""

    def __init__(self, kind, k, mu, scale, lb, ub, fixed, scheme=abi.SCHEME_JOINT, freq=1, warmup=0,
                 bw=0, until=float("inf"), eps=1e-4, arate=0.234, Sd=0.0, scheme_seq=None, constr=None, nadapt=4,
                 ram_qfun=0, ram_df=0.0, ram_eta_exp=0.0, device=None):
        self.device = _dev(device)
        self.kind, self.k = int(kind), int(k)
        self.h_fixed = np.ascontiguousarray(np.asarray(fixed, dtype=np.uint8))
        self.kf = int((self.h_fixed == 0).sum())
        # host mirrors of what fmcmc_mcmc_run_dev checks and sizes its launch with (fmcmc_kernel.h_*): with them the
        # entry point only enqueues work
        self.h_lb = np.ascontiguousarray(np.asarray(lb, dtype=np.float64))
        self.h_ub = np.ascontiguousarray(np.asarray(ub, dtype=np.float64))
        self.h_scale = np.ascontiguousarray(np.asarray(scale, dtype=np.float64))
        self.h_seq = None if scheme_seq is None else np.ascontiguousarray(np.asarray(scheme_seq, dtype=np.int32))
        self.mu = _t(mu, torch.float64, self.device)
        self.scale = _t(scale, torch.float64, self.device)
        self.lb = _t(lb, torch.float64, self.device)
        self.ub = _t(ub, torch.float64, self.device)
        self.fixed = _t(self.h_fixed, torch.uint8, self.device)
        self.scheme, self.freq, self.warmup, self.bw = int(scheme), int(freq), int(warmup), int(bw)
        self.until, self.eps, self.arate, self.Sd = float(until), float(eps), float(arate), float(Sd)
        self.nadapt = int(nadapt)
        # kernel_ram's built-in qfun / eta families (fmcmc_kernel.ram_*; zeros = the defaults of R/kernel_ram.R:67-68)
        self.ram_qfun, self.ram_df, self.ram_eta_exp = int(ram_qfun), float(ram_df), float(ram_eta_exp)
        # explicit update sequence: 0-based parameter indices (R/kernel.R:69-92); ram: constr[which., which.] mask
        self.scheme_seq = None if scheme_seq is None else _t(np.asarray(scheme_seq, dtype=np.int32), torch.int32, self.device)
        self.constr = None if constr is None else _t(np.asarray(constr, dtype=np.float64).reshape(self.kf, self.kf),
                                                      torch.float64, self.device)

    @property
    def kz(self):
        """proposal variates per step: one for the single-parameter schemes (R/kernel_normal.R:63)."""
        return 1 if (self.kind in abi.SIMPLE_KERNELS and self.scheme != abi.SCHEME_JOINT) else self.kf

    def c(self):
        return abi.Kernel(self.kind, self.k, self.mu.data_ptr(), self.scale.data_ptr(), self.lb.data_ptr(),
                          self.ub.data_ptr(), self.fixed.data_ptr(), self.scheme, self.freq, self.warmup,
                          self.bw, self.until, self.eps, self.arate, self.Sd,
                          self.scheme_seq.data_ptr() if self.scheme_seq is not None else None,
                          int(self.scheme_seq.numel()) if self.scheme_seq is not None else 0, self.nadapt,
                          self.constr.data_ptr() if self.constr is not None else None,
                          self.h_fixed.ctypes.data, self.h_lb.ctypes.data, self.h_ub.ctypes.data, self.h_scale.ctypes.data,
                          self.h_seq.ctypes.data if self.h_seq is not None else None,
                          self.ram_qfun, 0, self.ram_df, self.ram_eta_exp)


class ChainState:
    """fmcmc_state in HBM: last row of every chain + the kernels' persistent environments."""

    def __init__(self, initial, kf, device=None):
        self.device = _dev(device)
        th = torch.as_tensor(np.ascontiguousarray(initial), dtype=torch.float64) if not torch.is_tensor(initial) else initial
        self.theta0 = th.to(self.device, torch.float64).contiguous().clone()
        Cn = self.theta0.shape[0]
        z = dict(device=self.device)
        self.f0 = torch.zeros(Cn, dtype=torch.float64, **z)
        self.abs_iter = torch.zeros(Cn, dtype=torch.int64, **z)
        self.Sigma = torch.zeros(Cn, kf, kf, dtype=torch.float64, **z)
        self.mean_prev = torch.zeros(Cn, kf, dtype=torch.float64, **z)
        self.have_mean = torch.zeros(Cn, dtype=torch.int32, **z)
        self.nerrors = torch.zeros(Cn, dtype=torch.int32, **z)
        self.scheme_cols = None   # [C][nsteps] int32: plan of scheme = "random" (fmcmc_state.scheme_cols)
        k = self.theta0.shape[1]
        self.mirror_mu = torch.zeros(Cn, k, dtype=torch.float64, **z)      # mirror kernels: adapted mean / scale
        self.mirror_scale = torch.zeros(Cn, k, dtype=torch.float64, **z)
        self.obs_arate = torch.full((Cn, k), float("nan"), dtype=torch.float64, **z)   # (R's obs_arate: a k-vector after warm-up updates)
        self.fresh = 1
        self.step_base = 0

    def c(self, nsteps=None):
        cols = self.scheme_cols
        if cols is not None and nsteps is not None and cols.shape[1] != nsteps:
            if cols.shape[1] < nsteps:   # R: update_sequence[env$i, ] beyond the rows of the kernel's first call
                raise IndexError("subscript out of bounds: the update plan of this kernel has %d rows" % cols.shape[1])
            cols = cols[:, :nsteps].contiguous()
        self._cols_keep = cols      # (alive while the call runs; a copy made here is among the call's _made_for_call)
        return abi.State(self.theta0.data_ptr(), self.f0.data_ptr(), self.abs_iter.data_ptr(),
                         self.Sigma.data_ptr(), self.mean_prev.data_ptr(), self.have_mean.data_ptr(),
                         self.nerrors.data_ptr(), self.fresh, 0, cols.data_ptr() if cols is not None else None,
                         self.mirror_mu.data_ptr(), self.mirror_scale.data_ptr(), self.obs_arate.data_ptr())


class SweepResult:
    pass


def kept_rows(nsteps, burnin, thin):
    return (nsteps - burnin) // thin


def sweep(model, kernel, state, nsteps, burnin=0, thin=1, seed=0, chain_base=0,
          want_logpost=True, want_draws=True, want_bits=True, fed_logu=None, fed_z=None,
          stream=None, check=True, into=None, row0=0):
    """Enqueue one sweep (all local chains, nsteps iterations) and return the output tensors.

    into = (samples [C][k][cap], logpost [C][cap] or None, draws [C][k][cap] or None), row0: write the kept rows of this
    call at rows row0.. of a preallocated history (fmcmc_out.ld_rows = cap) instead of allocating; the result then holds
    views of those rows.

    model: a DeviceModel (a closed-form family) or a DeviceFun (a batched user-defined log-posterior, called between the
    engine's launches with `stream` as torch's current stream).

    stream: the stream of the call (None: torch's current stream).  With stream = s the call starts behind torch's current stream
    as it stands at the call, its results are ordered on s, and check=True waits for s (_call_stream).

    Raises ValueError for argument errors (messages mirror the reference's stop() texts) and
    RuntimeError for chain errors ("fun(par) is undefined", R/mcmc.R:758-765)."""
    L = abi.lib()
    dev = state.device
    out, crun, cout = _call_buffers(state, nsteps, burnin, thin, seed, chain_base, want_logpost, want_draws, want_bits,
                                    fed_logu, fed_z, into, row0)
    Cn, k = state.theta0.shape
    rng_mode = crun.rng_mode
    if kernel.kind in abi.SIMPLE_KERNELS and kernel.scheme == abi.SCHEME_RANDOM and state.scheme_cols is None:
        if rng_mode == abi.RNG_FED:
            raise ValueError("rng_mode = FED with scheme = 'random' needs state.scheme_cols (the plan R drew)")
        state.scheme_cols = torch.zeros((Cn, nsteps), dtype=torch.int32, device=dev)
    if isinstance(model, DeviceFun) and k != model.k:
        raise ValueError("Incorrect length of -initial-: the model has %d parameters, got %d." % (model.k, k))
    cs = state.c(nsteps)
    # (the output buffers above were made and filled on the current stream: the engine's stream starts behind them)
    stream = _call_stream(stream, dev, _made_for_call(out, state))
    if isinstance(model, DeviceFun):
        rc = _run_fun_dev(model, kernel.c(), crun, cs, cout, stream)
    else:
        cm, ck = model.c(), kernel.c()
        with torch.cuda.device(dev):
            rc = L.fmcmc_mcmc_run_dev(C.byref(cm), C.byref(ck), C.byref(crun), C.byref(cs), C.byref(cout),
                                      C.c_void_p(stream.cuda_stream))
    return _finish_call(out, state, rc, "fmcmc_mcmc_run_fun_dev" if isinstance(model, DeviceFun) else "fmcmc_mcmc_run_dev",
                        nsteps, burnin, thin, chain_base, check, stream)


def sweep_batch(batch, kernel, state, nsteps, burnin=0, thin=1, seed=0, chain_base=0,
                want_logpost=True, want_draws=True, want_bits=True, fed_logu=None, fed_z=None,
                stream=None, check=True, into=None, row0=0, stream_data=False, active=None):
    """sweep() for one model on many datasets (fmcmc_mcmc_run_batch_sel_dev): batch is a DeviceModelBatch of D datasets, state
    holds D x chains_per_model chains, dataset by dataset -- local chain c samples dataset c // chains_per_model with the
    stream of global chain chain_base + c.  One launch runs every step of every chain; the keywords and the result are
    sweep()'s.  stream_data = True reads the datasets from global memory every step instead of holding each in LDS
    (FMCMC_BATCH_STREAM_DATA; the same bits).  active: None, or an int32 device tensor [D] -- the chains of a dataset whose
    entry is 0 do not run: their state, their rows of `into` and their entries of every output stay as they were (the
    outputs this call allocates: zeros, NaN samples).  stream: as for sweep()."""
    L = abi.lib()
    dev = state.device
    if active is not None and (not torch.is_tensor(active) or active.dtype != torch.int32 or tuple(active.shape) != (batch.nmodels,)
                               or not active.is_contiguous() or not _on(active, dev)):
        raise ValueError("sweep_batch(active=...): a contiguous int32 tensor of shape [%d] on %s is needed; got %s" % (
            batch.nmodels, dev, _describe(active)))
    out, crun, cout = _call_buffers(state, nsteps, burnin, thin, seed, chain_base, want_logpost, want_draws, want_bits,
                                    fed_logu, fed_z, into, row0)
    Cn, k = state.theta0.shape
    if k != batch.k:
        raise ValueError("Incorrect length of -initial-: the model has %d parameters, got %d." % (batch.k, k))
    if kernel.kind in abi.SIMPLE_KERNELS and kernel.scheme == abi.SCHEME_RANDOM and state.scheme_cols is None:
        if crun.rng_mode == abi.RNG_FED:
            raise ValueError("rng_mode = FED with scheme = 'random' needs state.scheme_cols (the plan R drew)")
        state.scheme_cols = torch.zeros((Cn, nsteps), dtype=torch.int32, device=dev)
    cm, ck, cs = batch.c(), kernel.c(), state.c(nsteps)
    stream = _call_stream(stream, dev, _made_for_call(out, state))
    with torch.cuda.device(dev):
        rc = L.fmcmc_mcmc_run_batch_sel_dev(C.byref(cm), batch.nmodels, batch.x_stride, batch.y_stride, C.byref(ck), C.byref(crun),
                                            C.byref(cs), C.byref(cout), active.data_ptr() if active is not None else None,
                                            abi.BATCH_STREAM_DATA if stream_data else 0, C.c_void_p(stream.cuda_stream))
    return _finish_call(out, state, rc, "fmcmc_mcmc_run_batch_sel_dev", nsteps, burnin, thin, chain_base, check, stream)


def _call_buffers(state, nsteps, burnin, thin, seed, chain_base, want_logpost, want_draws, want_bits, fed_logu, fed_z, into, row0):
    """The output tensors of one call (or the views of `into` it writes) with the fmcmc_run and fmcmc_out that point at them."""
    dev = state.device
    Cn, k = state.theta0.shape
    S = kept_rows(nsteps, burnin, thin)
    if S < 0:
        S = 0
    nwords = (nsteps + 31) // 32
    out = SweepResult()
    f64 = dict(dtype=torch.float64, device=dev)
    ld = 0
    if into is not None:
        hs, hl, hd = into
        ld = int(hs.shape[2])
        if row0 + S > ld or hs.shape[0] != Cn or hs.shape[1] != k or not hs.is_contiguous():
            raise ValueError("sweep(into=...): the history holds %s rows, this call writes rows %d..%d" % (ld, row0, row0 + S))
        want_logpost, want_draws = hl is not None, hd is not None
        out.samples = hs[:, :, row0:row0 + S]
        out.logpost = hl[:, row0:row0 + S] if want_logpost else None
        out.draws = hd[:, :, row0:row0 + S] if want_draws else None
    else:
        out.samples = torch.full((Cn, k, max(S, 0)), float("nan"), **f64)
        out.logpost = torch.empty((Cn, S), **f64) if want_logpost else None
        out.draws = torch.empty((Cn, k, S), **f64) if want_draws else None
    out.accept_count = torch.zeros(Cn, dtype=torch.int64, device=dev)
    out.accept_bits = torch.zeros((Cn, nwords), dtype=torch.int32, device=dev) if want_bits else None
    out.status = torch.zeros(Cn, dtype=torch.int32, device=dev)
    out.status_step = torch.zeros(Cn, dtype=torch.int64, device=dev)
    out.status_theta = torch.zeros((Cn, k), **f64)
    out._made = [out.accept_count, out.accept_bits, out.status, out.status_step, out.status_theta]
    if into is None:
        out._made += [out.samples, out.logpost, out.draws]
    rng_mode = abi.RNG_FED if fed_logu is not None else abi.RNG_PHILOX
    crun = abi.Run(Cn, nsteps, burnin, thin, seed & 0xFFFFFFFFFFFFFFFF, chain_base, state.step_base,
                   rng_mode, 0, fed_logu.data_ptr() if fed_logu is not None else None,
                   fed_z.data_ptr() if fed_z is not None else None)
    # (a view's data_ptr() is the address of its first element: row row0 of chain 0, parameter 0)
    cout = abi.Out(out.samples.data_ptr(), out.logpost.data_ptr() if want_logpost else None,
                   out.draws.data_ptr() if want_draws else None, out.accept_count.data_ptr(),
                   out.accept_bits.data_ptr() if want_bits else None, out.status.data_ptr(),
                   out.status_step.data_ptr(), out.status_theta.data_ptr(), ld)
    return out, crun, cout


def _made_for_call(out, state):
    """the tensors _call_buffers and ChainState.c() allocated for this call (for _call_stream)"""
    made = list(out._made)
    if state._cols_keep is not None and state._cols_keep is not state.scheme_cols:
        made.append(state._cols_keep)
    return made


def _finish_call(out, state, rc, entry, nsteps, burnin, thin, chain_base, check, stream=None):
    """The return code of an entry point raised as sweep() documents it; the state advanced, the result labelled.  check: the
    chains' statuses are read back, after the work on `stream`."""
    if rc in (abi.ERR_ARG, abi.ERR_UNSUPPORTED):
        raise ValueError(abi.last_error())
    if rc != abi.OK:
        raise RuntimeError("%s failed (%d): %s" % (entry, rc, abi.last_error()))
    state.fresh = 0
    state.step_base += nsteps
    out.iters = burnin + thin * np.arange(1, max(kept_rows(nsteps, burnin, thin), 0) + 1)
    out.thin, out.nsteps, out.burnin = thin, nsteps, burnin
    if check:
        raise_on_chain_error(out, chain_base, stream)
    return out


def rng_stream(state, kernel, nsteps, seed=0, chain_base=0, logu=None, z=None, stream=None):
    """Canonical Philox stream of the next sweep of `state` in HBM (fmcmc_rng_stream_dev); pass the returned
    tensors as fed_logu / fed_z to sweep(): bit-identical to the in-library stream, buffers reusable.  stream: as for sweep()."""
    L = abi.lib()
    dev = state.device
    Cn = state.theta0.shape[0]
    kz = kernel.kz
    made = []
    if logu is None:
        logu = torch.empty((Cn, nsteps), dtype=torch.float64, device=dev)
        made.append(logu)
    if z is None:
        z = torch.empty((Cn, nsteps, kz), dtype=torch.float64, device=dev)
        made.append(z)
    stream = _call_stream(stream, dev, made)
    # the variate family the kernel's own in-library stream draws (mh_engine.hip, launch_sweep): kernel_ram's qfun families
    # (fmcmc_kernel.ram_qfun: rt(k, k) / rnorm(k) / rt(k, df)), U(0,1) for the uniform kernels, N(0,1) otherwise
    if kernel.kind == abi.KERNEL_RAM:
        df = {abi.RAM_QFUN_NORMAL: 0.0, abi.RAM_QFUN_T_DF: kernel.ram_df}.get(kernel.ram_qfun, float(kernel.kf))
    elif kernel.kind in (abi.KERNEL_UNIF, abi.KERNEL_UNIF_REFLECTIVE, abi.KERNEL_UMIRROR):
        df = -1.0
    else:
        df = 0.0
    with torch.cuda.device(dev):
        rc = L.fmcmc_rng_stream_dev(seed & 0xFFFFFFFFFFFFFFFF, state.step_base, chain_base, Cn, nsteps, kz, float(df),
                                    logu.data_ptr(), z.data_ptr(), C.c_void_p(stream.cuda_stream))
    if rc != abi.OK:
        raise RuntimeError("fmcmc_rng_stream_dev failed (%d): %s" % (rc, abi.last_error()))
    return logu, z


RNG_BLOCK = 256   # loop steps per fill of UserEnv's variates


class UserEnv:
    """What proposal(env) and logratio(env) of a kernel_new() kernel see of a loop step, for ALL local chains at once
    (R/kernel.R:169-184); one object per call, updated in place.

      i, nsteps, k       R's 1-based loop index (2 .. nsteps), the steps and the parameters of the call
      theta0, f0         [C, k], [C]: the current states and their values
      theta1, f1         [C, k], [C]: in proposal(), the LAST proposal and its value; in logratio(), the new ones
      chain_ids          [C] int64: the global chain ids, chain_base + c
      kernel             the kernel object (its kernel_new(**state) are attributes, assignable)
      f(theta)           the model at [C, k] -> [C]
      rnorm(n) / runif(n) / rt(n, df)   [C, n]: the engine's counter-based variates of THIS step -- variate a of (seed,
                         step_base + i, global chain) is what a built-in kernel draws in slot a, whatever the split of the
                         chains over calls or ranks

    The tensors are float64 views of the engine's device buffers: read them, never write them.  There is no env.ans (kept
    rows are not R's rows): a kernel that needs its history keeps it in its own state."""

    def __init__(self, kernel, model, state, nsteps, seed, chain_base, stream, fed):
        self.kernel, self.nsteps, self.i = kernel, int(nsteps), 1
        self.theta0, self.f0 = state.theta0, state.f0
        self.theta1, self.f1 = state.theta0, state.f0
        Cn, self.k = state.theta0.shape
        self.chain_ids = chain_base + torch.arange(Cn, dtype=torch.int64, device=state.device)
        self._model, self._stream, self._fed = model, stream, fed
        self._seed, self._chain_base, self._step_base = seed & 0xFFFFFFFFFFFFFFFF, chain_base, state.step_base
        self._blocks = {}   # (variate family, n) -> (first step of the block, z [C][1 + RNG_BLOCK][n])

    def f(self, theta):
        if isinstance(self._model, DeviceFun):
            return self._model.fun.fn(theta)
        return self._model.logpost(theta, stream=self._stream)

    def _variates(self, n, df):
        if self._fed:
            raise RuntimeError("env.rnorm / env.runif / env.rt are the engine's own stream: a call with fed_logu has none.")
        n = int(n)
        if n < 1:
            raise ValueError("the number of variates must be >= 1.")
        blk = self._blocks.get((df, n))
        if blk is None or not blk[0] <= self.i < blk[0] + RNG_BLOCK:
            # fmcmc_rng_stream_dev fills the steps 1 .. nsteps behind a step_base and leaves step 1 (row 1 draws nothing) zero:
            # a block that starts at loop step b0 >= 2 is the fill behind step_base + b0 - 2, its row 0 unused
            b0 = max(self.i, 2)
            rows = min(RNG_BLOCK, self.nsteps - b0 + 1) + 1
            dev, Cn = self.theta0.device, self.theta0.shape[0]
            logu = torch.empty((Cn, rows), dtype=torch.float64, device=dev)
            z = torch.empty((Cn, rows, n), dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                rc = abi.lib().fmcmc_rng_stream_dev(self._seed, self._step_base + b0 - 2, self._chain_base, Cn, rows, n, float(df),
                                                    logu.data_ptr(), z.data_ptr(), C.c_void_p(self._stream.cuda_stream))
            if rc != abi.OK:
                raise RuntimeError("fmcmc_rng_stream_dev failed (%d): %s" % (rc, abi.last_error()))
            blk = self._blocks[(df, n)] = (b0, z)
        return blk[1][:, self.i - blk[0] + 1, :]

    def rnorm(self, n):
        return self._variates(n, 0.0)

    def runif(self, n):
        return self._variates(n, -1.0)

    def rt(self, n, df):
        df = float(df)
        if not 0.0 < df < float("inf"):
            raise ValueError("-df- must be finite and positive.")
        return self._variates(n, df)


def sweep_user(model, kernel, state, nsteps, burnin=0, thin=1, seed=0, chain_base=0, want_logpost=True, want_draws=True,
               want_bits=True, fed_logu=None, stream=None, check=True, into=None, row0=0):
    """sweep() under a user-defined transition kernel (kernels.kernel_new; fmcmc_mcmc_run_user_dev): per loop step
    kernel.proposal(env) -> theta1 [C, k], the evaluation (model: a DeviceModel, evaluated by the engine, or a DeviceFun),
    kernel.logratio(env) -> [C] when the kernel has one, and one launch of the engine's accept / store step.  The keywords and
    the result are sweep()'s; fed_logu feeds the accept uniforms (env.rnorm / runif / rt then raise).  The callbacks run with
    `stream` as torch's current stream (as for sweep()); an exception raised in one ends the call and is raised again here."""
    L = abi.lib()
    dev = state.device
    Cn, k = state.theta0.shape
    if k != model.k:
        raise ValueError("Incorrect length of -initial-: the model has %d parameters, got %d." % (model.k, k))
    out, crun, cout = _call_buffers(state, nsteps, burnin, thin, seed, chain_base, want_logpost, want_draws, want_bits,
                                    fed_logu, None, into, row0)
    cs = state.c(nsteps)
    env = UserEnv(kernel, model, state, nsteps, seed, chain_base, None, fed_logu is not None)
    # (the output buffers above and env.chain_ids were made on the current stream: the engine's stream starts behind them)
    stream = env._stream = _call_stream(stream, dev, _made_for_call(out, state) + [env.chain_ids])
    caught, view = [], _Views(dev)

    def step_fn(user_fn, what, shape):
        def trampoline(env_p, out_p, stream_p, user):
            try:
                with torch.cuda.stream(stream):
                    e = env_p.contents
                    env.i, env.theta1, env.f1 = int(e.i), view(e.theta1, (Cn, k)), view(e.f1, (Cn,))
                    t = user_fn(env)
                    if not torch.is_tensor(t) or t.dtype != torch.float64 or not _on(t, dev) or tuple(t.shape) != shape:
                        raise ValueError("kernel_new: %s(env) must return a float64 tensor of shape %s on %s; got %s" % (
                            what, list(shape), dev, _describe(t)))
                    view(out_p, shape).copy_(t)
                return 0
            except BaseException as ex:   # (nothing may unwind through the C frames)
                caught.append(ex)
                return 1
        return abi.STEP_FN(trampoline)

    fun_cb = _logpost_trampoline(model, stream, view, caught) if isinstance(model, DeviceFun) else abi.LOGPOST_FN()
    prop_cb = step_fn(kernel.proposal, "proposal", (Cn, k))
    ratio_cb = step_fn(kernel.logratio, "logratio", (Cn,)) if kernel.logratio is not None else abi.STEP_FN()
    cm = None if isinstance(model, DeviceFun) else model.c()
    with torch.cuda.device(dev):
        rc = L.fmcmc_mcmc_run_user_dev(C.byref(cm) if cm is not None else None, fun_cb, prop_cb, ratio_cb, None, k,
                                       C.byref(crun), C.byref(cs), C.byref(cout), C.c_void_p(stream.cuda_stream))
    if caught:
        raise caught[0]
    return _finish_call(out, state, rc, "fmcmc_mcmc_run_user_dev", nsteps, burnin, thin, chain_base, check, stream)


def raise_on_chain_error(out, chain_base=0, stream=None):
    """Raises the first chain error of a call's result.  stream: the stream the call ran on (None: torch's current one, which the
    copy below waits for); the statuses are read after its work."""
    if stream is not None:
        stream.synchronize()
    st = out.status.cpu().numpy()
    bad = np.nonzero(st)[0]
    if bad.size:
        if (st == abi.CHAIN_SYNC_TIMEOUT).any():
            raise RuntimeError("fmcmc_amd: a grid-wide hand-over of the observation-sharded evaluation timed out (a device "
                               "fault, or the workgroups of the sweep were not co-resident); the results of this call are "
                               "invalid. FMCMC_AMD_DEBUG=shard=0 selects the chain-sharded kernel.")
        c = int(bad[0])
        step = int(out.status_step[c].item())
        theta = out.status_theta[c].cpu().numpy()
        what = {abi.CHAIN_NAN_LOGPOST: "fun(par) is undefined (NaN).",
                abi.CHAIN_NAN_RATIO: "fun(par) is undefined (f1 - f0 is NaN).",
                abi.CHAIN_NOT_PD: "'Sigma' is not positive definite.",
                abi.CHAIN_BAD_WINDOW: "subscript out of bounds: the rows kernel_adapt(bw / freq) adapts on reach before the "
                                      "first row of this call."}.get(int(st[c]), "chain error.")
        # (R/mcmc.R:759-765 attaches the fun / lb / ub hint to a NaN log-posterior only)
        hint = " Check either -fun- or the -lb- and -ub- parameters." if int(st[c]) in (abi.CHAIN_NAN_LOGPOST, abi.CHAIN_NAN_RATIO) else ""
        raise RuntimeError(
            "%s%s This error ocurred during step i = %d "
            "(chain %d) and proposal parameters theta1 = %s" % (what, hint, step, chain_base + c, np.array2string(theta, precision=4)))
