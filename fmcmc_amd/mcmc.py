"""MCMC() and its helpers with the reference's signatures (R/mcmc.R:325-340).

  MCMC / MCMC.default / .mcmc / .mcmc.list   R/mcmc.R:325-479  -> MCMC
  MCMC_without_conv_checker                  R/mcmc.R:485-838  -> MCMC_without_conv_checker
  MCMC_with_conv_checker                     R/mcmc.R:841-1019 -> MCMC_with_conv_checker
  check_initial                              R/checks.R:22-58  -> check_initial
  append_chains                              R/append_chains.R -> append_chains
  MCMC_OUTPUT logpost / draws                R/mcmc.R:822-823, R/mcmc_info.R:351-365 -> get_logpost / get_draws

The per-chain loop itself (R/mcmc.R:720-838) is NOT here: it is the HIP sweep kernel reached through
engine.sweep() -> C-ABI fmcmc_mcmc_run_dev.  `multicore`/`cl` select nothing on a GPU (all chains of
the call already run concurrently); `fun` is a closed-form family or a batched_fun (a vectorised torch log-posterior the
engine calls between its kernels' steps); with torch.distributed initialised the chains are sharded over
the ranks in contiguous blocks (one process per GPU) and RCCL is used only by the Gelman check.
"""
import functools
import time
import warnings

import numpy as np

from . import _abi as abi
from . import engine
from .kernels import fmcmc_kernel, fmcmc_user_kernel, kernel_normal
from .models import BatchedFun, LogPosterior


# ------------------------------------------------------------------------------ coda-like containers
class Mcmc:
    """coda::mcmc: data [niter x nvar] + mcpar = (start, end, thin)."""

    def __init__(self, data, start=1, end=None, thin=1, varnames=None):
        self.data = np.asarray(data, dtype=np.float64)
        if self.data.ndim == 1:
            self.data = self.data[:, None]
        n = self.data.shape[0]
        if end is None:
            end = start + (n - 1) * thin
        if n and (end - start) // thin + 1 != n:
            raise ValueError("Start, end and thin incompatible with data")
        self.mcpar = (int(start), int(end), int(thin))
        self.varnames = list(varnames) if varnames is not None else ["par%d" % (j + 1) for j in range(self.data.shape[1])]
        self.iters = start + thin * np.arange(n)

    niter = property(lambda self: self.data.shape[0])
    nvar = property(lambda self: self.data.shape[1])
    nchain = property(lambda self: 1)
    thin = property(lambda self: self.mcpar[2])
    start = property(lambda self: self.mcpar[0])
    end = property(lambda self: self.mcpar[1])

    def __array__(self, dtype=None):
        return self.data if dtype is None else self.data.astype(dtype)

    def __len__(self):
        return self.niter

    def tail(self, n):
        """utils::tail as fmcmc uses it (R/mcmc.R:362,406): the last n+1 rows."""
        return self.data[-(n + 1):]

    def __repr__(self):
        return "<Mcmc niter=%d nvar=%d mcpar=%s>" % (self.niter, self.nvar, self.mcpar)


class McmcList(list):
    """coda::mcmc.list."""
    nchain = property(lambda self: len(self))
    nvar = property(lambda self: self[0].nvar)
    niter = property(lambda self: self[0].niter)
    thin = property(lambda self: self[0].thin)
    iters = property(lambda self: self[0].iters)

    def as_array(self):
        return np.stack([m.data for m in self])  # [C][S][k]


def check_initial(initial, nchains):
    """R/checks.R:22-58. Returns (matrix [nchains x k], names)."""
    names = None
    if isinstance(initial, dict):
        names, initial = list(initial.keys()), list(initial.values())
    if isinstance(initial, McmcList):
        return np.stack([m.data[-1] for m in initial]), initial[0].varnames
    a = np.asarray(initial, dtype=np.float64)
    if a.ndim <= 1:
        a = np.atleast_1d(a)
        if nchains > 1:
            warnings.warn("While using multiple chains, a single initial point has been passed via `initial`: c(%s). "
                          "The values will be recycled. Ideally you would want to start each chain from different "
                          "locations." % ", ".join(repr(float(v)) for v in a))
        if a.size == 0:
            raise ValueError("The `initial` vector is of length zero.")
        a = np.tile(a, (nchains, 1))
    elif a.ndim != 2:
        raise ValueError("When `initial` is not a numeric vector, it should be a matrix. Right now it is an "
                         "object of class `%s`." % type(initial).__name__)
    elif a.shape[0] != nchains:
        raise ValueError("The number of rows of `initial` (%d) must coincide with the number of chains (%d)."
                         % (a.shape[0], nchains))
    if names is None:
        names = ["par%d" % (j + 1) for j in range(a.shape[1])]
    return np.ascontiguousarray(a), names


def append_chains(*chains):
    """R/append_chains.R:64-143 (iteration labels continue across runs)."""
    chains = [c for c in chains if c is not None and len(c) > 0]
    if not chains:
        raise ValueError("No method available to append these chains.")
    if len(chains) == 1:
        return chains[0]
    if isinstance(chains[0], McmcList):
        ns = [len(c) for c in chains]
        if len(set(ns)) != 1:
            raise ValueError("All mcmc.list objects must have the same number of chains. The passed objects have "
                             "%s respectively." % ", ".join(map(str, ns)))
        return McmcList(append_chains(*[c[i] for c in chains]) for i in range(ns[0]))
    thins = [c.thin for c in chains]
    if len(set(thins)) != 1:
        raise ValueError("All `mcmc` objects have to have the same `thin` parameter.Observed: %s respectively."
                         % ", ".join(map(str, thins)))
    nv = [c.nvar for c in chains]
    if len(set(nv)) != 1:
        raise ValueError("All `mcmc` objects have to have the same number of parameters.Observed: %s respectively."
                         % ", ".join(map(str, nv)))
    data = np.concatenate([c.data for c in chains], axis=0)
    start, thin = chains[0].start, thins[0]
    end = start + (data.shape[0] - 1) * thin
    return Mcmc(data, start=start, end=end, thin=thin, varnames=chains[0].varnames)


# ------------------------------------------------------------------------------ MCMC_OUTPUT (R/mcmc_info.R)
class _Output:
    def __init__(self):
        self.clear()

    def clear(self):
        self.logpost, self.draws, self.elapsed, self.nchains = None, None, None, 0
        self.accept_count, self.kernel = None, None
        self.info = {}            # the call's arguments, R/mcmc.R:443-455 (get_nsteps(), get_seed(), ...)


MCMC_OUTPUT = _Output()


def get_logpost():
    """R/mcmc_info.R:351-355: vector (one chain) or list of vectors."""
    lp = MCMC_OUTPUT.logpost
    if lp is None:
        raise RuntimeError("-logpost- not found in MCMC_OUTPUT.")
    return lp[0] if len(lp) == 1 else lp


def get_draws():
    """R/mcmc_info.R:361-365: proposed states."""
    d = MCMC_OUTPUT.draws
    if d is None:
        raise RuntimeError("-draws- not found in MCMC_OUTPUT.")
    return d[0] if len(d) == 1 else d


def get_elapsed():
    return MCMC_OUTPUT.elapsed


def get_(x):
    """R/mcmc_info.R:301-315: an argument of the last MCMC() call (or logpost / draws / elapsed)."""
    if x in ("logpost", "draws", "elapsed"):
        return {"logpost": get_logpost, "draws": get_draws, "elapsed": get_elapsed}[x]()
    if x not in MCMC_OUTPUT.info:
        raise RuntimeError("-%s- not found in MCMC_OUTPUT." % x)
    return MCMC_OUTPUT.info[x]


def _getter(name):
    def g():
        return get_(name)
    g.__name__ = "get_" + name
    g.__doc__ = "R/mcmc_info.R:317-400: `%s` of the last MCMC() call." % name
    return g


get_initial, get_fun, get_nsteps, get_seed, get_nchains, get_burnin, get_thin, get_kernel, get_multicore, \
    get_conv_checker, get_cl, get_progress, get_chain_id = (_getter(n) for n in (
        "initial", "fun", "nsteps", "seed", "nchains", "burnin", "thin", "kernel", "multicore", "conv_checker", "cl",
        "progress", "chain_id"))


# ------------------------------------------------------------------------------ sharding (one process per GPU)
def shard_bounds(nchains, world, rank):
    """Contiguous chain blocks: chain c lives on rank floor(c * world / nchains)'s block."""
    return (rank * nchains) // world, ((rank + 1) * nchains) // world


def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


# ------------------------------------------------------------------------------ device-side result of one call
class DeviceChains:
    """Samples of the local chains, resident in HBM: samples [C][k][S] (+ logpost, draws).

    With `capacity` rows allocated up front (MCMC_with_conv_checker: the kept rows of all bulks, R/mcmc.R:926-947) the
    buffers are [C][k][capacity] and `nrows` of them are filled; samples / logpost / draws are views of the filled part
    (their row stride stays `capacity`, which is what fmcmc_gelman_partial_dev takes as S)."""

    def __init__(self, samples, logpost, draws, iters, thin, names, chain_base, nchains_total, nrows=None):
        self._samples, self._logpost, self._draws = samples, logpost, draws
        self.nrows = int(samples.shape[-1]) if nrows is None else int(nrows)
        self.iters, self.thin, self.names = np.asarray(iters), thin, names
        self.chain_base, self.nchains_total = chain_base, nchains_total

    samples = property(lambda self: self._samples[:, :, :self.nrows])
    logpost = property(lambda self: None if self._logpost is None else self._logpost[:, :self.nrows])
    draws = property(lambda self: None if self._draws is None else self._draws[:, :, :self.nrows])
    capacity = property(lambda self: int(self._samples.shape[-1]))

    @classmethod
    def allocate(cls, nchains_local, k, capacity, thin, names, chain_base, nchains_total, device, want_logpost=True,
                 want_draws=True):
        import torch
        f64 = dict(dtype=torch.float64, device=device)
        return cls(torch.full((nchains_local, k, capacity), float("nan"), **f64),
                   torch.empty((nchains_local, capacity), **f64) if want_logpost else None,
                   torch.empty((nchains_local, k, capacity), **f64) if want_draws else None,
                   np.zeros(0, dtype=np.int64), thin, names, chain_base, nchains_total, nrows=0)

    def extend(self, iters_of_call):
        """The rows of one more call were written behind the filled part (engine.sweep(into=...)): labels continue
        (R/append_chains.R:113-142)."""
        it = np.asarray(iters_of_call)
        if it.size:
            self.iters = it if self.iters.size == 0 else np.concatenate(
                [self.iters, it - it[0] + self.iters[-1] + self.thin])
            self.nrows += int(it.size)

    def append(self, other):
        import torch
        iters = np.concatenate([self.iters, other.iters - other.iters[0] + self.iters[-1] + self.thin])
        cat = lambda a, b: None if a is None or b is None else torch.cat([a, b], dim=-1)
        return DeviceChains(cat(self.samples, other.samples), cat(self.logpost, other.logpost),
                            cat(self.draws, other.draws), iters, self.thin, self.names, self.chain_base,
                            self.nchains_total)

    def to_host(self):
        s = self.samples.cpu().numpy()  # [C][k][S]
        start, end = (int(self.iters[0]), int(self.iters[-1])) if self.iters.size else (1, 0)
        chains = [Mcmc(s[c].T.copy(), start=start, end=end, thin=self.thin, varnames=self.names)
                  for c in range(s.shape[0])]
        return chains[0] if (len(chains) == 1 and self.nchains_total == 1) else McmcList(chains)

    # posterior summaries reduced where the rows are (fmcmc_amd/summary.py -> csrc/summary.hip); nothing is copied to the host
    def summary(self, quantiles=(0.025, 0.25, 0.5, 0.75, 0.975), cols=None):
        from .summary import summary
        return summary(self, quantiles, cols)

    def effective_size(self, cols=None):
        from .summary import effective_size
        return effective_size(self, cols)

    def geweke(self, frac1=0.1, frac2=0.5, cols=None):
        """Geweke z-scores of every chain, [C][p] (convergence_geweke stays the single-chain checker of the reference)."""
        from .summary import geweke
        return geweke(self, frac1, frac2, cols)

    def heidel(self, eps=0.1, pvalue=0.05, cols=None):
        """Heidelberger-Welch diagnostic of every chain (convergence_heildel stays the single-chain checker of the reference)."""
        from .summary import heidel
        return heidel(self, eps, pvalue, cols)

    def raftery_diag(self, q=0.025, r=0.005, s=0.95, converge_eps=0.001, cols=None):
        """Raftery-Lewis run-length diagnostic of every chain: burn-in M, total N, lower bound Nmin, dependence factor I."""
        from .summary import raftery_diag
        return raftery_diag(self, q, r, s, converge_eps, cols)

    def chain_quantiles(self, probs=(0.025, 0.25, 0.5, 0.75, 0.975), cols=None):
        """Type-7 quantiles of every chain on its own, [C][p][nprobs] (summary() pools the chains)."""
        from .summary import chain_quantiles
        return chain_quantiles(self, probs, cols)

    def gelman_diag(self, confidence=0.95, autoburnin=True, multivariate=True, cols=None):
        """Gelman-Rubin factors with coda's upper confidence limit (convergence_gelman stays the auto-stop checker)."""
        from .summary import gelman_diag
        return gelman_diag(self, confidence, autoburnin, multivariate, cols)

    def rhat(self, autoburnin=False, cols=None):
        """Rank-normalised split R-hat (Vehtari et al. 2021): bulk, tail and their maximum per column."""
        from .summary import rhat
        return rhat(self, autoburnin, cols)

    def ess(self, autoburnin=False, cols=None):
        """Rank-normalised bulk and tail effective sample size (Vehtari et al. 2021), ess_mean and mcse_mean per column."""
        from .summary import ess
        return ess(self, autoburnin, cols)

    def waic(self, model, autoburnin=False, block_rows=None):
        """WAIC of the rows under `model` (a gaussian_linreg / logistic / iid_normal object, or a pointwise_fun, whose fn gets
        blocks of at most block_rows draws): a WaicResult."""
        from .summary import waic
        return waic(self, model, autoburnin, block_rows)

    def loo(self, model, autoburnin=False, block_rows=None):
        """PSIS-LOO of the rows under `model` (as for waic()), with the Pareto k of every observation: a LooResult."""
        from .summary import loo
        return loo(self, model, autoburnin, block_rows)

    def predict(self, model, newdata=None, probs=(0.025, 0.5, 0.975), kind="epred", autoburnin=False):
        """Fitted values (newdata None) or predictions at new covariates under `model` (a gaussian_linreg / logistic object), with
        their sd and credible band per point: a PredictResult."""
        from .summary import predict
        return predict(self, model, newdata, probs, kind, autoburnin)

    def predictive(self, model, newdata=None, y=None, probs=(0.025, 0.5, 0.975), autoburnin=False, max_passes=100):
        """The posterior predictive distribution of a new observation y at every point under `model` (a gaussian_linreg object):
        its quantiles at probs (prediction intervals) and the PIT of the given y: a PredictiveResult."""
        from .summary import predictive
        return predictive(self, model, newdata, y, probs, autoburnin, max_passes)

    def loo_predictive(self, model, autoburnin=False):
        """The leave-one-out predictive mean, sd and PIT of every observation under `model` (a gaussian_linreg / logistic object)
        from the PSIS weights of loo(): a LooPredictiveResult."""
        from .summary import loo_predictive
        return loo_predictive(self, model, autoburnin)

    def ppc(self, model, seed=1, autoburnin=False):
        """The posterior predictive check of the rows under `model` (a gaussian_linreg / logistic object): per draw the mean, sd,
        min, max and chi-square discrepancy of one replicated data set, and their p-values against y: a PpcResult."""
        from .summary import ppc
        return ppc(self, model, seed, autoburnin)

    def posterior_predict(self, model, ndraws=50, seed=1, autoburnin=False):
        """The replicated data sets of ndraws evenly spaced draws under `model`, a device tensor [ndraws][n]."""
        from .summary import posterior_predict
        return posterior_predict(self, model, ndraws, seed, autoburnin)

    def rank_scores(self, fold=False, cols=None):
        """The rank-normalised scores behind rhat(), a device tensor [p][2 C][N // 2] (for rank plots)."""
        from .summary import rank_scores
        return rank_scores(self, fold, cols)

    def hpd_interval(self, prob=0.95, cols=None):
        """Highest-posterior-density interval of every chain on its own (coda::HPDinterval): lower, upper [C][p]."""
        from .summary import hpd_interval
        return hpd_interval(self, prob, cols)

    def autocorr_diag(self, lags=(0, 1, 5, 10, 50), relative=True, cols=None):
        """Autocorrelations at the given lags (coda::autocorr.diag): acf [C][nlags][p] and its mean over the chains."""
        from .summary import autocorr_diag
        return autocorr_diag(self, lags, relative, cols)

    def crosscorr(self, cols=None):
        """Correlation matrix [p][p] of the pooled rows (coda::crosscorr)."""
        from .summary import crosscorr
        return crosscorr(self, cols)


def _validate_common(nsteps, nchains, burnin, thin, multicore):
    if multicore and nchains == 1:
        raise ValueError("When `multicore = TRUE`, `nchains` should be greater than 1.")
    if nchains < 1:
        raise ValueError("`nchains` must be an integer greater than 1.")
    if burnin >= nsteps:
        raise ValueError("-burnin- (%d) cannot be >= than -nsteps- (%d)." % (burnin, nsteps))
    if thin >= nsteps:
        raise ValueError("-thin- (%d) cannot be > than -nsteps- (%d)." % (thin, nsteps))
    if thin < 1:
        raise ValueError("-thin- should be >= 1.")


def _run_call(initial_local, fun, nsteps, burnin, thin, kernel, seed, chain_base, nchains_total, names,
              device, want_logpost=True, want_draws=True, history=None, fed=None):
    """One MCMC_without_conv_checker over the local chains -> DeviceChains (history: append the rows to it instead)."""
    import torch
    gm = fun.device_model(device)
    kernel._init(initial_local.shape[1])
    user = isinstance(kernel, fmcmc_user_kernel)   # kernel_new(): the proposal is the caller's (engine.sweep_user)
    if user and fed is not None:
        raise ValueError("-fed- supplies the variates of the built-in kernels: a kernel_new() kernel draws its own.")
    if not user and (kernel._spec is None or kernel._spec.device != gm.device):
        kernel._spec = kernel.spec(gm.device)
    sweep = functools.partial(engine.sweep_user, gm, kernel) if user else functools.partial(engine.sweep, gm, kernel._spec)
    if initial_local.shape[0] == 0:
        # a rank without chains (nchains < number of ranks): nothing to launch, but it still takes part in the checker's
        # all-reduce with an empty partial
        if history is not None:
            history.extend(burnin + thin * np.arange(1, engine.kept_rows(nsteps, burnin, thin) + 1))
            return history
        k, S = initial_local.shape[1], max(engine.kept_rows(nsteps, burnin, thin), 0)
        f64 = dict(dtype=torch.float64, device=gm.device)
        dc = DeviceChains(torch.empty((0, k, S), **f64), torch.empty((0, S), **f64) if want_logpost else None,
                          torch.empty((0, k, S), **f64) if want_draws else None,
                          burnin + thin * np.arange(1, S + 1), thin, names, chain_base, nchains_total)
        dc.accept_count = torch.zeros(0, dtype=torch.int64, device=gm.device)
        return dc
    st = kernel.state_for(initial_local, gm.device)
    fkw = {}
    if fed is not None:
        # FMCMC_RNG_FED: the caller supplies the variates of this call in the order the reference draws them (per chain:
        # log(runif(nsteps)), then the kernel's draws step by step, chains one after the other: R/mcmc.R:643-673,726)
        logu, z = fed(initial_local.shape[0], nsteps, kernel._spec.kz, kernel)
        fkw = dict(fed_logu=torch.as_tensor(np.ascontiguousarray(logu, dtype=np.float64)).to(gm.device),
                   fed_z=torch.as_tensor(np.ascontiguousarray(z, dtype=np.float64)).to(gm.device))
    if history is not None:
        out = sweep(st, nsteps, burnin=burnin, thin=thin, seed=seed, chain_base=chain_base, want_bits=False,
                    into=(history._samples, history._logpost, history._draws), row0=history.nrows, **fkw)
        history.extend(out.iters)
        history.accept_count = out.accept_count
        return history
    out = sweep(st, nsteps, burnin=burnin, thin=thin, seed=seed, chain_base=chain_base,
                want_logpost=want_logpost, want_draws=want_draws, want_bits=False, **fkw)
    dc = DeviceChains(out.samples, out.logpost, out.draws, out.iters, thin, names, chain_base, nchains_total)
    dc.accept_count = out.accept_count
    return dc


def _fun_names(fun, initial, names):
    """batched_fun(names=...) names the parameters unless `initial` does (a named vector or a previous result)."""
    if isinstance(fun, BatchedFun) and fun.names and not isinstance(initial, (dict, McmcList)) and len(fun.names) == len(names):
        return list(fun.names)
    return names


def MCMC_without_conv_checker(initial, fun, nsteps, nchains=1, burnin=0, thin=1, kernel=None, multicore=False,
                              conv_checker=None, cl=None, progress=False, chain_id=1, seed=0, device=None,
                              _return_device=False, keep_logpost=True, keep_draws=True, fed=None):
    """R/mcmc.R:485-838 for all chains at once."""
    if kernel is None:
        kernel = kernel_normal()
    if not isinstance(fun, (LogPosterior, BatchedFun)):
        raise TypeError("-fun- must be one of the engine's closed-form families (gaussian_linreg, logistic, "
                        "iid_normal): an arbitrary closure cannot run inside the fused GPU kernel.")
    if not isinstance(kernel, fmcmc_kernel):
        raise TypeError("-kernel- must be an fmcmc_kernel (kernel_normal, kernel_normal_reflective, kernel_adapt, kernel_ram).")
    init, names = check_initial(initial, nchains)
    names = _fun_names(fun, initial, names)
    _validate_common(nsteps, nchains, burnin, thin, multicore)
    if init.shape[1] != fun.k:
        raise ValueError("Incorrect length of -initial-: the model has %d parameters, got %d." % (fun.k, init.shape[1]))
    dist, rank, world = _dist()
    lo, hi = shard_bounds(nchains, world, rank)
    dc = _run_call(init[lo:hi], fun, nsteps, burnin, thin, kernel, seed, lo, nchains, names, device,
                   want_logpost=keep_logpost, want_draws=keep_draws, fed=fed)
    _store_output(dc, kernel)
    return dc if _return_device else dc.to_host()


def _store_output(dc, kernel):
    lp = dc.logpost.cpu().numpy() if dc.logpost is not None else None
    dr = dc.draws.cpu().numpy() if dc.draws is not None else None
    MCMC_OUTPUT.logpost = [lp[c] for c in range(lp.shape[0])] if lp is not None else None
    MCMC_OUTPUT.draws = [dr[c].T.copy() for c in range(dr.shape[0])] if dr is not None else None
    MCMC_OUTPUT.nchains = dc.samples.shape[0]
    MCMC_OUTPUT.kernel = kernel


def bulk_plan(nsteps, burnin, freq):
    """The steps of the bulks of an auto-stop call (R/mcmc.R:868-884): nsteps - burnin in bulks of `freq` and a remainder bulk,
    one bulk of nsteps when two bulks of `freq` do not fit, `burnin` added to the first."""
    if freq * 2 > nsteps:
        freq = 0
    if freq > 0:
        bulks = [freq] * ((nsteps - burnin) // freq)
        if (nsteps - burnin) % freq:
            bulks.append((nsteps - burnin) - sum(bulks))
    else:
        bulks = [nsteps]
    bulks[0] += burnin
    return bulks


def MCMC_with_conv_checker(initial, fun, nsteps, nchains, burnin, thin, kernel, multicore, conv_checker, cl=None,
                           progress=False, chain_id=1, seed=0, device=None, _return_device=False, verbose=True,
                           keep_logpost=True, keep_draws=True, fed=None):
    """R/mcmc.R:841-1019: run in bulks of `freq`, restart every chain from its last row, stop when the
    checker says so."""
    if conv_checker is None:
        raise ValueError("The convergence checker for this call cannot be null.")
    freq = getattr(conv_checker, "freq", None)
    if freq is None:
        freq = nsteps // 2
        warnings.warn("The -conv_checker- function has no freq attribute. Default value set to be %d" % freq)
    bulks = bulk_plan(nsteps, burnin, freq)
    if kernel is None:
        kernel = kernel_normal()
    if not isinstance(fun, (LogPosterior, BatchedFun)):
        raise TypeError("-fun- must be one of the engine's closed-form families (gaussian_linreg, logistic, "
                        "iid_normal): an arbitrary closure cannot run inside the fused GPU kernel.")
    if not isinstance(kernel, fmcmc_kernel):
        raise TypeError("-kernel- must be an fmcmc_kernel (kernel_normal, kernel_normal_reflective, kernel_adapt, kernel_ram).")
    init, names = check_initial(initial, nchains)
    if isinstance(fun, BatchedFun) and init.shape[1] != fun.k:
        raise ValueError("Incorrect length of -initial-: the model has %d parameters, got %d." % (fun.k, init.shape[1]))
    names = _fun_names(fun, initial, names)
    dist, rank, world = _dist()
    lo, hi = shard_bounds(nchains, world, rank)
    init_local = init[lo:hi]
    conv_checker.flush()
    converged = False
    free = None
    # the history of all bulks, allocated once: every bulk's kept rows are written behind the previous ones by the sweep
    # itself (fmcmc_out.ld_rows) -- no per-bulk concatenation of a history that reaches GBs at config C4
    capacity = sum(engine.kept_rows(nb, burnin if bi == 0 else 0, thin) for bi, nb in enumerate(bulks))
    gdev = fun.device_model(device).device
    ans = DeviceChains.allocate(hi - lo, init.shape[1], capacity, thin, names, lo, nchains, gdev,
                                want_logpost=keep_logpost, want_draws=keep_draws)
    for bi, nb in enumerate(bulks):
        if bi > 0:
            burnin = 0
            # initial <- ans[niter(ans), ]: the last KEPT row of every chain (R/mcmc.R:908-911), which with thin > 1 is not
            # the last row the loop visited
            # (a first bulk can end without a kept row -- burnin > 0 and freq < thin < freq + burnin pass the argument checks --
            #  where R's `ans[niter(ans), ]` has no row to take; the chains then continue from the state the kernel carries,
            #  their true last row, instead of from the NaN prefill of the history)
            init_local = ans._samples[:, :, ans.nrows - 1] if ans.nrows > 0 else kernel._state.theta0
        _validate_common(nb, nchains, burnin, thin, multicore)
        _run_call(init_local, fun, nb, burnin, thin, kernel, seed, lo, nchains, names, device, history=ans, fed=fed)
        if free is None:
            free = np.nonzero(~kernel.fixed)[0]
        converged = conv_checker.check_device(ans, free)
        msg = conv_checker.msg
        total = sum(bulks[:bi + 1])
        if converged:
            if verbose and rank == 0:
                print("Convergence has been reached with %d steps. %s(%d final count of samples)."
                      % (total, (msg + " ") if msg else "", ans.samples.shape[-1]))
            break
        elif verbose and rank == 0:
            print("No convergence yet (steps count: %d). %sTrying with the next bulk." % (total, (msg + " ") if msg else ""))
    if not converged and verbose and rank == 0:
        print("No convergence reached after %d steps (%d final count of samples)." % (sum(bulks[:bi + 1]), ans.samples.shape[-1]))
    ans.converged = converged
    _store_output(ans, kernel)
    return ans if _return_device else ans.to_host()


_seed_counter = [int(time.time_ns()) & 0xFFFFFFFF]


def MCMC(initial, fun, nsteps, *, seed=None, nchains=1, burnin=0, thin=1, kernel=None, multicore=False,
         conv_checker=None, cl=None, progress=False, chain_id=1, device=None, _return_device=False,
         keep_logpost=True, keep_draws=True, fed=None):
    """Drop-in for fmcmc::MCMC (R/mcmc.R:325-340).

    initial: vector, [nchains x k] matrix, or a previous result (Mcmc: its last `nchains` rows,
    R/mcmc.R:344-378; McmcList: each chain's last row, :382-422).  fun: gaussian_linreg / logistic /
    iid_normal object, or batched_fun(fn, k) for any other model.  seed: Philox key (None: a fresh one per call; with torch.distributed every rank uses rank 0's).
    keep_logpost / keep_draws = False: do not record MCMC_OUTPUT's logpost / draws (R always does, R/mcmc.R:822-823; at
    config C4 the draws alone are 2 GB per GPU).  fed: callable (nchains, nsteps, kz, kernel) -> (logu [C][nsteps],
    z [C][nsteps][kz]) supplying the variates of every call instead of the Philox stream (fmcmc_run.rng_mode = FED; one
    process only): fed R's own Mersenne-Twister stream the engine retraces fmcmc's printed outputs."""
    MCMC_OUTPUT.clear()
    t0 = time.time()
    if isinstance(initial, Mcmc):
        initial = initial.tail(nchains - 1)
        if initial.shape[0] == 1:
            initial = initial[0]
    elif isinstance(initial, McmcList):
        if nchains != len(initial):
            raise ValueError("The parameter `nchains` must equal the number of chains passed by `initial`.")
    if seed is None:
        _seed_counter[0] = (_seed_counter[0] * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        seed = _seed_counter[0] & 0x7FFFFFFFFFFFFFFF
        dist, rank, world = _dist()
        if dist is not None:
            # the RNG is keyed by (seed, GLOBAL chain id): every rank must use the same key or sharding would change the chains
            import torch
            dev = fun.device_model(device).device if isinstance(fun, (LogPosterior, BatchedFun)) else "cpu"
            t = torch.tensor([seed], dtype=torch.int64, device=dev)
            dist.broadcast(t, src=0)
            seed = int(t.item())
    if kernel is None:
        kernel = kernel_normal()
    MCMC_OUTPUT.info = dict(initial=initial, fun=fun, nsteps=nsteps, seed=seed, nchains=nchains, burnin=burnin, thin=thin,
                            kernel=kernel, multicore=multicore, conv_checker=conv_checker, cl=cl, progress=progress,
                            chain_id=chain_id)
    if conv_checker is not None:
        ans = MCMC_with_conv_checker(initial, fun, nsteps, nchains, burnin, thin, kernel, multicore, conv_checker,
                                     cl, progress, chain_id, seed=seed, device=device, _return_device=_return_device,
                                     keep_logpost=keep_logpost, keep_draws=keep_draws, fed=fed)
    else:
        ans = MCMC_without_conv_checker(initial, fun, nsteps, nchains, burnin, thin, kernel, multicore, None, cl,
                                        progress, chain_id, seed=seed, device=device, _return_device=_return_device,
                                        keep_logpost=keep_logpost, keep_draws=keep_draws, fed=fed)
    MCMC_OUTPUT.elapsed = time.time() - t0
    return ans


# ------------------------------------------------------------------------------ one model on many datasets
class McmcBatch:
    """The result of MCMC_batch(): D datasets x nchains chains, resident in HBM.  len(ans) == D; ans[d] is the DeviceChains
    of dataset d's chains (slices of the call's buffers, no copies: gelman_diag(ans[d]), summary(ans[d]), ... work per
    dataset); ans.chains holds all D x nchains chains, dataset by dataset, for the per-chain diagnostics in one launch;
    ans.to_host() is a list of D McmcList; ans.gelman_diag() is gelman_diag(ans[d]) of every dataset from one reduction.

    After MCMC_batch(stop_each = ...) the datasets stopped at different bulks and the result is ragged:
      converged [D] bool      did the dataset pass the test
      steps [D]               the steps it ran
      nrows [D]               the rows it kept; its rows beyond them are NaN
      rhat_history            a list of (steps so far, values [D]): the statistic of every check, NaN where a dataset was
                              not tested (frozen before, or a check that could not be computed)
    ans[d], last_rows() and to_host() use each dataset's own rows and iteration labels; ans.chains covers the rows EVERY
    dataset has (min(nrows)), so the per-chain diagnostics stay finite on it; ans.history holds all rows.  Without
    stop_each: converged is None, steps and nrows are the call's for every dataset, rhat_history is empty."""

    def __init__(self, chains, nmodels, nchains, nrows=None, steps=None, converged=None, rhat_history=None):
        self.nmodels, self.nchains = int(nmodels), int(nchains)
        self.history = chains                # every row of the call
        self.nrows = np.full(self.nmodels, chains.nrows, dtype=np.int64) if nrows is None else np.asarray(nrows, dtype=np.int64)
        if self.nrows.shape != (self.nmodels,) or (self.nrows < 0).any() or (self.nrows.size and self.nrows.max() > chains.nrows):
            raise ValueError("`nrows` must give every dataset's rows, at most the %d of the buffers" % chains.nrows)
        self.steps = None if steps is None else np.asarray(steps, dtype=np.int64)
        self.converged = None if converged is None else np.asarray(converged, dtype=bool)
        self.rhat_history = list(rhat_history or [])
        common = int(self.nrows.min()) if self.nrows.size else chains.nrows
        if common == chains.nrows:
            self.chains = chains
        else:                                # the rows every dataset has
            self.chains = DeviceChains(chains._samples, chains._logpost, chains._draws, chains.iters[:common], chains.thin,
                                       chains.names, chains.chain_base, chains.nchains_total, nrows=common)
            if hasattr(chains, "accept_count"):
                self.chains.accept_count = chains.accept_count

    @property
    def ragged(self):
        """did the datasets stop after different numbers of steps (or keep different numbers of rows)"""
        differ = lambda v: v is not None and v.size > 0 and bool((v != v[0]).any())
        return differ(self.nrows) or differ(self.steps)

    def __len__(self):
        return self.nmodels

    def __getitem__(self, d):
        if not -self.nmodels <= d < self.nmodels:
            raise IndexError("dataset index out of range")
        d %= self.nmodels
        a, ch, nr = d * self.nchains, self.history, int(self.nrows[d])
        sl = slice(a, a + self.nchains)
        cut = lambda t: None if t is None else t[sl]
        dc = DeviceChains(cut(ch._samples), cut(ch._logpost), cut(ch._draws), ch.iters[:nr], ch.thin, ch.names, ch.chain_base + a,
                          self.nchains, nrows=nr)
        if hasattr(ch, "accept_count"):
            dc.accept_count = ch.accept_count[sl]
        return dc

    def __iter__(self):
        return (self[d] for d in range(self.nmodels))

    def last_rows(self):
        """[D x nchains][k]: the last kept row of every chain (a device tensor), each dataset's own"""
        smp = self.history._samples
        if not self.ragged:
            return smp[:, :, int(self.nrows[0]) - 1]
        import torch
        last = torch.as_tensor(np.repeat(self.nrows - 1, self.nchains)).to(smp.device)
        return smp[torch.arange(smp.shape[0], device=smp.device), :, last]

    def to_host(self):
        out = []
        for d in range(self.nmodels):
            h = self[d].to_host()
            out.append(h if isinstance(h, McmcList) else McmcList([h]))
        return out

    def gelman_diag(self, confidence=0.95, autoburnin=True, multivariate=True, cols=None):
        """gelman_diag(ans[d]) of every dataset (a list of GelmanDiag with the stacked psrf [D][p][2] and mpsrf [D]) from one
        grouped reduction on the device; on a ragged result every dataset is tested on its own rows."""
        from .summary import gelman_diag_batch
        return gelman_diag_batch(self, confidence, autoburnin, multivariate, cols)

    def summary(self, quantiles=(0.025, 0.25, 0.5, 0.75, 0.975), cols=None):
        """summary(ans[d]) of every dataset (a list of McmcSummary with the stacked statistics [D][p][4], quantiles [D][p][nprobs],
        ess [D][p] and per_chain arrays) from one grouped call on the device; on a ragged result every dataset is summarised on
        its own rows."""
        from .summary import summary_batch
        return summary_batch(self, quantiles, cols)

    def effective_size(self, cols=None):
        """effective_size(ans[d]) of every dataset, [D][p], from one grouped call on the device."""
        from .summary import effective_size_batch
        return effective_size_batch(self, cols)

    def rhat(self, autoburnin=False, cols=None):
        """rhat(ans[d]) of every dataset (a list of RhatDiag with the stacked bulk, tail, rhat and median [D][p]) from one
        grouped call on the device; on a ragged result every dataset is ranked on its own rows."""
        from .summary import rhat_batch
        return rhat_batch(self, autoburnin, cols)

    def ess(self, autoburnin=False, cols=None):
        """ess(ans[d]) of every dataset (a list of EssDiag with the stacked bulk, tail, mean, mcse_mean, ... [D][p] and lags
        [D][p][4]) from one grouped call on the device; on a ragged result every dataset has its own rows."""
        from .summary import ess_batch
        return ess_batch(self, autoburnin, cols)

    def waic(self, models, autoburnin=False):
        """waic(ans[d], models[d]) of every dataset (a list of WaicResult with the stacked elpd_waic, p_waic, ... [D] and
        pointwise [D][n][4]) from one grouped call on the device; on a ragged result every dataset has its own rows."""
        from .summary import waic_batch
        return waic_batch(self, models, autoburnin)

    def loo(self, models, autoburnin=False):
        """loo(ans[d], models[d]) of every dataset (a list of LooResult with the stacked elpd_loo, p_loo, pareto_k, ...) from one
        grouped device call; on a ragged batch one call per distinct row count: a LooBatch."""
        from .summary import loo_batch
        return loo_batch(self, models, autoburnin)


def batch_initial(initial, nmodels, nchains):
    """`initial` of MCMC_batch() as the [D x nchains][k] matrix of the call (dataset by dataset) and the parameter names:
    [k] (every chain of every dataset), [nchains][k] (recycled over the datasets), [D][nchains][k], or a previous McmcBatch
    (each chain's last row; a device tensor then)."""
    if isinstance(initial, McmcBatch):
        if initial.nmodels != nmodels or initial.nchains != nchains:
            raise ValueError("The previous result passed by `initial` has %d datasets x %d chains; this call has %d x %d."
                             % (initial.nmodels, initial.nchains, nmodels, nchains))
        if initial.ragged:
            raise ValueError("The previous result passed by `initial` is ragged: its datasets stopped after different numbers "
                             "of steps (stop_each), so their chains stand at different places of their variate streams, and "
                             "a call has one step base (fmcmc_run.step_base) for all of its chains. Continue the datasets "
                             "that are left with a call of their own.")
        if initial.nrows.min() < 1:
            raise ValueError("The previous result passed by `initial` has no kept row to continue from.")
        return initial.last_rows(), initial.chains.names
    names = None
    if isinstance(initial, dict):
        names, initial = list(initial.keys()), list(initial.values())
    a = np.asarray(initial, dtype=np.float64)
    if a.ndim <= 1:
        a = np.atleast_1d(a)
        if a.size == 0:
            raise ValueError("The `initial` vector is of length zero.")
        a = np.tile(a, (nmodels * nchains, 1))
    elif a.ndim == 2:
        if a.shape[0] != nchains:
            raise ValueError("The number of rows of `initial` (%d) must coincide with the number of chains per dataset (%d)."
                             % (a.shape[0], nchains))
        a = np.tile(a, (nmodels, 1))
    elif a.ndim == 3:
        if a.shape[0] != nmodels or a.shape[1] != nchains:
            raise ValueError("A three-way `initial` must be [datasets][chains][parameters] = [%d][%d][k]; got %s."
                             % (nmodels, nchains, list(a.shape)))
        a = a.reshape(nmodels * nchains, a.shape[2])
    else:
        raise ValueError("`initial` must be a vector, a [nchains][k] matrix, a [D][nchains][k] array or a previous McmcBatch.")
    if names is None:
        names = ["par%d" % (j + 1) for j in range(a.shape[1])]
    return np.ascontiguousarray(a), names


def MCMC_batch(initial, batch, nsteps, nchains=1, burnin=0, thin=1, kernel=None, seed=None, device=None, keep_logpost=True,
               keep_draws=True, conv_checker=None, stop_each=None, verbose=False):
    """MCMC() of one model on every dataset of `batch` (models.model_batch) in ONE launch: nchains chains per dataset, the
    chains of dataset d are the global chains d nchains .. (d + 1) nchains - 1 and every one of them is bit for bit the chain
    MCMC(fun = batch[d]) runs under that id.  initial: see batch_initial; a previous McmcBatch continues every chain from its
    last row with the kernel object's carried state.  Kernels: kernel_normal(_reflective), kernel_unif(_reflective) (every
    scheme), kernel_adapt(bw = 0, freq = 1), kernel_ram, up to 64 parameters.  Returns an McmcBatch.

    stop_each = convergence_gelman(freq, threshold, check_invariant): every dataset stops on its own.  The call runs in the
    bulks of MCMC(conv_checker = ...) (bulk_plan); after each bulk ONE grouped reduction tests the datasets that still run
    (summary.enqueue_gelman_groups), the host finishes them, and a dataset whose statistic (mpsrf; psrf at one free parameter)
    is below the threshold is frozen: the next bulks skip its chains (engine.sweep_batch(active = ...)), whose state and rows
    stay as they are.  Every dataset's rows, statistics and stop bulk are those of MCMC(fun = batch[d], conv_checker = ...)
    run with its chains' global ids.  The checker object is only read (freq, threshold, check_invariant).

    stop_each = convergence_rhat(freq, threshold, autoburnin, min_ess): the same loop on the rank-normalised split R-hat, one
    chain per dataset is enough.  After each bulk ONE grouped call ranks the datasets that still run
    (summary.enqueue_rank_rhat_groups); a dataset stops when the largest max(bulk, tail) over its free columns is below the
    threshold, and with min_ess only if also its smallest effective sample size reaches it (one more grouped call, masked
    to those whose R-hat passed: summary.enqueue_rank_ess_groups).  rhat_history holds the R-hat values."""
    from .models import ModelBatch
    if conv_checker is not None:
        raise ValueError("MCMC_batch runs without a -conv_checker-: the datasets would stop at different times. Pass "
                         "stop_each = convergence_gelman(...) to stop every dataset on its own, or check gelman_diag(ans) "
                         "and continue with initial = ans.")
    if stop_each is not None:
        from .convergence import convergence_gelman, convergence_rhat
        if not isinstance(stop_each, (convergence_gelman, convergence_rhat)):
            raise TypeError("-stop_each- must be a convergence_gelman(freq, threshold, check_invariant) or a "
                            "convergence_rhat(freq, threshold, autoburnin, min_ess): the single-chain checkers have no "
                            "batched form.")
        if isinstance(stop_each, convergence_gelman) and nchains < 2:
            raise ValueError("Convergence test with the Gelman is only available when `nchains` > 1L.")
    if not isinstance(batch, ModelBatch):
        raise TypeError("-batch- must be a model_batch(...) of the engine's closed-form families.")
    if kernel is None:
        kernel = kernel_normal()
    if isinstance(kernel, fmcmc_user_kernel):
        raise ValueError("MCMC_batch runs the built-in kernels: a kernel_new() kernel calls back to the host every step.")
    if not isinstance(kernel, fmcmc_kernel):
        raise TypeError("-kernel- must be an fmcmc_kernel (kernel_normal, kernel_normal_reflective, kernel_adapt, kernel_ram).")
    if _dist()[2] > 1:
        raise ValueError("MCMC_batch runs on one rank: shard the datasets over the ranks and call it once per rank.")
    D = batch.nmodels
    _validate_common(nsteps, nchains, burnin, thin, False)
    init, names = batch_initial(initial, D, nchains)
    if init.shape[1] != batch.k:
        raise ValueError("Incorrect length of -initial-: the model has %d parameters, got %d." % (batch.k, init.shape[1]))
    if not isinstance(initial, (dict, McmcBatch)) and batch.names and len(batch.names) == len(names):
        names = list(batch.names)
    if seed is None:
        _seed_counter[0] = (_seed_counter[0] * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        seed = _seed_counter[0] & 0x7FFFFFFFFFFFFFFF
    gm = batch.device_model(device)
    kernel._init(init.shape[1])
    if kernel._spec is None or kernel._spec.device != gm.device:
        kernel._spec = kernel.spec(gm.device)
    st = kernel.state_for(init, gm.device)
    if stop_each is not None:
        return _batch_stop_each(gm, kernel, st, D, nchains, nsteps, burnin, thin, seed, names, keep_logpost, keep_draws,
                                stop_each, verbose)
    out = engine.sweep_batch(gm, kernel._spec, st, nsteps, burnin=burnin, thin=thin, seed=seed, want_logpost=keep_logpost,
                             want_draws=keep_draws, want_bits=False)
    dc = DeviceChains(out.samples, out.logpost, out.draws, out.iters, thin, names, 0, D * nchains)
    dc.accept_count = out.accept_count
    return McmcBatch(dc, D, nchains, steps=np.full(D, nsteps, dtype=np.int64))


def _batch_rhat_check(hist, D, nchains, free, active, mask, checker):
    """One check of MCMC_batch(stop_each = convergence_rhat(...)): the datasets of `active` (bool [D]; mask: the same as a
    device tensor, None = all) tested on the window of `hist` by ONE grouped call -> (values [D], passed [D]), per dataset
    what convergence_rhat.check_device makes of its chains alone.  With min_ess the effective sample sizes of the datasets whose
    R-hat passed come from ONE more grouped call masked to them (summary.enqueue_rank_ess_groups; dataset by dataset on its slice,
    summary.enqueue_rank_ess, where a group does not fit): they can only take a pass back."""
    from .convergence import _window
    from .summary import (enqueue_rank_ess, enqueue_rank_ess_groups, enqueue_rank_rhat, enqueue_rank_rhat_groups, ess_finish,
                          ess_groups_finish, rank_groups_fit, rhat_batch_verdicts, rhat_finish, rhat_groups_finish,
                          _raise_non_finite)
    row0, N = _window(hist.iters) if checker.autoburnin else (0, int(hist.nrows))
    if N < 4 or (checker.min_ess is not None and N < 8):
        return np.full(D, np.nan), np.zeros(D, dtype=bool)
    run = np.nonzero(active)[0]
    rhat = np.full((D, int(free.size)), np.nan)
    non_finite = np.zeros((D, int(free.size)))

    def slice_of(d):
        sl = slice(d * nchains, (d + 1) * nchains)
        return DeviceChains(hist._samples[sl], None, None, hist.iters, hist.thin, hist.names, d * nchains, nchains, nrows=hist.nrows)

    if rank_groups_fit(nchains, N):
        out, _scores, _work, cols = enqueue_rank_rhat_groups(hist, D, nchains, row0, N, free, mask)
        fin = rhat_groups_finish(out.cpu().numpy()[run], nchains, N // 2)
        rhat[run], non_finite[run] = fin.rhat, fin.non_finite
    else:                                            # (a group too large for the grouped call: dataset by dataset)
        outs = [enqueue_rank_rhat(slice_of(d), row0, N, free) for d in run]
        cols = free if not outs else outs[0][2]
        for d, (out, _work, _cols) in zip(run, outs):
            fin = rhat_finish(out.cpu().numpy(), nchains, N // 2)
            rhat[d], non_finite[d] = fin.rhat, fin.non_finite
    for d in run:
        try:
            _raise_non_finite(non_finite[d][None, :], cols, "rank")
        except ValueError as e:
            raise ValueError("dataset %d: %s" % (d, e)) from None
    vals, passed = rhat_batch_verdicts(rhat, checker.threshold, active)
    if checker.min_ess is not None:
        cand = np.nonzero(passed)[0]
        if cand.size and rank_groups_fit(nchains, N):    # one grouped call, masked to the datasets whose R-hat passed
            import torch
            emask = np.zeros(D, dtype=np.int32)
            emask[cand] = 1
            eout, _work, _cols = enqueue_rank_ess_groups(hist, D, nchains, row0, N, free, torch.as_tensor(emask).to(hist._samples.device))
            efin = ess_groups_finish(eout[torch.as_tensor(cand).to(eout.device)].cpu().numpy(), nchains, N)
            both = np.minimum(efin.bulk, efin.tail)
            passed[cand] = ~np.isnan(both).any(axis=1) & (both.min(axis=1) >= checker.min_ess)
        else:
            eouts = [enqueue_rank_ess(slice_of(d), row0, N, free)[0] for d in cand]     # all enqueued before the first copy waits
            for d, eout in zip(cand, eouts):
                efin = ess_finish(eout.cpu().numpy(), nchains, N)
                both = np.minimum(efin.bulk, efin.tail)
                passed[d] = bool(not np.isnan(both).any() and both.min() >= checker.min_ess)
    return vals, passed


def _batch_stop_each(gm, kernel, st, D, nchains, nsteps, burnin, thin, seed, names, keep_logpost, keep_draws, checker, verbose):
    """The auto-stop loop of MCMC_batch(stop_each = ...): MCMC_with_conv_checker's loop with a verdict per dataset."""
    import torch
    from .convergence import _window, convergence_gelman, convergence_rhat
    from .summary import enqueue_gelman_groups
    dev, Cn, k = gm.device, D * nchains, int(st.theta0.shape[1])
    bulks = bulk_plan(nsteps, burnin, checker.freq)
    capacity = sum(engine.kept_rows(nb, burnin if bi == 0 else 0, thin) for bi, nb in enumerate(bulks))
    # the history of all bulks, allocated once and NaN everywhere: the rows a frozen dataset never writes stay NaN
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    hist = DeviceChains(nan(Cn, k, capacity), nan(Cn, capacity) if keep_logpost else None,
                        nan(Cn, k, capacity) if keep_draws else None, np.zeros(0, dtype=np.int64), thin, names, 0, Cn, nrows=0)
    hist.accept_count = torch.zeros(Cn, dtype=torch.int64, device=dev)
    by_rank = isinstance(checker, convergence_rhat)
    # (the caller's object is only read)
    own = None if by_rank else convergence_gelman(checker.freq, checker.threshold, checker.check_invariant)
    free = np.nonzero(~kernel.fixed)[0]
    p = int(free.size)
    active = np.ones(D, dtype=bool)
    nrows, steps, converged = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64), np.zeros(D, dtype=bool)
    rhat = []
    for bi, nb in enumerate(bulks):
        mask = None if active.all() else torch.as_tensor(active.astype(np.int32)).to(dev)
        if bi > 0:
            burnin = 0
            if hist.nrows > 0:
                # the last KEPT row of every chain that goes on (MCMC_with_conv_checker); a frozen chain keeps its theta0
                last = hist._samples[:, :, hist.nrows - 1]
                if mask is None:
                    st.theta0.copy_(last)
                else:
                    st.theta0.copy_(torch.where(mask.repeat_interleave(nchains)[:, None] != 0, last, st.theta0))
        _validate_common(nb, nchains, burnin, thin, False)
        out = engine.sweep_batch(gm, kernel._spec, st, nb, burnin=burnin, thin=thin, seed=seed, want_bits=False,
                                 into=(hist._samples, hist._logpost, hist._draws), row0=hist.nrows, active=mask)
        hist.extend(out.iters)
        hist.accept_count = out.accept_count if mask is None else torch.where(mask.repeat_interleave(nchains) != 0,
                                                                              out.accept_count, hist.accept_count)
        nrows[active], steps[active] = hist.nrows, steps[active] + nb
        total = int(sum(bulks[:bi + 1]))
        vals = np.full(D, np.nan)
        if by_rank:
            vals, passed = _batch_rhat_check(hist, D, nchains, free, active, mask, checker)
            converged |= passed
        row0, N = (0, 0) if by_rank else _window(hist.iters)
        if N >= 2:
            partials, _work, _cols = enqueue_gelman_groups(hist, D, nchains, row0, N, free, mask)
            ph = partials.cpu().numpy()
            plen = ph.shape[1] - 2
            for d in np.nonzero(active)[0]:
                own.last = None
                if own._finish(ph[d], p, N, int(hist.iters[-1]), plen, nchains):
                    converged[d] = True
                if own.last is not None:
                    vals[d] = own.last
        rhat.append((total, vals))
        active &= ~converged
        if verbose:
            print("%d steps: %d of %d datasets have converged." % (total, int(converged.sum()), D))
        if not active.any():
            break
    return McmcBatch(hist, D, nchains, nrows=nrows, steps=steps, converged=converged, rhat_history=rhat)
