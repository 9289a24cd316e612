"""Closed-form log-posterior families selected through MCMC()'s `fun` argument.

fmcmc calls an arbitrary R closure `fun(theta, ...)` every iteration (R/mcmc.R:683-718,754); a
fused GPU kernel cannot, so the engine ships the families the reference's own documentation uses:

  gaussian_linreg(X, y)   README.md:128-139 (guarded) / :356-361 (guard=False)
  logistic(X, y)          vignettes/workflow-with-fmcmc.Rmd:35-41 (prior -sum(beta^2)/8)
  iid_normal(D)           R/mcmc.R:141-144

Each constructor returns a LogPosterior: a tagged object carrying the data (moved to HBM once per
device) that MCMC() recognises.  Calling it, fun(theta), evaluates the same closed form in numpy for
inspection only -- MCMC() never calls it.

Any other model goes through batched_fun(fn, k): fn evaluates the log-posterior of ALL local chains at
once as a vectorised torch function on the device, called by the engine between the steps of its
kernels (include/fmcmc_amd.h, fmcmc_logpost_fn).
"""
import numpy as np

from . import _abi as abi


class LogPosterior:
    def __init__(self, family, X, y, intercept, guard, prior_div, names=None):
        self.family = family
        self.y = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
        if X is not None:
            X = np.asarray(X, dtype=np.float64)
            if X.ndim == 1:
                X = X[:, None]
            if X.shape[0] != self.y.shape[0]:
                raise ValueError("X has %d rows but y has %d" % (X.shape[0], self.y.shape[0]))
        self.X = X
        self.p = 0 if X is None else X.shape[1]
        self.intercept, self.guard, self.prior_div = bool(intercept), bool(guard), float(prior_div)
        self.names = names
        self._dev = {}

    @property
    def k(self):
        if self.family == abi.FAM_GAUSSIAN_LINREG:
            return int(self.intercept) + self.p + 1
        if self.family == abi.FAM_LOGISTIC:
            return int(self.intercept) + self.p
        return 2

    def device_model(self, device):
        from .engine import DeviceModel
        key = str(device)
        if key not in self._dev:
            self._dev[key] = DeviceModel(self.family, self.X, self.y, self.intercept, self.guard,
                                         self.prior_div, device=device)
        return self._dev[key]

    def __call__(self, theta):
        th = np.asarray(theta, dtype=np.float64)
        ic = int(self.intercept)
        with np.errstate(all="ignore"):
            if self.family == abi.FAM_LOGISTIC:
                eta = (th[0] if ic else 0.0) + (self.X @ th[ic:] if self.p else 0.0)
                s = np.where(self.y != 0, eta, -eta)
                f = float(np.sum(np.where(s < 0, s - np.log1p(np.exp(s)), -np.log1p(np.exp(-s)))))
                if self.prior_div:
                    f -= float(np.sum(th ** 2)) / self.prior_div
            else:
                if self.family == abi.FAM_IID_NORMAL:
                    mu, sigma = th[0], th[1]
                else:
                    mu = (th[0] if ic else 0.0) + (self.X @ th[ic:ic + self.p] if self.p else 0.0)
                    sigma = th[ic + self.p]
                if sigma < 0:
                    f = float("nan")
                elif sigma == 0:
                    f = float("-inf")
                else:
                    f = float(-self.y.size * (np.log(sigma) + 0.9189385332046727) -
                              0.5 * np.sum((self.y - mu) ** 2) / sigma ** 2)
        if self.guard and not np.isfinite(f):
            return float("-inf")
        return f


def gaussian_linreg(X, y, intercept=True, guard=True):
    """sum(dnorm(y - (b0 + X b), sd = sigma, log = TRUE)); theta = (b0, b_1..b_p, sigma)."""
    return LogPosterior(abi.FAM_GAUSSIAN_LINREG, X, y, intercept, guard, 0.0)


def logistic(X, y, intercept=False, prior_div=8.0, guard=False):
    """Bernoulli-logit log-likelihood with the N(0, prior_div/2) prior of the vignette.
    Pass the model matrix as the vignette does (own intercept column) or set intercept=True."""
    return LogPosterior(abi.FAM_LOGISTIC, X, y, intercept, guard, prior_div)


def iid_normal(D, guard=False):
    """sum(log(dnorm(D, mu, sigma))); theta = (mu, sigma)."""
    return LogPosterior(abi.FAM_IID_NORMAL, None, D, True, guard, 0.0)


class BatchedFun:
    """A user-defined log-posterior evaluated for all local chains at once: fn(theta) takes a float64 tensor [C_local, k] on
    the device (read-only: it is the engine's proposal buffer) and returns the float64 tensor [C_local] of log f(theta[c, ]),
    enqueued on the current torch stream.  MCMC() runs it with kernel_normal(_reflective), kernel_unif(_reflective) (every
    scheme), kernel_adapt(bw = 0, freq = 1) and kernel_ram; fn is called once for row 1, then once per loop step (bounded
    kernel_ram: twice, on the un-reflected and on the reflected proposal, R/kernel_ram.R:129-152)."""

    def __init__(self, fn, k, names=None):
        if not callable(fn):
            raise TypeError("batched_fun: -fn- must be callable.")
        k = int(k)
        if not 1 <= k <= abi.MAX_K:
            raise ValueError("batched_fun: k = %d outside [1, %d]." % (k, abi.MAX_K))
        if names is not None and len(names) != k:
            raise ValueError("batched_fun: %d names for k = %d parameters." % (len(names), k))
        self.fn, self.names = fn, (list(names) if names is not None else None)
        self._k = k

    @property
    def k(self):
        return self._k

    def device_model(self, device):
        from .engine import DeviceFun
        return DeviceFun(self, device)

    def __call__(self, theta):
        """fn on one parameter vector (inspection only), on the current device."""
        import torch
        th = torch.as_tensor(np.asarray(theta, dtype=np.float64)).reshape(1, self.k).to("cuda")
        return float(self.fn(th)[0].item())


def batched_fun(fn, k, names=None):
    """A user-defined log-posterior for MCMC(): fn(theta [C_local, k] float64 tensor on the device) -> [C_local] float64
    tensor on the same device.  names: optional parameter names (as the names of a named `initial`)."""
    return BatchedFun(fn, k, names)


class PointwiseFun:
    """A user-defined pointwise log-likelihood for waic() and loo(): fn(theta) takes the float64 tensor [B, k] of B draws on the
    device (read-only: it is the library's buffer) and returns the float64 tensor [B, n] of log p(y_i | theta_b) on the same
    device, the likelihood alone (no prior), enqueued on the current torch stream.  The draws come in blocks of rows; fn is called
    once per block."""

    def __init__(self, fn, n, k, names=None):
        if not callable(fn):
            raise TypeError("pointwise_fun: -fn- must be callable.")
        n, k = int(n), int(k)
        if not 1 <= k <= abi.MAX_K:
            raise ValueError("pointwise_fun: k = %d outside [1, %d]." % (k, abi.MAX_K))
        if n < 1:
            raise ValueError("pointwise_fun: n = %d observations; at least 1 is needed." % n)
        if names is not None and len(names) != k:
            raise ValueError("pointwise_fun: %d names for k = %d parameters." % (len(names), k))
        self.fn, self.names = fn, (list(names) if names is not None else None)
        self._n, self._k = n, k

    @property
    def k(self):
        return self._k

    @property
    def n(self):
        return self._n


def pointwise_fun(fn, n, k, names=None):
    """A user-defined model for waic() / loo(): fn(theta [B, k] float64 tensor on the device) -> [B, n] float64 tensor on the
    same device, log p(y_i | theta_b) of the n observations.  names: optional parameter names."""
    return PointwiseFun(fn, n, k, names)


class ModelBatch:
    """One closed-form family fitted to D datasets of one shape (model_batch): what MCMC_batch() samples in one launch.
    batch[d] is dataset d's LogPosterior; the data go to HBM once per device, as X [D][p][n] and y [D][n]."""

    def __init__(self, models):
        self.models = models
        m0 = models[0]
        self.family, self.p, self.n = m0.family, m0.p, int(m0.y.shape[0])
        self.intercept, self.guard, self.prior_div, self.names = m0.intercept, m0.guard, m0.prior_div, m0.names
        self._dev = {}

    nmodels = property(lambda self: len(self.models))
    k = property(lambda self: self.models[0].k)

    def __len__(self):
        return len(self.models)

    def __getitem__(self, d):
        return self.models[d]

    def device_model(self, device):
        from .engine import DeviceModelBatch
        key = str(device)
        if key not in self._dev:
            Xs = np.stack([m.X for m in self.models]) if self.p else None
            self._dev[key] = DeviceModelBatch(self.family, Xs, np.stack([m.y for m in self.models]), self.intercept,
                                              self.guard, self.prior_div, device=device)
        return self._dev[key]


def model_batch(models):
    """A batch of datasets for MCMC_batch(): `models` is a sequence of LogPosterior (gaussian_linreg / logistic / iid_normal
    objects) of one family with equal p, n, intercept, guard and prior_div."""
    models = list(models)
    if not models:
        raise ValueError("model_batch: -models- is empty.")
    for d, m in enumerate(models):
        if not isinstance(m, LogPosterior):
            raise TypeError("model_batch: models[%d] is a %s, not one of the engine's closed-form families (gaussian_linreg, "
                            "logistic, iid_normal)." % (d, type(m).__name__))
    m0 = models[0]
    shape = lambda m: (("family", m.family), ("p", m.p), ("n", int(m.y.shape[0])), ("intercept", m.intercept),
                       ("guard", m.guard), ("prior_div", m.prior_div))
    for d, m in enumerate(models[1:], 1):
        for (name, a), (_, b) in zip(shape(m0), shape(m)):
            if a != b:
                raise ValueError("model_batch: every dataset must have the same -%s-: models[0] has %r, models[%d] has %r."
                                 % (name, a, d, b))
    return ModelBatch(models)
