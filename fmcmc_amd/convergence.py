"""convergence_gelman (R/convergence.R:191-246): Gelman-Rubin auto-stop.

The reference hands the whole accumulated mcmc.list to coda::gelman.diag on every check.  Here the
samples stay in HBM: a HIP kernel reduces the window (second half of the history, coda's
autoburnin) of every local chain to its mean and covariance, a second one sums those over the local
chains in a fixed order, ONE all-reduce(sum) of 1 + 5p + 2p^2 doubles joins the GPUs (RCCL over
xGMI; the only collective of the engine), and fmcmc_gelman_finish forms W, B, psrf and mpsrf.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from .summary import gelman_partial_dev


def _window(iters):
    """coda's autoburnin: if start(x) < end(x)/2 keep iterations >= end/2 + 1."""
    iters = np.asarray(iters)
    if iters.size == 0:          # a bulk that kept no row (burnin / thin): nothing to test yet
        return 0, 0
    start, end = iters[0], iters[-1]
    if start < end / 2:
        row0 = int(np.searchsorted(iters, end / 2 + 1, side="left"))
    else:
        row0 = 0
    return row0, int(iters.size - row0)


class convergence_gelman:
    def __init__(self, freq=1000, threshold=1.10, check_invariant=True):
        self.freq, self.threshold, self.check_invariant = int(freq), float(threshold), bool(check_invariant)
        self.flush()

    def flush(self):
        """convergence_data_flush (R/convergence.R:119-165): LAST_CONV_CHECK store."""
        self.history = []  # (end iteration, value, psrf)
        self.msg = ""
        self.last = None

    # -------- device path used by MCMC_with_conv_checker
    def check_device(self, chains, cols, group=None):
        """chains: DeviceChains of the LOCAL chains. Returns the same logical on every rank."""
        import torch
        import torch.distributed as dist
        L = abi.lib()
        samples = chains.samples             # view of the filled rows; the buffer's row stride is its capacity
        Cn, k, S = samples.shape
        dev = samples.device
        p = int(len(cols))
        distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
        total_chains = chains.nchains_total if distributed else Cn
        self.msg = ""
        if total_chains < 2:
            raise ValueError("Convergence test with the Gelman is only available when `nchains` > 1L.")
        row0, N = _window(chains.iters)
        if N < 2:
            return False
        cols_d = torch.as_tensor(np.asarray(cols, dtype=np.int32)).to(dev)
        plen = int(L.fmcmc_gelman_partial_len(p))
        partial = torch.zeros(plen + 2, dtype=torch.float64, device=dev)
        # centre = first kept row of global chain 0 (broadcast through the same all-reduce pattern)
        center = torch.zeros(p, dtype=torch.float64, device=dev)
        if chains.chain_base == 0 and Cn > 0:
            center.copy_(samples[0, cols_d.long(), row0])
        if distributed:
            dist.all_reduce(center, op=dist.ReduceOp.SUM, group=group)
        if Cn > 0:
            work = torch.empty(int(L.fmcmc_gelman_work_len(Cn, p)), dtype=torch.float64, device=dev)
            gelman_partial_dev(samples, Cn, k, chains.capacity, row0, N, cols_d, center, work, partial)
            if self.check_invariant:  # rm_invariant: sd of ALL entries (R/convergence.R:171-173)
                # sum and sum of squares of the whole window from the per-chain means / variances the reduction just left in
                # `work` (an indexed copy of the window itself was 1 GB and ~1 ms per check at config C4)
                wk = work.view(Cn, p + p * p)
                xb = wk[:, :p] + center
                s2 = wk[:, p:].reshape(Cn, p, p).diagonal(dim1=1, dim2=2)
                partial[plen] = float(N) * xb.sum()
                partial[plen + 1] = ((N - 1.0) * s2 + float(N) * xb * xb).sum()
        if distributed:
            dist.all_reduce(partial, op=dist.ReduceOp.SUM, group=group)  # the engine's only collective
        ph = partial.cpu().numpy()
        return self._finish(ph, p, N, int(chains.iters[-1]), plen, total_chains)

    def _finish(self, ph, p, N, end_iter, plen, total_chains):
        L = abi.lib()
        if self.check_invariant:
            cnt = total_chains * p * N
            var_all = (ph[plen + 1] - ph[plen] ** 2 / cnt) / max(cnt - 1, 1)
            if var_all < 1e-10:
                return False
        psrf = np.empty(p)
        mps = C.c_double()
        part = np.ascontiguousarray(ph[:plen])
        rc = L.fmcmc_gelman_finish(part.ctypes.data_as(C.POINTER(C.c_double)), p, N,
                                   psrf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(mps))
        if rc != abi.OK:
            import warnings
            warnings.warn("At %d `gelman.diag` failed to be computed. Will skip and try with the next batch." % end_iter)
            return False
        val = mps.value if p > 1 else float(psrf[0])
        self.history.append((end_iter, val, psrf.copy()))
        self.last = val
        self.msg = "Gelman-Rubin's R: %.4f." % val
        return bool(val < self.threshold)

    # -------- R-style call on a host mcmc.list
    def __call__(self, x):
        import torch
        from .mcmc import McmcList, DeviceChains
        if not isinstance(x, McmcList) or len(x) < 2:
            raise ValueError("Convergence test with the Gelman is only available when `nchains` > 1L.")
        arr = np.ascontiguousarray(x.as_array().transpose(0, 2, 1))  # [C][k][S]
        dc = DeviceChains(torch.as_tensor(arr).cuda(), None, None, x.iters, x.thin, x[0].varnames, 0, len(x))
        return self.check_device(dc, np.arange(arr.shape[1]))


# ================================================================================================
# Single-chain checkers (R/convergence.R:248-360).  Their arithmetic lives in coda (not under the reference tree);
# restated from coda's published algorithms: spectrum0.ar = AR(p) fit by Yule-Walker / Levinson-Durbin with AIC order
# selection (stats::ar.yw), geweke.diag, heidel.diag (Cramer-von Mises statistic of the Brownian bridge, pcramer series).
# They are host-side (one chain, a few thousand numbers): the chain is copied out of HBM once per check.
# ================================================================================================
def _ar_yw(y):
    """stats::ar(y, aic = TRUE) (ar.yw.default): returns (coefficients, var.pred, order)."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    order_max = int(min(n - 1, np.floor(10 * np.log10(n))))
    x = y - y.mean()
    r = np.array([np.dot(x[:n - l], x[l:]) / n for l in range(order_max + 1)])   # acf(type = "covariance"): divisor n
    if r[0] == 0:
        raise FloatingPointError("zero-variance series")
    coefs = np.zeros((order_max + 1, order_max + 1))
    vars_ = np.empty(order_max + 1)
    vars_[0] = r[0]
    for m in range(1, order_max + 1):            # Levinson-Durbin (eureka)
        acc = r[m] - np.dot(coefs[m - 1, 1:m], r[m - 1:0:-1])
        phi = acc / vars_[m - 1]
        coefs[m, m] = phi
        coefs[m, 1:m] = coefs[m - 1, 1:m] - phi * coefs[m - 1, m - 1:0:-1]
        vars_[m] = vars_[m - 1] * (1 - phi * phi)
    aic = n * np.log(vars_) + 2 * np.arange(order_max + 1) + 2
    order = int(np.argmin(aic))
    var_pred = vars_[order] * n / (n - (order + 1))
    return coefs[order, 1:order + 1].copy(), float(var_pred), order


def spectrum0_ar(y):
    """coda::spectrum0.ar for one series: (spectral density at frequency zero, AR order)."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    z = np.arange(1, n + 1, dtype=np.float64)
    if n < 3:
        raise FloatingPointError("series too short")
    A = np.stack([np.ones(n), z], axis=1)
    res = y - A @ np.linalg.lstsq(A, y, rcond=None)[0]
    sd = np.sqrt(np.sum((res - res.mean()) ** 2) / (n - 1))
    if sd < 1.5e-8:                               # identical(all.equal(sd(residuals), 0), TRUE)
        return 0.0, 0
    ar, var_pred, order = _ar_yw(y)
    return var_pred / (1 - ar.sum()) ** 2, order


def _window_rows(iters, start=None, end=None):
    """stats::window on an mcmc object: rows whose iteration label lies in [start, end]."""
    iters = np.asarray(iters, dtype=np.float64)
    lo = 0 if start is None else int(np.searchsorted(iters, start - 1e-9, side="left"))
    hi = iters.size if end is None else int(np.searchsorted(iters, end + 1e-9, side="right"))
    return lo, hi


def geweke_diag(data, iters, frac1=0.1, frac2=0.5):
    """coda::geweke.diag: z-scores of mean(first frac1) - mean(last frac2), variances from spectrum0.ar."""
    data = np.asarray(data, dtype=np.float64)
    start, end = float(iters[0]), float(iters[-1])
    xstart = (start, np.floor(end - frac2 * (end - start)))
    xend = (np.ceil(start + frac1 * (end - start)), end)
    means, variances = [], []
    for s, e in zip(xstart, xend):
        lo, hi = _window_rows(iters, s, e)
        w = data[lo:hi]
        variances.append(np.array([spectrum0_ar(w[:, j])[0] for j in range(w.shape[1])]) / w.shape[0])
        means.append(w.mean(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (means[0] - means[1]) / np.sqrt(variances[0] + variances[1])


def _pcramer(q, eps=1e-5):
    """Distribution function of the Cramer-von Mises statistic (coda::heidel.diag's pcramer)."""
    from scipy.special import gamma, kv
    log_eps = np.log(eps)
    total = 0.0
    for k in range(4):
        zc = gamma(k + 0.5) * np.sqrt(4 * k + 1) / (gamma(k + 1) * np.pi ** 1.5 * np.sqrt(q))
        u = (4 * k + 1) ** 2 / (16 * q)
        total += 0.0 if u > -log_eps else zc * np.exp(-u) * kv(0.25, u)
    return float(total)


def heidel_diag(data, iters, eps=0.1, pvalue=0.05):
    """coda::heidel.diag: rows (stest, start, pvalue, htest, mean, halfwidth) per variable."""
    data = np.asarray(data, dtype=np.float64)
    iters = np.asarray(iters, dtype=np.float64)
    n_all = data.shape[0]
    out = np.full((data.shape[1], 6), np.nan)
    start, end = iters[0], iters[-1]
    start_vec = np.arange(start, end / 2 + 1e-9, n_all / 10.0) if n_all / 10.0 > 0 else np.array([start])
    for j in range(data.shape[1]):
        Y, it = data[:, j], iters
        lo, _ = _window_rows(it, end / 2)
        S0 = spectrum0_ar(Y[lo:])[0]
        converged, I = False, np.nan
        for st in start_vec:
            lo, _ = _window_rows(it, st)
            Y, it = Y[lo:], it[lo:]
            n = Y.size
            ybar = Y.mean()
            B = np.cumsum(Y) - ybar * np.arange(1, n + 1)
            with np.errstate(divide="ignore", invalid="ignore"):
                I = float(np.sum(B * B / (n * S0)) / n)
            converged = bool(np.isfinite(I) and _pcramer(I) < 1 - pvalue)
            if converged:
                break
        S0ci = spectrum0_ar(Y)[0]
        halfwidth = 1.96 * np.sqrt(S0ci / n)
        passed = bool(np.isfinite(halfwidth) and abs(halfwidth / ybar) <= eps)
        if (not converged) or (not np.isfinite(I)) or (not np.isfinite(halfwidth)):
            out[j] = [float(converged), np.nan, 1 - _pcramer(I) if np.isfinite(I) else np.nan, np.nan, np.nan, np.nan]
        else:
            out[j] = [1.0, it[0], 1 - _pcramer(I), float(passed), ybar, halfwidth]
    return out


def raftery_threshold(data, q):
    """u [p]: R's type-7 quantile at q of every column of data [n][p] on its own (the arithmetic of summary.type7_quantiles)."""
    from .summary import type7_order_ranks, type7_quantiles
    data = np.asarray(data, dtype=np.float64)
    n = data.shape[0]
    order = np.sort(data, axis=0)[type7_order_ranks(n, [q])[0]]            # [2][p] = x_(lo), x_(hi)
    return type7_quantiles(order.T[:, None, :], n, [q])[:, 0]


def raftery_counts(Z, j0, nj):
    """The integers raftery.diag needs of an indicator Z [n][p] (0 / 1) for the thinnings j = j0 .. j0 + nj - 1: the rows
    0, j, 2 j, ... (m of them) give tri [p][nj][8], the counts of the consecutive triples (a, b, c) at 4 a + 2 b + c (all 0 when
    m < 3), and last_pair [p][nj][2] = (Z_{m-2}, Z_{m-1}) of the thinned series (Z_{m-2} given as 0 when m == 1)."""
    Z = np.asarray(Z, dtype=np.int64)
    p = Z.shape[1]
    tri, last = np.zeros((p, nj, 8), dtype=np.int64), np.zeros((p, nj, 2), dtype=np.int64)
    for a, j in enumerate(range(j0, j0 + nj)):
        z = Z[::j]
        m = z.shape[0]
        for col in range(p):
            if m >= 3:
                tri[col, a] = np.bincount(4 * z[:-2, col] + 2 * z[1:-1, col] + z[2:, col], minlength=8)
            last[col, a] = (z[m - 2, col] if m >= 2 else 0, z[m - 1, col])
    return tri, last


def raftery_diag(data, iters, q=0.025, r=0.005, s=0.95, converge_eps=0.001):
    """coda::raftery.diag of one chain: data [n][p] -> rows (M, N, Nmin, I) per variable, I unrounded (coda prints signif(I, 3)).
    nmin = ceiling(q (1 - q) qnorm((1 + s) / 2)^2 / r^2); with fewer rows every entry but Nmin is NaN (coda: c("Error", nmin)).
    Per variable: u = the type-7 quantile of the series at q, Z = (x <= u); for kthin = thin, 2 thin, ... the series is thinned
    to the rows 0, j, 2 j, ..., the 2x2x2 table of its consecutive triples gives G2 against the second-order fit and
    BIC = G2 - 2 log(m - 2); at the first kthin with BIC < 0 the 2x2 table of consecutive pairs gives alpha and beta, and
    M, N = M + nkeep and I = N / nmin follow (summary.raftery_finish, shared with the device path).  A constant series (an empty
    row of the pair table) and a search that runs out of rows (m < 3) give NaN except Nmin."""
    from types import SimpleNamespace
    from .summary import raftery_bound, raftery_search, raftery_table
    data = np.asarray(data, dtype=np.float64)
    iters = np.asarray(iters)
    if data.ndim != 2 or data.shape[0] != iters.size:
        raise ValueError("raftery_diag: data [n][p] and the n iteration labels are needed")
    n, p = data.shape
    bad = ~np.isfinite(data)
    if bad.any():
        raise ValueError("%d non-finite value(s) among the rows to test (columns %s)"
                         % (int(bad.sum()), [j for j in range(p) if bad[:, j].any()]))
    _, nmin = raftery_bound(q, r, s)
    if nmin > n:
        return raftery_table(SimpleNamespace(nmin=nmin), (p,))
    thin = int(iters[1] - iters[0]) if n > 1 else 1
    Z = data <= raftery_threshold(data, q)[None, :]
    fin = raftery_search(lambda j0, nj: raftery_counts(Z, j0, nj), n, thin, q, r, s, converge_eps)
    return raftery_table(fin, (p,))


class _SingleChainChecker:
    """Common plumbing of the single-chain checkers: LAST_CONV_CHECK-style history, rm_invariant, device entry."""
    name = ""

    def __init__(self, freq=1000, check_invariant=True):
        self.freq, self.check_invariant = int(freq), bool(check_invariant)
        self.flush()

    def flush(self):
        self.history, self.msg, self.last = [], "", None

    def check_device(self, chains, cols, group=None):
        if chains.nchains_total > 1:
            raise ValueError(self._multi_msg)
        data = chains.samples[0].cpu().numpy().T[:, np.asarray(cols)]      # [S][p]
        return self._check(data, chains.iters)

    def __call__(self, x):
        from .mcmc import Mcmc, McmcList
        if isinstance(x, McmcList):
            if len(x) > 1:
                raise ValueError(self._multi_msg)
            x = x[0]
        if not isinstance(x, Mcmc):
            raise TypeError("expected an Mcmc object")
        return self._check(x.data, x.iters)

    def _prepare(self, data):
        data = np.asarray(data, dtype=np.float64)
        if self.check_invariant and data.size > 1 and np.std(data, ddof=1) < 1e-10:    # rm_invariant, R/convergence.R:169-186
            return None
        return data


class convergence_geweke(_SingleChainChecker):
    """R/convergence.R:248-292.  As in the reference, the quantity compared with `threshold` is d = 1 - 2 pnorm(-|z|)
    (one minus the two-sided p-value): the check returns TRUE iff every d > threshold."""
    _multi_msg = "The `geweke` convergence check is only available with runs of a single chain."

    def __init__(self, freq=1000, threshold=0.025, check_invariant=True, frac1=0.1, frac2=0.5):
        super().__init__(freq, check_invariant)
        self.threshold, self.frac1, self.frac2 = float(threshold), frac1, frac2

    def _check(self, data, iters):
        import warnings
        from math import erfc
        data = self._prepare(data)
        try:
            if data is None:
                raise FloatingPointError("invariant chain")
            z = geweke_diag(data, iters, self.frac1, self.frac2)
        except (FloatingPointError, np.linalg.LinAlgError, ValueError, ZeroDivisionError):
            warnings.warn("At %d `geweke.diag` failed to be computed. Will skip and try with the next batch." % len(iters))
            return False
        self.history.append((int(iters[-1]), z.copy()))
        fin = z[np.isfinite(z)]
        self.last = float(fin.mean()) if fin.size else float("nan")
        self.msg = "avg Geweke's Z: %.4f." % self.last
        d = np.array([1 - erfc(abs(v) / np.sqrt(2.0)) if np.isfinite(v) else np.nan for v in z])   # 1 - 2 pnorm(-|z|)
        if np.any(~np.isfinite(d)):
            return False
        return bool(np.all(d > self.threshold))


class convergence_heildel(_SingleChainChecker):
    """R/convergence.R:295-344: converged iff the stationarity and the half-width tests pass for every parameter."""
    _multi_msg = "The -heidel- convergence check is only available with runs of a single chain."

    def __init__(self, freq=1000, check_invariant=True, eps=0.1, pvalue=0.05):
        super().__init__(freq, check_invariant)
        self.eps, self.pvalue = eps, pvalue

    def _check(self, data, iters):
        import warnings
        data = self._prepare(data)
        try:
            if data is None:
                raise FloatingPointError("invariant chain")
            d = heidel_diag(data, iters, self.eps, self.pvalue)
        except (FloatingPointError, np.linalg.LinAlgError, ValueError, ZeroDivisionError):
            warnings.warn("At %d -coda::heidel.diag- failed to be computed. Will skip and try with the next batch." % len(iters))
            return False
        self.history.append((int(iters[-1]), d.copy()))
        self.last = float(np.nanmean(d[:, 2]))
        self.msg = "Heidel's Avg. pval: %.2f" % self.last
        tests = d[:, [0, 3]]
        if np.any(~np.isfinite(tests)):
            return False
        return bool(np.all(tests == 1))


class convergence_auto:
    """R/convergence.R:346-368: Gelman-Rubin when there are several chains, Geweke otherwise."""

    def __init__(self, freq=1000):
        self.freq = int(freq)
        self._gelman, self._geweke = convergence_gelman(freq), convergence_geweke(freq)
        self._used = self._geweke

    def flush(self):
        self._gelman.flush()
        self._geweke.flush()

    def check_device(self, chains, cols, group=None):
        self._used = self._gelman if chains.nchains_total > 1 else self._geweke
        return self._used.check_device(chains, cols, group)

    def __call__(self, x):
        from .mcmc import McmcList
        self._used = self._gelman if isinstance(x, McmcList) and len(x) > 1 else self._geweke
        return self._used(x)

    history = property(lambda self: self._used.history)
    msg = property(lambda self: self._used.msg)
    last = property(lambda self: self._used.last)


# ================================================================================================
# Rank-normalised split R-hat (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021).  The definition is INTEGRATION.md §2.2;
# the device computes it in csrc/diag_rank.hpp (summary.rhat), this is its restatement on the host.
# ================================================================================================
def split_chains(data):
    """data [C][N][p] -> [2 C][N // 2][p]: split chain 2 c = the first N // 2 rows of chain c, 2 c + 1 its last N // 2 (an odd N
    drops the middle row)."""
    data = np.asarray(data, dtype=np.float64)
    Cn, N, p = data.shape
    nh = N // 2
    return np.stack([data[:, :nh], data[:, N - nh:]], axis=1).reshape(2 * Cn, nh, p)


def rank_z(values):
    """values [m][n] -> (z [m][n], 2 r [m][n]): the average ranks r among all m n values (ties by numerical equality) and
    z = qnorm((r - 0.375) / (m n + 0.25))."""
    from scipy.special import ndtri
    from scipy.stats import rankdata
    v = np.asarray(values, dtype=np.float64) + 0.0
    r = rankdata(v.ravel(), method="average").reshape(v.shape)
    return ndtri((r - 0.375) / (v.size + 0.25)), 2.0 * r


def rhat_host(data):
    """The rank-normalised split R-hat of data [C][N][p] (or an McmcList / Mcmc) on the host: a namespace of bulk, tail, rhat,
    median, each [p] (summary.rhat is the device form; the two share rhat_of_moments)."""
    from types import SimpleNamespace
    from .mcmc import Mcmc, McmcList
    from .summary import rhat_max, rhat_of_moments
    if isinstance(data, Mcmc):
        data = McmcList([data])
    if isinstance(data, McmcList):
        data = data.as_array()
    data = np.asarray(data, dtype=np.float64)
    if data.ndim != 3 or data.shape[0] < 1 or data.shape[1] < 4:
        raise ValueError("rhat_host: data [C][N][p] with N >= 4 rows are needed")
    bad = ~np.isfinite(data)
    if bad.any():
        raise ValueError("%d non-finite value(s) among the rows to rank (columns %s)"
                         % (int(bad.sum()), [j for j in range(data.shape[2]) if bad[:, :, j].any()]))
    sp = split_chains(data)
    m, nh, p = sp.shape
    bulk, tail, med = np.empty(p), np.empty(p), np.empty(p)
    for j in range(p):
        x = sp[:, :, j] + 0.0
        srt = np.sort(x.ravel())
        med[j] = (srt[m * nh // 2 - 1] + srt[m * nh // 2]) / 2.0
        for dest, v in ((bulk, x), (tail, np.abs(x - med[j]))):
            z = rank_z(v)[0].astype(np.longdouble)
            dest[j] = rhat_of_moments(z.mean(axis=1), z.var(axis=1, ddof=1), nh)
    return SimpleNamespace(bulk=bulk, tail=tail, rhat=rhat_max(bulk, tail), median=med)


def autocov_sums(y, t0, t1):
    """y [m][n] -> (S(t0) .. S(t1 - 1), the means [m]) of the definition: the biased autocovariances of
    every row summed over the rows, every product and sum in np.longdouble."""
    y = np.asarray(y, dtype=np.longdouble)
    n = y.shape[1]
    mu = y.sum(axis=1) / n
    u = y - mu[:, None]
    return np.array([(u[:, :n - t] * u[:, t:]).sum() / n for t in range(t0, t1)], dtype=np.longdouble), mu


def ess_series_host(y):
    """geyer_tau of the series y [m][n] on longdouble autocovariances, computed in the device's rounds of lags until the pair
    test is decided: (the namespace of geyer_tau, S as far as it was needed)."""
    from .summary import LagsNeeded, ess_lag_cap, geyer_tau
    m, n = np.shape(y)
    cap = ess_lag_cap(n)
    S, t1 = np.zeros(0, dtype=np.longdouble), min(256, cap)
    while True:
        more, mu = autocov_sums(y, S.size, t1)
        S = np.concatenate([S, more])
        try:
            return geyer_tau(S.astype(np.float64), m, n, mu.astype(np.float64)), S
        except LagsNeeded:
            t1 = min(max(512, 2 * t1), cap)


def ess_host(data):
    """The rank-normalised bulk and tail effective sample size of data [C][N][p] (or an McmcList / Mcmc) on the host: a
    namespace of bulk, tail_q05, tail_q95, tail, mean, mcse_mean, tau_bulk, q05, q95, pooled_sd [p], lags [p][4] and counts
    [p][2] (the pooled values that are <= q05, <= q95) (summary.ess is the device form; the two share geyer_tau).  The autocovariances are summed directly in np.longdouble."""
    from types import SimpleNamespace
    from .mcmc import Mcmc, McmcList
    from .summary import type7_order_ranks, type7_quantiles
    if isinstance(data, Mcmc):
        data = McmcList([data])
    if isinstance(data, McmcList):
        data = data.as_array()
    data = np.asarray(data, dtype=np.float64)
    if data.ndim != 3 or data.shape[0] < 1 or data.shape[1] < 8:
        raise ValueError("ess_host: data [C][N][p] with N >= 8 rows are needed")
    bad = ~np.isfinite(data)
    if bad.any():
        raise ValueError("%d non-finite value(s) among the rows to rank (columns %s)"
                         % (int(bad.sum()), [j for j in range(data.shape[2]) if bad[:, :, j].any()]))
    sp = split_chains(data)
    m, nh, p = sp.shape
    M = m * nh
    probs = [0.05, 0.95]
    ranks = type7_order_ranks(M, probs)
    ess, tau = np.full((p, 4), np.nan), np.full((p, 4), np.nan)
    lags = np.zeros((p, 4), dtype=np.int64)
    q, sd = np.empty((p, 2)), np.empty(p)
    counts = np.zeros((p, 2), dtype=np.int64)
    for j in range(p):
        x = sp[:, :, j] + 0.0
        srt = np.sort(x.ravel())
        q[j] = type7_quantiles(srt[ranks], M, probs)
        counts[j] = [(x <= q[j, 0]).sum(), (x <= q[j, 1]).sum()]
        sd[j] = float(np.sqrt(x.astype(np.longdouble).var(ddof=1)))
        series = (rank_z(x)[0], (x <= q[j, 0]).astype(np.float64), (x <= q[j, 1]).astype(np.float64), x)
        for kind, y in enumerate(series):
            g, _ = ess_series_host(y)
            lags[j, kind] = g.K
            if srt[0] != srt[-1]:                    # a constant column: NaN throughout
                ess[j, kind], tau[j, kind] = g.ess, g.tau
    with np.errstate(invalid="ignore", divide="ignore"):
        mcse = sd / np.sqrt(ess[:, 3])
    return SimpleNamespace(bulk=ess[:, 0], tail_q05=ess[:, 1], tail_q95=ess[:, 2], tail=np.minimum(ess[:, 1], ess[:, 2]),
                           mean=ess[:, 3], mcse_mean=mcse, tau_bulk=tau[:, 0], q05=q[:, 0].copy(), q95=q[:, 1].copy(),
                           pooled_sd=sd, lags=lags, counts=counts)


class convergence_rhat:
    """Auto-stop on the rank-normalised split R-hat: converged when the largest rhat = max(bulk, tail) over the free columns
    is below `threshold` (1.01 is the usual one).  With `autoburnin` the rows are coda's window (_window: the second half of
    the history, what convergence_gelman tests), else all rows.  NaN (a constant column) or fewer than 4 rows: not converged.
    With `min_ess` (400 is the usual one) a check converges only if also the smallest of the bulk and tail effective sample
    sizes (summary.ess) over the free columns reaches it; a NaN there, or fewer than 8 rows: not converged.
    One chain is enough.  The chains of ONE process only: pooled ranks across GPUs are not built.
    MCMC_batch(stop_each = convergence_rhat(...)) reads the four settings and gives every dataset this verdict from one grouped
    call per check (mcmc._batch_rhat_check, summary.rhat_batch_verdicts); the object itself is left as it was."""

    def __init__(self, freq=1000, threshold=1.01, autoburnin=True, min_ess=None):
        self.freq, self.threshold, self.autoburnin = int(freq), float(threshold), bool(autoburnin)
        self.min_ess = None if min_ess is None else float(min_ess)
        self.flush()

    def flush(self):
        self.history = []  # (end iteration, value, rhat [p]), and with min_ess: min(bulk, tail) ESS [p]
        self.msg = ""
        self.last = None

    def check_device(self, chains, cols, group=None):
        import torch.distributed as dist
        from .summary import enqueue_rank_rhat, rhat_finish, _raise_non_finite
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            raise NotImplementedError("convergence_rhat ranks the values of ONE process: under torch.distributed with more than "
                                      "one rank the chains are sharded and pooled ranks across GPUs are not implemented.")
        self.msg = ""
        row0, N = _window(chains.iters) if self.autoburnin else (0, int(chains.nrows))
        if N < 4 or (self.min_ess is not None and N < 8):
            return False
        out, _work, cols = enqueue_rank_rhat(chains, row0, N, cols)
        if self.min_ess is not None:                 # both calls are enqueued before the first copy waits for them
            from .summary import enqueue_rank_ess, ess_finish
            eout, _ework, _ = enqueue_rank_ess(chains, row0, N, cols)
        fin = rhat_finish(out.cpu().numpy(), int(chains._samples.shape[0]), N // 2)
        _raise_non_finite(fin.non_finite[None, :], cols, "rank")
        val = float("nan") if np.isnan(fin.rhat).any() else float(fin.rhat.max())
        self.last = val
        self.msg = "Rank-normalised split R-hat: %.4f." % val
        if self.min_ess is None:
            self.history.append((int(chains.iters[-1]), val, fin.rhat.copy()))
            return bool(val < self.threshold)
        efin = ess_finish(eout.cpu().numpy(), int(chains._samples.shape[0]), N)
        both = np.minimum(efin.bulk, efin.tail)
        least = float("nan") if np.isnan(both).any() else float(both.min())
        self.history.append((int(chains.iters[-1]), val, fin.rhat.copy(), both.copy()))
        self.msg += " Smallest ESS: %.1f." % least
        return bool(val < self.threshold and least >= self.min_ess)

    def __call__(self, x):
        import torch
        from .mcmc import DeviceChains, Mcmc, McmcList
        if isinstance(x, Mcmc):
            x = McmcList([x])
        if not isinstance(x, McmcList) or len(x) < 1:
            raise TypeError("expected an McmcList object")
        arr = np.ascontiguousarray(x.as_array().transpose(0, 2, 1))  # [C][k][S]
        dc = DeviceChains(torch.as_tensor(arr).cuda(), None, None, x.iters, x.thin, x[0].varnames, 0, len(x))
        return self.check_device(dc, np.arange(arr.shape[1]))
