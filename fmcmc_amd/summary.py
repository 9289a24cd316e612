"""summary() / effective_size() / geweke() / heidel() / raftery_diag() / gelman_diag() / chain_quantiles() / hpd_interval() /
autocorr_diag() / crosscorr() of a result, computed on the device (coda::summary.mcmc(.list), coda::effectiveSize,
coda::geweke.diag, coda::heidel.diag, coda::raftery.diag, coda::gelman.diag, coda::HPDinterval, coda::autocorr.diag,
coda::crosscorr).

The first thing every example of the reference does with a result is `summary(ans)` (README.md:178-201, R/mcmc.R:212).  Here the
kept rows stay where the sweep left them: csrc/summary.hip reduces every (chain, column) series to its mean, variance and
spectral density at zero (coda::spectrum0.ar), pools them over the chains and selects the exact order statistics the
quantiles need; a few hundred numbers come back.  The host finish below is the type-7 interpolation and the standard errors.
gelman_diag() is coda's cross-chain diagnostic: csrc/gelman.hip reduces the window, gelman_diag_finish adds coda's upper limit.
rhat() / rank_scores() / ess() are the diagnostics that are not coda's: the rank-normalised split R-hat (csrc/diag_rank.hpp) and
the rank-normalised bulk and tail effective sample size that is read beside it (csrc/diag_ess.hpp).
There is no CPU fallback.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from . import _abi as abi

DEFAULT_QUANTILES = (0.025, 0.25, 0.5, 0.75, 0.975)


# ------------------------------------------------------------------------------------------------ host finish (pure numpy)
def type7_ranks(n, probs):
    """R's quantile type 7: index = 1 + (n - 1) prob; returns (index, lo, hi) with lo = floor(index), hi = ceil(index), 1-based."""
    index = 1.0 + np.float64(n - 1) * np.asarray(probs, dtype=np.float64)
    return index, np.floor(index).astype(np.int64), np.ceil(index).astype(np.int64)


def type7_quantiles(order_stats, n, probs):
    """order_stats [..., nprobs, 2] = x_(lo), x_(hi)  ->  quantiles [..., nprobs]: x_(lo), and (1 - h) x_(lo) + h x_(hi) with
    h = index - lo where index > lo and x_(hi) != x_(lo)."""
    order_stats = np.asarray(order_stats, dtype=np.float64)
    index, lo, _ = type7_ranks(n, probs)
    h = index - lo
    xlo, xhi = order_stats[..., 0], order_stats[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        mixed = (1.0 - h) * xlo + h * xhi
    return np.where((index > lo) & (xhi != xlo), mixed, xlo)


def finish_statistics(pooled_stats, nchain, niter):
    """pooled_stats [p][>= 3] = {pooled mean, pooled variance, mean spec0}  ->  [p][4] = Mean, SD, Naive SE, Time-series SE
    (coda::summary.mcmc.list: sqrt(var / (C N)) and sqrt(mean_c(spec0) / (C N)))."""
    ps = np.asarray(pooled_stats, dtype=np.float64)
    n = float(nchain) * float(niter)
    with np.errstate(invalid="ignore"):
        return np.stack([ps[:, 0], np.sqrt(ps[:, 1]), np.sqrt(ps[:, 1] / n), np.sqrt(ps[:, 2] / n)], axis=1)


def _fmt_column(values, digits=4):
    """One printed column the way R lays out a matrix column: a common number of decimals that gives every entry at least
    `digits` significant digits."""
    values = np.asarray(values, dtype=np.float64)
    dec = 0
    for v in values:
        if np.isfinite(v) and v != 0.0:
            dec = max(dec, digits - 1 - int(np.floor(np.log10(abs(float("%.*e" % (digits - 1, v)))))))
    dec = min(max(dec, 0), 15)
    return ["%.*f" % (dec, v) for v in values]


def _fmt_table(rownames, colnames, matrix, fmt=_fmt_column):
    cols = [[name] + fmt(matrix[:, j]) for j, name in enumerate(colnames)]
    widths = [max(len(s) for s in col) for col in cols]
    w0 = max([len(r) for r in rownames] + [0])
    lines = []
    for i in range(len(rownames) + 1):
        head = ("" if i == 0 else rownames[i - 1]).ljust(w0)
        lines.append(head + " " + " ".join(col[i].rjust(w) for col, w in zip(cols, widths)))
    return "\n".join(lines)


def _fmt_block(rownames, heads, cols):
    """coda's diagnostic tables: left-aligned columns under two-line headings."""
    cols = [list(h) + c for h, c in zip(heads, cols)]
    rows = ["", ""] + list(rownames)
    widths = [max(len(v) for v in col) for col in [rows] + cols]
    return "\n".join(" ".join(col[i].ljust(w) for col, w in zip([rows] + cols, widths)) for i in range(len(rows)))


def _par_names(index):
    """The names of unnamed parameters: par1, par2, ... for the 0-based `index`."""
    return ["par%d" % (j + 1) for j in index]


class McmcSummary:
    """coda's summary.mcmc object: statistics [p][4] (Mean, SD, Naive SE, Time-series SE), quantiles [p][nprobs], and
    per_chain (mean, sd, tsse, ess, order; each [nchain][p]) -- which chains mix badly is what the pooled table cannot say."""
    stat_names = ("Mean", "SD", "Naive SE", "Time-series SE")

    def __init__(self, statistics, quantiles, probs, varnames, start, end, thin, nchain, per_chain=None, ess=None):
        self.statistics = np.asarray(statistics, dtype=np.float64)
        self.quantiles = np.asarray(quantiles, dtype=np.float64)
        self.probs = tuple(float(q) for q in probs)
        self.varnames = list(varnames)
        self.start, self.end, self.thin, self.nchain = int(start), int(end), int(thin), int(nchain)
        self.per_chain = per_chain
        self.ess = ess

    niter = property(lambda self: (self.end - self.start) // self.thin + 1)
    quantile_names = property(lambda self: ["%g%%" % (100.0 * q) for q in self.probs])

    def __str__(self):
        out = ["", "Iterations = %d:%d" % (self.start, self.end), "Thinning interval = %d " % self.thin,
               "Number of chains = %d " % self.nchain, "Sample size per chain = %d " % self.niter, "",
               "1. Empirical mean and standard deviation for each variable,", "   plus standard error of the mean:", "",
               _fmt_table(self.varnames, self.stat_names, self.statistics), ""]
        if self.quantiles.size:
            out += ["2. Quantiles for each variable:", "", _fmt_table(self.varnames, self.quantile_names, self.quantiles), ""]
        return "\n".join(out)

    def __repr__(self):
        return "<McmcSummary nvar=%d nchain=%d niter=%d>" % (len(self.varnames), self.nchain, self.niter)


# ------------------------------------------------------------------------------------------------ device side
def _single_process():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("summary() / effective_size() / geweke() / heidel() reduce the chains of ONE process: under "
                                  "torch.distributed with more than one rank the chains are sharded and a sharded summary "
                                  "(all-reduced sums and histograms) is not implemented.")


def _as_device_chains(x):
    """DeviceChains as they are; an Mcmc / McmcList is uploaded first (as convergence_gelman.__call__ does)."""
    import torch
    from .mcmc import DeviceChains, Mcmc, McmcList
    if isinstance(x, DeviceChains):
        return x
    if isinstance(x, Mcmc):
        x = McmcList([x])
    if not isinstance(x, McmcList) or len(x) < 1:
        raise TypeError("expected a DeviceChains, Mcmc or McmcList object")
    arr = np.ascontiguousarray(x.as_array().transpose(0, 2, 1))   # [C][k][S]
    return DeviceChains(torch.as_tensor(arr).cuda(), None, None, x.iters, x.thin, x[0].varnames, 0, len(x))


def _columns(dc, cols):
    k = int(dc._samples.shape[1])
    cols = np.arange(k, dtype=np.int32) if cols is None else np.atleast_1d(np.asarray(cols)).astype(np.int32)
    if cols.size < 1 or cols.min() < 0 or cols.max() >= k:
        raise ValueError("`cols` must name at least one of the %d parameters (0-based)." % k)
    return cols


def _names(dc, cols):
    return [dc.names[c] for c in cols] if dc.names is not None else _par_names(cols)


def _open(dc, cols, verb):
    """What every enqueue_* starts with: the library L, the samples smp [C][k][S] that it can read, Cn, k, cap = S, their device
    dev, the columns cols, their device copy cols_d and their number p; the caller checks its own arguments next."""
    import torch
    _single_process()
    smp = dc._samples
    Cn, k, cap = (int(v) for v in smp.shape)
    if Cn < 1:
        raise ValueError("no chains to %s" % verb)
    if smp.dtype != torch.float64 or not smp.is_contiguous():
        raise ValueError("samples must be a contiguous float64 [C][k][S] tensor")
    cols = _columns(dc, cols)
    return SimpleNamespace(L=abi.lib(), smp=smp, Cn=Cn, k=k, cap=cap, dev=smp.device, cols=cols,
                           cols_d=torch.as_tensor(cols).to(smp.device), p=int(cols.size))


def _doubles(o, n):
    """n doubles (at least one) on the device of what _open returned."""
    import torch
    return torch.empty(max(int(n), 1), dtype=torch.float64, device=o.dev)


def _stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _windowed(o, entry, row0, N, *rest):
    """The one C call of an enqueue_*: entry(samples, C, k, S, row0, N, cols, p, *rest, stream) on the current torch stream."""
    import torch
    with torch.cuda.device(o.dev):
        rc = entry(o.smp.data_ptr(), o.Cn, o.k, o.cap, int(row0), int(N), o.cols_d.data_ptr(), o.p, *rest, _stream(o.dev))
    if rc != abi.OK:
        raise (NotImplementedError if rc == abi.ERR_UNSUPPORTED else ValueError if rc == abi.ERR_ARG else RuntimeError)(
            abi.last_error())


def enqueue_window(dc, row0, N, cols, probs=(), want_chains=True):
    """Enqueues one fmcmc_summary_dev call on the window [row0, row0 + N) of the kept rows of `dc` (current torch stream).
    Returns the device tensors (pooled, chain_stats or None, work) and the columns; nothing is synchronised."""
    o = _open(dc, cols, "summarise")
    if row0 < 0 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    probs_h = np.ascontiguousarray(probs, dtype=np.float64)
    work = _doubles(o, o.L.fmcmc_summary_work_len(o.Cn, o.p, len(probs)))
    pooled = _doubles(o, o.L.fmcmc_summary_pooled_len(o.p, len(probs)))
    chain_stats = _doubles(o, o.Cn * o.p * 4).view(o.Cn, o.p, 4) if want_chains else None
    _windowed(o, o.L.fmcmc_summary_dev, row0, N, probs_h.ctypes.data_as(C.POINTER(C.c_double)), len(probs), work.data_ptr(),
              chain_stats.data_ptr() if want_chains else None, pooled.data_ptr())
    return pooled, chain_stats, work, o.cols


# per series at the head of `work` (csrc/summary.hip: ACS, SLOT_*): r_0 .. r_64 (divisor N; exactly 0 above the window's largest
# AR order), the mean, the residual sd of the straight-line fit, the count of non-finite values
WORK_SERIES_LEN, WORK_MAX_ORDER, WORK_MEAN, WORK_RESID_SD, WORK_NON_FINITE = 72, 64, 65, 66, 67


def _series_work(work, nseries):
    """The [nseries][72] head of the `work` tensor of enqueue_window (series = chain * p + column), still on the device."""
    return work[:nseries * WORK_SERIES_LEN].view(nseries, WORK_SERIES_LEN)


def window_stats(dc, row0, N, cols, probs=(), want_chains=True):
    """One device summary of the window [row0, row0 + N), copied back:
    (pooled_stats [p][5], order_stats [p][nprobs][2], chain_stats [C][p][4] or None) as numpy arrays."""
    pooled, chain_stats, _work, cols = enqueue_window(dc, row0, N, cols, probs, want_chains)
    p, nprobs = int(cols.size), len(probs)
    ph = pooled.cpu().numpy()
    cs = chain_stats.cpu().numpy() if want_chains else None
    ps = ph[:5 * p].reshape(p, 5)
    os_ = ph[5 * p:].reshape(p, nprobs, 2)
    _raise_non_finite(ps[None, :, 4], cols, "summarise")
    return ps, os_, cs


def _per_chain(cs, N):
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.where(cs[:, :, 2] == 0.0, 0.0, N * cs[:, :, 1] / cs[:, :, 2])
    return SimpleNamespace(mean=cs[:, :, 0].copy(), sd=np.sqrt(cs[:, :, 1]), tsse=np.sqrt(cs[:, :, 2] / N), ess=ess,
                           spec0=cs[:, :, 2].copy(), order=cs[:, :, 3].astype(np.int64))


def summary(x, quantiles=DEFAULT_QUANTILES, cols=None):
    """coda::summary of a result: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first); an McmcBatch gives
    an McmcSummaryBatch, one McmcSummary per dataset from one grouped call (summary_batch)."""
    from .mcmc import McmcBatch
    if isinstance(x, McmcBatch):
        return summary_batch(x, quantiles, cols)
    dc = _as_device_chains(x)
    probs = tuple(float(q) for q in np.atleast_1d(np.asarray(quantiles, dtype=np.float64)))
    if len(probs) > abi.SUMMARY_MAX_PROBS:
        raise ValueError("at most %d quantiles per call" % abi.SUMMARY_MAX_PROBS)
    N, Cn = int(dc.nrows), int(dc._samples.shape[0])
    ps, os_, cs = window_stats(dc, 0, N, cols, probs)
    names = _names(dc, _columns(dc, cols))
    return McmcSummary(finish_statistics(ps, Cn, N), type7_quantiles(os_, Cn * N, probs), probs, names,
                       int(dc.iters[0]), int(dc.iters[-1]), dc.thin, Cn, per_chain=_per_chain(cs, N), ess=ps[:, 3].copy())


def effective_size(x, cols=None):
    """coda::effectiveSize: per column, the sum over the chains of N var / spec0 (0 where spec0 is 0); [D][p] for an McmcBatch,
    row d what effective_size(ans[d]) gives, from one grouped call."""
    from .mcmc import McmcBatch
    if isinstance(x, McmcBatch):
        return effective_size_batch(x, cols)
    dc = _as_device_chains(x)
    ps, _, _ = window_stats(dc, 0, int(dc.nrows), cols, (), want_chains=False)
    return ps[:, 3].copy()


def geweke(dc, frac1=0.1, frac2=0.5, cols=None):
    """coda::geweke.diag for every chain at once: z [C][p] from two window calls (the windows of convergence.geweke_diag)."""
    from .convergence import _window_rows
    dc = _as_device_chains(dc)
    iters = np.asarray(dc.iters)
    start, end = float(iters[0]), float(iters[-1])
    wins = ((start, np.ceil(start + frac1 * (end - start))), (np.floor(end - frac2 * (end - start)), end))
    means, variances = [], []
    for s, e in wins:
        lo, hi = _window_rows(iters, s, e)
        _, _, cs = window_stats(dc, lo, hi - lo, cols, ())
        means.append(cs[:, :, 0])
        variances.append(cs[:, :, 2] / (hi - lo))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (means[0] - means[1]) / np.sqrt(variances[0] + variances[1])


# ------------------------------------------------------------------------------------------------ Heidelberger-Welch
def pcramer(q, eps=1e-5):
    """convergence._pcramer (the distribution function of the Cramer-von Mises statistic, coda's four-term series) for an
    array of q."""
    from scipy.special import gamma, kv
    q = np.asarray(q, dtype=np.float64)
    log_eps = np.log(eps)
    total = np.zeros(q.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for k in range(4):
            zc = gamma(k + 0.5) * np.sqrt(4 * k + 1) / (gamma(k + 1) * np.pi ** 1.5 * np.sqrt(q))
            u = (4 * k + 1) ** 2 / (16 * q)
            total = total + np.where(u > -log_eps, 0.0, zc * np.exp(-u) * kv(0.25, u))
    return np.where(np.isnan(q), np.nan, total)


def heidel_candidates(iters):
    """The windows of convergence.heidel_diag: (the candidate labels coda's seq() yields, the first row each keeps, the row of
    label end / 2).  A candidate label need not be an iteration of the chain: the tail starts at iters[row]."""
    from .convergence import _window_rows
    iters = np.asarray(iters, dtype=np.float64)
    if iters.size < 1:
        raise ValueError("no rows to test")
    start, end = iters[0], iters[-1]
    labels = np.arange(start, end / 2 + 1e-9, iters.size / 10.0)
    if labels.size < 1:
        raise ValueError("heidel: the first iteration %g lies beyond end / 2 = %g, so there is no candidate start "
                         "(coda::heidel.diag fails here: wrong sign in 'by' argument)" % (start, end / 2))
    rows = np.array([_window_rows(iters, st)[0] for st in labels], dtype=np.int64)
    return labels, rows, _window_rows(iters, end / 2)[0]


class HeidelDiag:
    """coda::heidel.diag of every chain: stest, start, pvalue, htest, mean, halfwidth, each [C][p] (NaN where coda prints NA);
    table [C][p][6] in coda's column order, so table[c] is convergence.heidel_diag of chain c; cvm [C][p][ncand], the
    Cramer-von Mises statistic of the tail from each of `candidates` (the labels coda's seq() yields; `start` is the label of
    the first row such a tail keeps, which differs where niter / 10 is off the thinning grid)."""
    columns = ("stest", "start", "pvalue", "htest", "mean", "halfwidth")

    def __init__(self, table, cvm, candidates, varnames=None, eps=0.1, pvalue=0.05):
        self.table = np.asarray(table, dtype=np.float64)
        self.cvm = np.asarray(cvm, dtype=np.float64)
        self.candidates = np.asarray(candidates, dtype=np.float64)
        self.varnames = list(varnames) if varnames is not None else _par_names(range(self.table.shape[1]))
        self.eps, self.alpha = float(eps), float(pvalue)

    stest = property(lambda self: self.table[:, :, 0])
    start = property(lambda self: self.table[:, :, 1])
    pvalue = property(lambda self: self.table[:, :, 2])
    htest = property(lambda self: self.table[:, :, 3])
    mean = property(lambda self: self.table[:, :, 4])
    halfwidth = property(lambda self: self.table[:, :, 5])

    def __str__(self):
        word = lambda v: "NA" if np.isnan(v) else ("passed" if v else "failed")
        num = lambda v: "NA" if np.isnan(v) else "%.3g" % v
        out = []
        for c, t in enumerate(self.table):
            if len(self.table) > 1:
                out += ["[[%d]]" % (c + 1)]
            out += [" " * 35,
                    _fmt_block(self.varnames, (("Stationarity", "test"), ("start", "iteration"), ("p-value", "")),
                               ([word(v) for v in t[:, 0]], [num(v) for v in t[:, 1]], [num(v) for v in t[:, 2]])),
                    " " * 30,
                    _fmt_block(self.varnames, (("Halfwidth", "test"), ("Mean", ""), ("Halfwidth", "")),
                               ([word(v) for v in t[:, 3]], [num(v) for v in t[:, 4]], [num(v) for v in t[:, 5]])), ""]
        return "\n".join(out)

    def __repr__(self):
        return "<HeidelDiag nchain=%d nvar=%d ncand=%d>" % (self.table.shape[0], self.table.shape[1], self.candidates.size)


def heidel_finish(n, mean, spec0, Q, S0, starts, eps=0.1, pvalue=0.05, varnames=None, candidates=None):
    """The host finish of heidel(): n [ncand] rows of each candidate tail; mean, spec0, Q [ncand][C][p] of the tails (Q the sum
    of squares of the Brownian bridge); S0 [C][p], the spectral density of the window from end / 2; starts [ncand], the
    iteration label of the first row of each tail (coda's start(Y): what `start` reports); candidates: the labels asked for.
    Follows convergence.heidel_diag: the start is the first candidate whose statistic I = Q / (n^2 S0) has
    pcramer(I) < 1 - pvalue (else the last one is reported), halfwidth = 1.96 sqrt(spec0 / n) of that tail."""
    n = np.asarray(n, dtype=np.float64)[:, None, None]
    mean, spec0, Q = (np.asarray(a, dtype=np.float64) for a in (mean, spec0, Q))
    S0 = np.asarray(S0, dtype=np.float64)[None]
    ncand = Q.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        I = Q / (n * S0) / n                                            # [ncand][C][p]
        pc = pcramer(I)
        ok = np.isfinite(I) & (pc < 1 - pvalue)
        converged = ok.any(axis=0)
        pick = np.where(converged, ok.argmax(axis=0), ncand - 1)[None]   # first passing candidate, else the last examined
        take = lambda a: np.take_along_axis(np.broadcast_to(a, Q.shape), pick, axis=0)[0]
        I_s, pc_s, n_s, mean_s = take(I), take(pc), take(n), take(mean)
        halfwidth = 1.96 * np.sqrt(take(spec0) / n_s)
        passed = np.isfinite(halfwidth) & (np.abs(halfwidth / mean_s) <= eps)
    na = ~converged | ~np.isfinite(I_s) | ~np.isfinite(halfwidth)
    start = np.broadcast_to(np.asarray(starts, dtype=np.float64)[:, None, None], Q.shape)
    blank = lambda a: np.where(na, np.nan, a)
    table = np.stack([converged.astype(np.float64), blank(take(start)), np.where(np.isfinite(I_s), 1 - pc_s, np.nan),
                      blank(passed.astype(np.float64)), blank(mean_s), blank(halfwidth)], axis=-1)
    return HeidelDiag(table, np.moveaxis(I, 0, -1), starts if candidates is None else candidates, varnames, eps, pvalue)


def enqueue_heidel(dc, half_row, cand_rows, cols):
    """Enqueues one fmcmc_heidel_dev call on the kept rows of `dc` (current torch stream).  Returns the device tensors
    (out, work) and the columns; nothing is synchronised."""
    o = _open(dc, cols, "test")
    cand = np.ascontiguousarray(cand_rows, dtype=np.int64)
    work = _doubles(o, o.L.fmcmc_heidel_work_len(o.Cn, o.p, cand.size))
    out = _doubles(o, o.L.fmcmc_heidel_out_len(o.Cn, o.p, cand.size))
    _windowed(o, o.L.fmcmc_heidel_dev, 0, dc.nrows, int(half_row), cand.ctypes.data_as(C.POINTER(C.c_int64)), int(cand.size),
              work.data_ptr(), out.data_ptr())
    return out, work, o.cols


def heidel(x, eps=0.1, pvalue=0.05, cols=None):
    """coda::heidel.diag for every chain at once: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first).
    The windows are those of convergence.heidel_diag; the device reduces every one of them to its mean, spec0 and the sum of
    squares of its Brownian bridge (csrc/summary.hip), heidel_finish does the rest on a few numbers per series."""
    dc = _as_device_chains(x)
    labels, rows, half_row = heidel_candidates(dc.iters)
    N, Cn, ncand = int(dc.nrows), int(dc._samples.shape[0]), int(rows.size)
    out, work, cols = enqueue_heidel(dc, half_row, rows, cols)
    p = int(cols.size)
    _raise_non_finite(_series_work(work, Cn * p)[:, WORK_NON_FINITE].reshape(Cn, p).sum(0, keepdim=True).cpu().numpy(), cols,
                      "test")
    oh = out.cpu().numpy()
    stats = oh[:(1 + ncand) * Cn * p * 4].reshape(1 + ncand, Cn, p, 4)
    Q = oh[(1 + ncand) * Cn * p * 4:].reshape(ncand, Cn, p)
    names = _names(dc, cols) if dc.names is not None else None          # (None: HeidelDiag numbers them by position)
    return heidel_finish(N - rows, stats[1:, :, :, 0], stats[1:, :, :, 2], Q, stats[0, :, :, 2], np.asarray(dc.iters)[rows], eps,
                         pvalue, names, candidates=labels)


# ------------------------------------------------------------------------------------------------ Raftery-Lewis, per-chain quantiles
RAFTERY_BATCH = 16          # thinnings per device launch (and per step of the host restatement): j = 1 .. 16, then 17 .. 32, ...
RAFTERY_DEFAULTS = dict(q=0.025, r=0.005, s=0.95, converge_eps=0.001)


def raftery_bound(q, r, s):
    """coda::raftery.diag: (phi, nmin) = qnorm((1 + s) / 2), ceiling(q (1 - q) phi^2 / r^2): 3746 rows for the defaults."""
    from scipy.special import ndtri
    q, r, s = float(q), float(r), float(s)
    if not (0.0 < q < 1.0 and r > 0.0 and 0.0 < s < 1.0):
        raise ValueError("raftery_diag: need 0 < q < 1, r > 0 and 0 < s < 1")
    phi = float(ndtri(0.5 * (1.0 + s)))
    return phi, int(np.ceil((q * (1.0 - q) * (phi * phi)) / (r * r)))


def raftery_finish(tri, last_pair, m, thin, q=0.025, r=0.005, s=0.95, converge_eps=0.001, j=None):
    """The finish of raftery_diag(), from integer counts only, for any leading shape [...] (a series, [p], [C][p]):
    tri [...][nj][8]: per thinning j the counts T[a][b][c] (at 4 a + 2 b + c) of the consecutive triples (Z_i, Z_{i+1}, Z_{i+2}),
    i = 0 .. m - 3, of the indicator thinned to the rows 0, j, 2 j, ...; last_pair [...][nj][2] = (Z_{m-2}, Z_{m-1}) of that
    thinned series; m [nj] = ceil(n / j), its length; j [nj]: the thinnings (default 1 .. nj); thin: the spacing of the labels.
    Per thinning G2 = sum over the non-empty cells, a outermost, of T log(T / fit) 2 with fit = T_ab. T_.bc / T_.b., and
    BIC = G2 - log(m - 2) 2; the thinning taken is the first with BIC < 0.  The pairs F[a][b] of that thinning are sum_c T[a][b][c]
    plus the last pair; alpha = F01 / (F00 + F01), beta = F10 / (F10 + F11); M, N, I as coda forms them.
    Returns a namespace of [...] arrays: M, N, I, kthin (NaN where there is no result), j (0 there), alpha, beta, and the flags
    `failed` (a thinning with m < 3 was reached before any BIC < 0) and `undecided` (every thinning tried had m >= 3 and
    BIC >= 0: more are needed), then bic [...][nj] and nmin.  Equal counts give equal bits."""
    phi, nmin = raftery_bound(q, r, s)
    tri = np.asarray(tri, dtype=np.int64)
    last_pair = np.asarray(last_pair, dtype=np.int64)
    m = np.atleast_1d(np.asarray(m, dtype=np.int64))
    nj = m.size
    j = np.arange(1, nj + 1, dtype=np.int64) if j is None else np.atleast_1d(np.asarray(j, dtype=np.int64))
    if tri.shape[-2:] != (nj, 8) or last_pair.shape != tri.shape[:-1] + (2,) or j.size != nj:
        raise ValueError("raftery_finish: tri [...][nj][8], last_pair [...][nj][2], m [nj] and j [nj] are needed")
    lead = tri.shape[:-2]
    T = np.ascontiguousarray(tri, dtype=np.float64).reshape(lead + (nj, 2, 2, 2))
    with np.errstate(all="ignore"):
        ab = T[..., 0] + T[..., 1]                                   # [..][nj][a][b]
        bc = T[..., 0, :, :] + T[..., 1, :, :]                       # [..][nj][b][c]
        mid = ab[..., 0, :] + ab[..., 1, :]                          # [..][nj][b]
        fit = (ab[..., :, :, None] * bc[..., None, :, :]) / mid[..., None, :, None]
        term = T * np.log(np.ascontiguousarray(T / fit)) * 2.0
        term = np.where(T != 0.0, term, 0.0).reshape(lead + (nj, 8))
        g2 = np.zeros(lead + (nj,))
        for cell in range(8):                                        # (coda's loop order; an empty cell adds nothing)
            g2 = g2 + term[..., cell]
        valid = m >= 3
        bic = np.where(valid, g2 - np.log(np.where(valid, m - 2, 1).astype(np.float64)) * 2.0, np.nan)
        passing = valid & (bic < 0.0)
        # m falls as j grows: a thinning with m < 3 is behind every valid one
        found = passing.any(axis=-1)
        pick = passing.argmax(axis=-1)
        failed = ~found & (~valid).any()
        undecided = ~found & bool(valid.all())
        sel = pick[..., None, None]
        Tj = np.take_along_axis(tri, sel, axis=-2)[..., 0, :].reshape(lead + (2, 2, 2))
        lp = np.take_along_axis(last_pair, sel, axis=-2)[..., 0, :]
        F = Tj[..., 0] + Tj[..., 1]                                  # [..][a][b], integers
        F = F + ((lp[..., 0, None, None] == np.arange(2)[:, None]) & (lp[..., 1, None, None] == np.arange(2)[None, :]))
        F = F.astype(np.float64)
        alpha = F[..., 0, 1] / (F[..., 0, 0] + F[..., 0, 1])
        beta = F[..., 1, 0] / (F[..., 1, 0] + F[..., 1, 1])
        kthin = (j[pick] * int(thin)).astype(np.float64)
        ab_ = alpha + beta
        tempburn = np.log((converge_eps * ab_) / np.maximum(alpha, beta)) / np.log(np.abs(1.0 - alpha - beta))
        M = np.ceil(tempburn) * kthin
        tempprec = ((2.0 - alpha - beta) * alpha * beta * (phi * phi)) / ((ab_ * ab_ * ab_) * (r * r))
        nkeep = np.ceil(tempprec) * kthin
        N = M + nkeep
        I = N / nmin
    bad = ~found | ~np.isfinite(M) | ~np.isfinite(N)
    blank = lambda a: np.where(bad, np.nan, a)
    return SimpleNamespace(M=blank(M), N=blank(N), I=blank(I), kthin=np.where(found, kthin, np.nan), j=np.where(found, j[pick], 0),
                           alpha=np.where(found, alpha, np.nan), beta=np.where(found, beta, np.nan), failed=failed,
                           undecided=undecided, bic=bic, nmin=nmin)


def raftery_search(counts, n, thin, q=0.025, r=0.005, s=0.95, converge_eps=0.001):
    """The thinning search both raftery_diag()s share: counts(j0, nj) -> (tri [...][nj][8], last_pair [...][nj][2]) of the
    thinnings j0 .. j0 + nj - 1 is asked for one batch after the other while some series has no thinning with BIC < 0 yet and
    the next one still has m = ceil(n / j) >= 3 rows.  Returns raftery_finish of everything counted."""
    tris, lasts, j0 = [], [], 1
    while True:
        t, l = counts(j0, RAFTERY_BATCH)
        tris.append(np.asarray(t, dtype=np.int64))
        lasts.append(np.asarray(l, dtype=np.int64))
        j0 += RAFTERY_BATCH
        j = np.arange(1, j0, dtype=np.int64)
        fin = raftery_finish(np.concatenate(tris, axis=-2), np.concatenate(lasts, axis=-2), -(-int(n) // j), thin, q, r, s,
                             converge_eps, j=j)
        if not fin.undecided.any() or -(-int(n) // j0) < 3:       # (an undecided series fails at the next thinning: NaN already)
            return fin


def host_chain_order(series, ranks):
    """The order statistics fmcmc_chain_order_dev selects, from a sort: series [..., n], 0-based ranks -> [..., nranks]."""
    return np.sort(np.asarray(series, dtype=np.float64), axis=-1)[..., np.asarray(ranks, dtype=np.int64)]


def type7_order_ranks(n, probs):
    """The 0-based ranks [nprobs][2] of x_(lo), x_(hi) that type7_quantiles(., n, probs) needs."""
    _, lo, hi = type7_ranks(n, probs)
    return np.clip(np.stack([lo, hi], axis=-1) - 1, 0, n - 1)


def host_chain_quantiles(series, probs):
    """chain_quantiles() without the device: series [..., n] -> type-7 quantiles [..., nprobs] of every series on its own."""
    series = np.asarray(series, dtype=np.float64)
    n = series.shape[-1]
    ranks = type7_order_ranks(n, probs)
    return type7_quantiles(host_chain_order(series, ranks.ravel()).reshape(series.shape[:-1] + ranks.shape), n, probs)


class RafteryDiag:
    """coda::raftery.diag of every chain: M (burn-in), N (total), I = N / nmin (unrounded; coda prints signif(I, 3)) and kthin,
    each [C][p], NaN where coda has no number (a constant series; fewer than nmin rows: `nmin` is set all the same);
    table [C][p][4] in coda's column order (M, N, Nmin, I), so table[c] is convergence.raftery_diag of chain c;
    u [C][p]: the per-series threshold, the type-7 quantile at q; alpha, beta [C][p]: the transition rates of the indicator."""
    columns = ("M", "N", "Nmin", "I")

    def __init__(self, table, kthin, nmin, nrows, q, r, s, converge_eps, varnames=None, u=None, alpha=None, beta=None):
        self.table = np.asarray(table, dtype=np.float64)
        self.kthin = np.asarray(kthin, dtype=np.float64)
        self.nmin, self.nrows = int(nmin), int(nrows)
        self.q, self.r, self.s, self.converge_eps = float(q), float(r), float(s), float(converge_eps)
        self.varnames = list(varnames) if varnames is not None else _par_names(range(self.table.shape[1]))
        self.u, self.alpha, self.beta = u, alpha, beta

    M = property(lambda self: self.table[:, :, 0])
    N = property(lambda self: self.table[:, :, 1])
    I = property(lambda self: self.table[:, :, 3])

    def __str__(self):
        whole = lambda v: "NA" if np.isnan(v) else "%d" % v
        out = []
        for c, t in enumerate(self.table):
            if len(self.table) > 1:
                out += ["[[%d]]" % (c + 1)]
            out += ["", "Quantile (q) = %g" % self.q, "Accuracy (r) = +/- %g" % self.r, "Probability (s) = %g " % self.s, ""]
            if self.nmin > self.nrows:
                out += ["You need a sample size of at least %d with these values of q, r and s" % self.nmin, ""]
                continue
            out += [_fmt_block(self.varnames, (("Burn-in", "(M)"), ("Total", "(N)"), ("Lower bound", "(Nmin)"),
                                               ("Dependence", "factor (I)")),
                               ([whole(v) for v in t[:, 0]], [whole(v) for v in t[:, 1]], [whole(v) for v in t[:, 2]],
                                ["NA" if np.isnan(v) else "%.3g" % v for v in t[:, 3]])), ""]
        return "\n".join(out)

    def __repr__(self):
        return "<RafteryDiag nchain=%d nvar=%d nmin=%d>" % (self.table.shape[0], self.table.shape[1], self.nmin)


def raftery_table(fin, shape):
    """[...][4] = M, N, Nmin, I from raftery_finish's namespace (or all NaN but Nmin when fin is the bound alone)."""
    table = np.full(tuple(shape) + (4,), np.nan)
    table[..., 2] = fin.nmin
    if hasattr(fin, "M"):
        table[..., 0], table[..., 1], table[..., 3] = fin.M, fin.N, fin.I
    return table


def _raise_non_finite(nbad, cols, what):
    """nbad [C][p] counts of non-finite values per series: the one error every diagnostic raises for them."""
    per_col = np.asarray(nbad).sum(axis=0)
    if per_col.sum():
        raise ValueError("%d non-finite value(s) among the rows to %s (columns %s)"
                         % (int(per_col.sum()), what, [int(c) for c, b in zip(cols, per_col) if b]))


def enqueue_chain_order(dc, ranks, cols):
    """Enqueues one fmcmc_chain_order_dev call on the kept rows of `dc` (current torch stream): the values at the 0-based
    `ranks` of every (chain, column) series.  Returns the device tensors (out [C][p][nranks], non-finite counts [C][p]) and the
    columns; nothing is synchronised."""
    o = _open(dc, cols, "order")
    ranks = np.ascontiguousarray(ranks, dtype=np.int64).ravel()
    work = _doubles(o, o.L.fmcmc_chain_order_work_len(o.Cn, o.p, ranks.size))
    out = _doubles(o, o.Cn * o.p * max(int(ranks.size), 1)).view(o.Cn, o.p, -1)
    _windowed(o, o.L.fmcmc_chain_order_dev, 0, dc.nrows, ranks.ctypes.data_as(C.POINTER(C.c_int64)), int(ranks.size),
              work.data_ptr(), out.data_ptr())
    return out, work[:o.Cn * o.p].view(o.Cn, o.p), o.cols


def chain_quantiles(x, probs=DEFAULT_QUANTILES, cols=None):
    """R's type-7 quantiles of every chain on its own, [C][p][nprobs] (summary() pools the chains): x a DeviceChains (read in
    place), an Mcmc or a McmcList (uploaded first); at most 16 probs.  The order statistics are selected exactly on the device
    (csrc/raftery.hip, one workgroup per series); the interpolation is type7_quantiles."""
    dc = _as_device_chains(x)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if probs.size < 1 or probs.size > abi.SUMMARY_MAX_PROBS:
        raise ValueError("between 1 and %d probs per call" % abi.SUMMARY_MAX_PROBS)
    if not np.all((probs >= 0.0) & (probs <= 1.0)):
        raise ValueError("`probs` must lie in [0, 1]")
    n = int(dc.nrows)
    ranks = type7_order_ranks(n, probs)
    out, nbad, cols = enqueue_chain_order(dc, ranks.ravel(), cols)
    _raise_non_finite(nbad.cpu().numpy(), cols, "order")
    os_ = out.cpu().numpy()
    return type7_quantiles(os_.reshape(os_.shape[:2] + ranks.shape), n, probs)


def enqueue_raftery(dc, q, j0, nj, cols):
    """Enqueues one fmcmc_raftery_dev call on the kept rows of `dc` (current torch stream) for the thinnings j0 .. j0 + nj - 1.
    Returns the device tensors (head [C][p][4] = u, x_(lo), x_(hi), non-finite count; counts [C][p][nj][10] int64; work) and the
    columns; nothing is synchronised."""
    import torch
    o = _open(dc, cols, "test")
    work = _doubles(o, o.L.fmcmc_raftery_work_len(o.Cn, o.p, int(dc.nrows)))
    out = _doubles(o, o.L.fmcmc_raftery_out_len(o.Cn, o.p, nj))
    _windowed(o, o.L.fmcmc_raftery_dev, 0, dc.nrows, float(q), int(j0), int(nj), work.data_ptr(), out.data_ptr())
    series = o.Cn * o.p
    return (out[:series * 4].view(o.Cn, o.p, 4),
            out[series * 4:series * (4 + 10 * nj)].view(torch.int64).view(o.Cn, o.p, nj, 10), work, o.cols)


def raftery_diag(x, q=0.025, r=0.005, s=0.95, converge_eps=0.001, cols=None):
    """coda::raftery.diag for every chain at once: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first).
    The device selects every series' own type-7 quantile at q, packs the indicator x <= u and counts its triples for a batch of
    thinnings (csrc/raftery.hip); raftery_finish does the rest on those integers, the same function convergence.raftery_diag
    ends in, so the two agree bit for bit.  A second batch is launched only while some series has no thinning with BIC < 0."""
    dc = _as_device_chains(x)
    n, Cn = int(dc.nrows), int(dc._samples.shape[0])
    cols_ = _columns(dc, cols)
    names = _names(dc, cols_) if dc.names is not None else None
    _single_process()
    phi, nmin = raftery_bound(q, r, s)
    shape = (Cn, int(cols_.size))
    if nmin > n:
        return RafteryDiag(raftery_table(SimpleNamespace(nmin=nmin), shape), np.full(shape, np.nan), nmin, n, q, r, s,
                           converge_eps, names)
    heads = []

    def counts(j0, nj):
        head, cnt, _work, _ = enqueue_raftery(dc, q, j0, nj, cols)
        ch = cnt.cpu().numpy()
        if not heads:
            heads.append(head.cpu().numpy())
            _raise_non_finite(heads[0][:, :, 3], cols_, "test")
        return ch[..., :8], ch[..., 8:]

    iters = np.asarray(dc.iters)
    thin = int(iters[1] - iters[0]) if iters.size > 1 else int(dc.thin)
    fin = raftery_search(counts, n, thin, q, r, s, converge_eps)
    return RafteryDiag(raftery_table(fin, shape), fin.kthin, nmin, n, q, r, s, converge_eps, names, u=heads[0][:, :, 0].copy(),
                       alpha=fin.alpha, beta=fin.beta)


raftery = raftery_diag      # (the name the package exports it under: fmcmc_amd.raftery_diag is the host restatement)


# ------------------------------------------------------------------------------------------------ Gelman-Rubin
def _fmt_column_sig(values, digits=3):
    """One printed column the way R's print.default(digits) lays it out: the fewest decimals, common to the column, that show
    every entry to `digits` significant digits (trailing zeros that no entry needs are dropped: 1.001 and 1.004 print as 1)."""
    dec = 0
    for v in np.asarray(values, dtype=np.float64).ravel():
        if np.isfinite(v) and v != 0.0:
            mant, exp = ("%.*e" % (digits - 1, v)).split("e")
            nsig = len(mant.replace("-", "").replace(".", "").rstrip("0")) or 1
            dec = max(dec, nsig - 1 - int(exp))
    dec = min(max(dec, 0), 15)
    return ["NA" if np.isnan(v) else "%.*f" % (dec, v) for v in np.asarray(values, dtype=np.float64).ravel()]


class GelmanDiag:
    """coda's gelman.diag object: psrf [p][2] ("Point est.", "Upper C.I."), mpsrf (None when it was not asked for or p == 1),
    the window [start, end] of iteration labels the factors were computed on, and the confidence of the upper limit."""
    columns = ("Point est.", "Upper C.I.")

    def __init__(self, psrf, mpsrf, varnames=None, start=None, end=None, confidence=0.95):
        self.psrf = np.asarray(psrf, dtype=np.float64).reshape(-1, 2)
        self.mpsrf = None if mpsrf is None else float(mpsrf)
        self.varnames = list(varnames) if varnames is not None else _par_names(range(self.psrf.shape[0]))
        self.start, self.end, self.confidence = start, end, float(confidence)

    def __str__(self):
        out = ["Potential scale reduction factors:", "", _fmt_table(self.varnames, self.columns, self.psrf, _fmt_column_sig)]
        if self.mpsrf is not None:
            out += ["", "Multivariate psrf", "", _fmt_column_sig([self.mpsrf])[0]]
        return "\n".join(out) + "\n"

    def __repr__(self):
        return "<GelmanDiag nvar=%d mpsrf=%s>" % (self.psrf.shape[0], "None" if self.mpsrf is None else "%.4g" % self.mpsrf)


_GELMAN_FEW_CHAINS = "Convergence test with the Gelman is only available when `nchains` > 1L."


def gelman_diag_finish(partial, p, N, confidence=0.95, multivariate=True, varnames=None, start=None, end=None):
    """The host finish of gelman_diag(): a pure function of the (summed) partial vector of fmcmc_gelman_partial_dev
    (include/fmcmc_amd.h; partial[0] = number of chains m), p, the window length N and `confidence`.
    The point estimates and mpsrf are fmcmc_gelman_finish's.  The upper limit is coda::gelman.diag's, from the terms that
    function forms (w, b, var.w, df.adj):
        sqrt(df.adj ((N - 1) / N + qf((1 + confidence) / 2, m - 1, 2 w^2 / var.w) (1 + 1 / m) b / (N w)));
    where var.w is 0 (every chain has the same variance) the quantile is that of R at an infinite denominator df,
    qchisq(., m - 1) / (m - 1)."""
    from scipy import stats
    P = np.ascontiguousarray(partial, dtype=np.float64)
    p, N = int(p), int(N)
    if P.size < 1 + 5 * p + 2 * p * p or p < 1 or N < 2:
        raise ValueError("gelman_diag: a partial of 1 + 5p + 2p^2 numbers, p >= 1 and N >= 2 rows are needed")
    m = float(P[0])
    if m < 2:
        raise ValueError(_GELMAN_FEW_CHAINS)
    if not 0.0 < confidence < 1.0:
        raise ValueError("`confidence` must lie in (0, 1).")
    L = abi.lib()
    point = np.empty(p)
    mps = C.c_double()
    dp = C.POINTER(C.c_double)
    rc = L.fmcmc_gelman_finish(P.ctypes.data_as(dp), p, N, point.ctypes.data_as(dp), C.byref(mps))
    if rc == abi.ERR_CHAIN and not (multivariate and p > 1):
        rc = abi.OK              # (the point estimates are complete before the Cholesky factor of W is tried)
    if rc == abi.ERR_CHAIN:
        raise ValueError("cannot compute: W is not positive definite")
    if rc != abi.OK:
        raise RuntimeError("fmcmc_gelman_finish failed (%d)" % rc)
    o = 1
    sx = P[o:o + p]; o += p
    sxx = P[o:o + p * p].reshape(p, p).diagonal(); o += 2 * p * p
    sS = P[o - p * p:o].reshape(p, p).diagonal()
    s_s2, s_s2s2, s_s2x, s_s2xx = (P[o + i * p:o + (i + 1) * p] for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = sx / m
        w = sS / m
        b = N * (sxx - m * mu * mu) / (m - 1)
        ms2 = s_s2 / m
        var_s2 = (s_s2s2 - m * ms2 * ms2) / (m - 1)
        cov_s2_x2 = (s_s2xx - m * ms2 * (sxx / m)) / (m - 1)
        cov_s2_x = (s_s2x - m * ms2 * mu) / (m - 1)
        var_w = var_s2 / m
        var_b = 2 * b * b / (m - 1)
        cov_wb = (N / m) * (cov_s2_x2 - 2 * mu * cov_s2_x)
        V = (N - 1) * w / N + (1 + 1 / m) * b / N
        var_V = ((N - 1.0) ** 2 * var_w + (1 + 1 / m) ** 2 * var_b + 2.0 * (N - 1) * (1 + 1 / m) * cov_wb) / (float(N) * N)
        df_V = 2 * V * V / var_V
        df_adj = (df_V + 3) / (df_V + 1)
        q = (1.0 + confidence) / 2.0
        flat = var_w == 0.0
        qf = np.where(flat, stats.chi2.ppf(q, m - 1) / (m - 1),
                      stats.f.ppf(q, m - 1, np.where(flat, 1.0, 2 * w * w / np.where(flat, 1.0, var_w))))
        upper = np.sqrt(df_adj * ((N - 1.0) / N + qf * (1 + 1 / m) * b / (N * w)))
    mpsrf = mps.value if (multivariate and p > 1) else None
    return GelmanDiag(np.stack([point, upper], axis=1), mpsrf, varnames, start, end, confidence)


def gelman_partial_dev(base, Cn, k, stride, row0, N, cols_d, center, work, partial):
    """The one call site of fmcmc_gelman_partial_dev (current torch stream): the window [row0, row0 + N) of Cn chains of k columns
    that start at the tensor `base` with `stride` rows per column, reduced over the device columns `cols_d` around `center` into
    `work` and the head of `partial`.  Nothing is synchronised."""
    import torch
    with torch.cuda.device(base.device):
        rc = abi.lib().fmcmc_gelman_partial_dev(base.data_ptr(), int(Cn), int(k), int(stride), int(row0), int(N), cols_d.data_ptr(),
                                                int(cols_d.numel()), center.data_ptr(), work.data_ptr(), partial.data_ptr(),
                                                _stream(base.device))
    if rc != abi.OK:
        raise RuntimeError("fmcmc_gelman_partial_dev failed (%d)" % rc)


def enqueue_gelman(dc, row0, N, cols):
    """Enqueues one fmcmc_gelman_partial_dev call on the window [row0, row0 + N) of the kept rows of `dc` (current torch
    stream), centred on the window's first row of chain 0.  Returns the device tensors (partial, work) and the columns."""
    o = _open(dc, cols, "compare")
    if row0 < 0 or N < 2 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) needs at least two of the %d kept rows" % (row0, row0 + N, dc.nrows))
    if o.p > abi.MAX_K:
        raise ValueError("at most %d columns per call" % abi.MAX_K)
    center = o.smp[0, o.cols_d.long(), row0].contiguous()
    partial = _doubles(o, o.L.fmcmc_gelman_partial_len(o.p))
    work = _doubles(o, o.L.fmcmc_gelman_work_len(o.Cn, o.p))
    gelman_partial_dev(o.smp, o.Cn, o.k, o.cap, row0, N, o.cols_d, center, work, partial)
    return partial, work, o.cols


def enqueue_gelman_groups(dc, ngroups, chains_per_group, row0, N, cols, active=None):
    """The one call site of fmcmc_gelman_groups_dev (current torch stream): the window [row0, row0 + N) of the rows of `dc`,
    whose chains are ngroups groups of chains_per_group consecutive chains (McmcBatch: a group = a dataset), reduced group by
    group, each centred on the window's first row of its first chain.  active: None or an int32 device tensor [ngroups]; the
    rows of the groups whose entry is 0 keep their NaN prefill.  Returns the device tensors (partials
    [ngroups][fmcmc_gelman_partial_len(p) + 2], work) and the columns; nothing is synchronised."""
    import torch
    o = _open(dc, cols, "compare")
    ngroups, cpg = int(ngroups), int(chains_per_group)
    if ngroups < 1 or cpg < 1 or ngroups * cpg != o.Cn:
        raise ValueError("%d groups of %d chains are not the %d chains of the result" % (ngroups, cpg, o.Cn))
    if row0 < 0 or N < 2 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) needs at least two of the %d kept rows" % (row0, row0 + N, dc.nrows))
    if o.p > abi.MAX_K_WAVE:
        raise NotImplementedError("the grouped Gelman-Rubin reduction takes at most %d columns per call" % abi.MAX_K_WAVE)
    if active is not None and (not torch.is_tensor(active) or active.dtype != torch.int32 or tuple(active.shape) != (ngroups,)
                               or not active.is_contiguous() or active.device != o.dev):
        raise ValueError("`active` must be a contiguous int32 tensor of shape [%d] on %s" % (ngroups, o.dev))
    plen = int(o.L.fmcmc_gelman_partial_len(o.p))
    partials = torch.full((ngroups, plen + 2), float("nan"), dtype=torch.float64, device=o.dev)
    work = _doubles(o, o.L.fmcmc_gelman_groups_work_len(ngroups, cpg, o.p))
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_gelman_groups_dev(o.smp.data_ptr(), ngroups, cpg, o.k, o.cap, int(row0), int(N), o.cols_d.data_ptr(), o.p,
                                         active.data_ptr() if active is not None else None, work.data_ptr(),
                                         partials.data_ptr(), _stream(o.dev))
    if rc != abi.OK:
        raise (NotImplementedError if rc == abi.ERR_UNSUPPORTED else ValueError if rc == abi.ERR_ARG else RuntimeError)(
            abi.last_error())
    return partials, work, o.cols


class GelmanDiagBatch(list):
    """gelman_diag() of an McmcBatch: a list of D GelmanDiag, one per dataset (what gelman_diag(ans[d]) returns), with the
    stacked arrays psrf [D][p][2] ("Point est.", "Upper C.I.") and mpsrf [D] (NaN where a GelmanDiag has None)."""

    def __init__(self, diags):
        super().__init__(diags)
        self.psrf = np.stack([g.psrf for g in self]) if len(self) else np.zeros((0, 0, 2))
        self.mpsrf = np.array([np.nan if g.mpsrf is None else g.mpsrf for g in self], dtype=np.float64)

    def __repr__(self):
        return "<GelmanDiagBatch ndatasets=%d nvar=%d>" % (len(self), self.psrf.shape[1])


def gelman_diag_batch(ans, confidence=0.95, autoburnin=True, multivariate=True, cols=None):
    """gelman_diag(ans[d]) for every dataset d of an McmcBatch from ONE grouped reduction (fmcmc_gelman_groups_dev) and one copy
    back: the same partial vectors bit for bit, the same host finish.  After MCMC_batch(stop_each = ...) the datasets hold
    different numbers of rows; each is tested on its own rows (its own autoburnin window), with one reduction per distinct
    row count -- at most one per bulk of that call."""
    import torch
    from .convergence import _window
    _single_process()
    if ans.nchains < 2:
        raise ValueError(_GELMAN_FEW_CHAINS)
    full = ans.history
    D = ans.nmodels
    counts = ans.nrows
    diags = [None] * D
    for nr in sorted(set(int(v) for v in counts)):
        sel = np.nonzero(counts == nr)[0]
        iters = full.iters[:nr]
        row0, N = _window(iters) if autoburnin else (0, nr)
        if N < 2:
            raise ValueError("the window [%d, %d) needs at least two of the %d kept rows" % (row0, row0 + N, nr))
        active = None
        if sel.size != D:
            mask = np.zeros(D, dtype=np.int32)
            mask[sel] = 1
            active = torch.as_tensor(mask).to(full._samples.device)
        partials, _work, cs = enqueue_gelman_groups(full, D, ans.nchains, row0, N, cols, active)
        ph = partials.cpu().numpy()
        p = int(cs.size)
        for d in sel:
            diags[d] = gelman_diag_finish(ph[d, :-2], p, N, confidence, multivariate, _names(full, cs), int(iters[row0]),
                                          int(iters[-1]))
    return GelmanDiagBatch(diags)


def gelman_diag(x, confidence=0.95, autoburnin=True, multivariate=True, cols=None):
    """coda::gelman.diag of a result: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first); an McmcBatch
    gives a GelmanDiagBatch, one GelmanDiag per dataset from one grouped reduction (gelman_diag_batch).  With
    `autoburnin` the factors are those of the second half of the rows (coda's window, the one convergence_gelman tests).
    The device reduces every chain's window to its mean and covariance and sums them (fmcmc_gelman_partial_dev, any
    p <= 256); gelman_diag_finish does the rest on that vector.  coda's `transform = TRUE` (log / logit of bounded
    variables before the test) is not offered: transform the columns before the call."""
    from .convergence import _window
    from .mcmc import Mcmc, McmcBatch, McmcList
    if isinstance(x, McmcBatch):
        return gelman_diag_batch(x, confidence, autoburnin, multivariate, cols)
    _single_process()
    if isinstance(x, Mcmc) or (isinstance(x, McmcList) and len(x) < 2):       # (before anything is uploaded)
        raise ValueError(_GELMAN_FEW_CHAINS)
    dc = _as_device_chains(x)
    if int(dc._samples.shape[0]) < 2:
        raise ValueError(_GELMAN_FEW_CHAINS)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    partial, _work, cols = enqueue_gelman(dc, row0, N, cols)
    return gelman_diag_finish(partial.cpu().numpy(), int(cols.size), N, confidence, multivariate, _names(dc, cols),
                              int(dc.iters[row0]), int(dc.iters[-1]))


# ------------------------------------------------------------------------------------------------ summary of an McmcBatch
def enqueue_summary_groups(dc, ngroups, chains_per_group, row0, N, cols, probs, active=None, want_chains=True):
    """The one call site of fmcmc_summary_groups_dev (current torch stream): the window [row0, row0 + N) of the rows of `dc`,
    whose chains are ngroups groups of chains_per_group consecutive chains (McmcBatch: a group = a dataset), summarised group by
    group.  active: None or an int32 device tensor [ngroups]; the rows of the groups whose entry is 0 keep their NaN prefill.
    Returns the device tensors (pooled [ngroups][fmcmc_summary_pooled_len(p, nprobs)], chain_stats [ngroups chains_per_group][p][4]
    or None, work) and the columns; nothing is synchronised."""
    import torch
    o = _open(dc, cols, "summarise")
    ngroups, cpg = int(ngroups), int(chains_per_group)
    if ngroups < 1 or cpg < 1 or ngroups * cpg != o.Cn:
        raise ValueError("%d groups of %d chains are not the %d chains of the result" % (ngroups, cpg, o.Cn))
    if row0 < 0 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    if active is not None and (not torch.is_tensor(active) or active.dtype != torch.int32 or tuple(active.shape) != (ngroups,)
                               or not active.is_contiguous() or active.device != o.dev):
        raise ValueError("`active` must be a contiguous int32 tensor of shape [%d] on %s" % (ngroups, o.dev))
    probs_h = np.ascontiguousarray(probs, dtype=np.float64)
    nprobs = int(probs_h.size)
    nan = float("nan")
    plen = max(int(o.L.fmcmc_summary_pooled_len(o.p, nprobs)), 1)
    pooled = torch.full((ngroups, plen), nan, dtype=torch.float64, device=o.dev)
    chain_stats = torch.full((o.Cn, o.p, 4), nan, dtype=torch.float64, device=o.dev) if want_chains else None
    work = _doubles(o, o.L.fmcmc_summary_groups_work_len(ngroups, cpg, o.p, nprobs))
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_summary_groups_dev(o.smp.data_ptr(), ngroups, cpg, o.k, o.cap, int(row0), int(N), o.cols_d.data_ptr(), o.p,
                                          active.data_ptr() if active is not None else None,
                                          probs_h.ctypes.data_as(C.POINTER(C.c_double)), nprobs, work.data_ptr(),
                                          chain_stats.data_ptr() if want_chains else None, pooled.data_ptr(), _stream(o.dev))
    if rc != abi.OK:
        raise (NotImplementedError if rc == abi.ERR_UNSUPPORTED else ValueError if rc == abi.ERR_ARG else RuntimeError)(
            abi.last_error())
    return pooled, chain_stats, work, o.cols


class McmcSummaryBatch(list):
    """summary() of an McmcBatch: a list of D McmcSummary, one per dataset (what summary(ans[d]) returns), with the stacked arrays
    a simulation study reads: statistics [D][p][4], quantiles [D][p][nprobs], ess [D][p], and per_chain (mean, sd, tsse, ess,
    spec0, order; each [D nchains][p], dataset by dataset)."""

    def __init__(self, summaries):
        super().__init__(summaries)
        stack = lambda get, tail: np.stack([get(s) for s in self]) if len(self) else np.zeros((0,) + tail)
        self.statistics = stack(lambda s: s.statistics, (0, 4))
        self.quantiles = stack(lambda s: s.quantiles, (0, 0))
        self.ess = stack(lambda s: s.ess, (0,))
        fields = ("mean", "sd", "tsse", "ess", "spec0", "order")
        self.per_chain = SimpleNamespace(**{f: np.concatenate([getattr(s.per_chain, f) for s in self]) for f in fields}) \
            if len(self) else None

    def __repr__(self):
        return "<McmcSummaryBatch ndatasets=%d nvar=%d>" % (len(self), self.statistics.shape[1])


def _pooled_parts(pooled_row, p, nprobs):
    """One row of the grouped call's `pooled` -> (pooled_stats [p][5], order_stats [p][nprobs][2])."""
    return pooled_row[:5 * p].reshape(p, 5), pooled_row[5 * p:5 * p + 2 * p * nprobs].reshape(p, nprobs, 2)


def summary_batch_finish(pooled, chain_stats, nchains, N, probs, varnames, start, end, thin, datasets=None):
    """The host finish of summary_batch(), pure numpy: pooled [D][5 p + 2 p nprobs] and chain_stats [D nchains][p][4] as
    fmcmc_summary_groups_dev leaves them, summarised over N rows per chain  ->  the list of McmcSummary of `datasets` (default:
    every row), each what summary() makes of that dataset alone: finish_statistics, type7_quantiles, _per_chain."""
    pooled = np.asarray(pooled, dtype=np.float64)
    probs = tuple(float(q) for q in probs)
    p, nprobs, nchains, N = len(varnames), len(probs), int(nchains), int(N)
    cs = np.asarray(chain_stats, dtype=np.float64).reshape(-1, nchains, p, 4)
    out = []
    for d in (range(pooled.shape[0]) if datasets is None else datasets):
        ps, os_ = _pooled_parts(pooled[d], p, nprobs)
        out.append(McmcSummary(finish_statistics(ps, nchains, N), type7_quantiles(os_, nchains * N, probs), probs, varnames,
                               start, end, thin, nchains, per_chain=_per_chain(cs[d], N), ess=ps[:, 3].copy()))
    return out


def _batch_calls(ans):
    """The grouped calls a (ragged) McmcBatch needs: one per distinct row count, (rows, datasets, mask or None)."""
    D, counts = ans.nmodels, np.asarray(ans.nrows)
    for nr in sorted(set(int(v) for v in counts)):
        sel = np.nonzero(counts == nr)[0]
        mask = None
        if sel.size != D:
            mask = np.zeros(D, dtype=np.int32)
            mask[sel] = 1
        yield nr, sel, mask


def _batch_groups(ans, nr, mask, cols, probs, want_chains):
    """One grouped call on the first nr rows of ans.history and ONE copy back: (pooled [D][.], chain_stats or None, columns)."""
    import torch
    full, D = ans.history, ans.nmodels
    active = None if mask is None else torch.as_tensor(mask).to(full._samples.device)
    pooled, chain_stats, _work, cs = enqueue_summary_groups(full, D, ans.nchains, 0, nr, cols, probs, active, want_chains)
    if not want_chains:
        return pooled.cpu().numpy(), None, cs
    both = torch.cat([pooled.reshape(-1), chain_stats.reshape(-1)]).cpu().numpy()
    return both[:pooled.numel()].reshape(D, -1), both[pooled.numel():].reshape(chain_stats.shape), cs


def _raise_non_finite_batch(pooled_h, sel, p, cols, what):
    for d in sel:
        try:
            _raise_non_finite(pooled_h[d, :5 * p].reshape(1, p, 5)[:, :, 4], cols, what)
        except ValueError as e:
            raise ValueError("dataset %d: %s" % (d, e)) from None


def summary_batch(ans, quantiles=DEFAULT_QUANTILES, cols=None):
    """summary(ans[d]) for every dataset d of an McmcBatch from ONE grouped call (fmcmc_summary_groups_dev) and one copy back:
    the same numbers bit for bit, the same host finish.  On a ragged result (MCMC_batch(stop_each = ...)) each dataset is
    summarised on its own rows with its own iteration labels, with one call per distinct row count -- at most one per bulk."""
    from .mcmc import McmcBatch
    if not isinstance(ans, McmcBatch):
        raise TypeError("summary_batch() expects an McmcBatch (the result of MCMC_batch)")
    _single_process()
    probs = tuple(float(q) for q in np.atleast_1d(np.asarray(quantiles, dtype=np.float64)))
    if len(probs) > abi.SUMMARY_MAX_PROBS:
        raise ValueError("at most %d quantiles per call" % abi.SUMMARY_MAX_PROBS)
    full = ans.history
    out = [None] * ans.nmodels
    for nr, sel, mask in _batch_calls(ans):
        pooled_h, chain_h, cs = _batch_groups(ans, nr, mask, cols, probs, True)
        _raise_non_finite_batch(pooled_h, sel, int(cs.size), cs, "summarise")
        iters = full.iters[:nr]
        for d, s in zip(sel, summary_batch_finish(pooled_h, chain_h, ans.nchains, nr, probs, _names(full, cs), int(iters[0]),
                                                  int(iters[-1]), full.thin, datasets=sel)):
            out[d] = s
    return McmcSummaryBatch(out)


def effective_size_batch(ans, cols=None):
    """effective_size(ans[d]) for every dataset of an McmcBatch, [D][p], from the grouped call without quantiles."""
    from .mcmc import McmcBatch
    if not isinstance(ans, McmcBatch):
        raise TypeError("effective_size_batch() expects an McmcBatch (the result of MCMC_batch)")
    _single_process()
    out = None
    for nr, sel, mask in _batch_calls(ans):
        pooled_h, _none, cs = _batch_groups(ans, nr, mask, cols, (), False)
        p = int(cs.size)
        _raise_non_finite_batch(pooled_h, sel, p, cs, "summarise")
        if out is None:
            out = np.empty((ans.nmodels, p))
        out[sel] = pooled_h[sel, :5 * p].reshape(sel.size, p, 5)[:, :, 3]
    return out


# ------------------------------------------------------------------------------------------------ HPD intervals
def hpd_gap(n, prob):
    """coda::HPDinterval: the rows an interval spans, max(1, min(n - 1, round(n prob))) with R's round (half to even)."""
    prob = float(prob)
    if not 0.0 < prob < 1.0:
        raise ValueError("`prob` must lie in (0, 1).")
    return int(max(1, min(int(n) - 1, int(np.rint(np.float64(n) * np.float64(prob))))))


def host_hpd_interval(series, prob=0.95, gap=None):
    """hpd_interval() without the device, from np.sort: series [..., n] -> (lower [...], upper [...], index [...]) of every
    series on its own: the first minimum over i of x_(i + gap) - x_(i), gap = hpd_gap(n, prob) unless it is given."""
    srt = np.sort(np.asarray(series, dtype=np.float64), axis=-1)
    n = srt.shape[-1]
    gap = hpd_gap(n, prob) if gap is None else int(gap)
    if not 1 <= gap <= n - 1:
        raise ValueError("gap = %d is outside [1, %d]" % (gap, n - 1))
    with np.errstate(over="ignore", invalid="ignore"):
        width = srt[..., gap:] - srt[..., :n - gap]
    index = np.argmin(width, axis=-1)                              # (the first of equal widths, as which.min)
    take = lambda a: np.take_along_axis(a, index[..., None], axis=-1)[..., 0]
    return take(srt[..., :n - gap]), take(srt[..., gap:]), index.astype(np.int64)


class HpdInterval:
    """coda::HPDinterval of every chain: lower, upper [C][p], index [C][p] (the 0-based rank of `lower` among the sorted rows of
    its series; `upper` is `gap` ranks above it), table [C][p][2] so that table[c] is coda's matrix of chain c, and the
    attribute probability = gap / nrows."""
    columns = ("lower", "upper")

    def __init__(self, lower, upper, index, gap, nrows, varnames=None):
        self.lower, self.upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
        self.index = np.asarray(index, dtype=np.int64)
        self.gap, self.nrows = int(gap), int(nrows)
        self.varnames = list(varnames) if varnames is not None else _par_names(range(self.lower.shape[1]))

    table = property(lambda self: np.stack([self.lower, self.upper], axis=-1))
    probability = property(lambda self: self.gap / self.nrows)

    def __str__(self):
        out = []
        for c, t in enumerate(self.table):
            out += ["[[%d]]" % (c + 1), _fmt_table(self.varnames, self.columns, t), 'attr(,"Probability")',
                    "[1] %.7g" % self.probability, ""]
        return "\n".join(out)

    def __repr__(self):
        return "<HpdInterval nchain=%d nvar=%d probability=%.4g>" % (self.lower.shape[0], self.lower.shape[1], self.probability)


def enqueue_hpd(dc, gap, cols):
    """Enqueues one fmcmc_hpd_dev call on the kept rows of `dc` (current torch stream) for intervals that span `gap` rows.
    Returns the device tensors (out [C][p][4] = lower, upper, i*, non-finite count; work [C][p][2], the two thresholds) and the
    columns; nothing is synchronised."""
    o = _open(dc, cols, "order")
    work = _doubles(o, o.L.fmcmc_hpd_work_len(o.Cn, o.p))
    out = _doubles(o, o.Cn * o.p * 4).view(o.Cn, o.p, 4)
    _windowed(o, o.L.fmcmc_hpd_dev, 0, dc.nrows, int(gap), work.data_ptr(), out.data_ptr())
    return out, work[:o.Cn * o.p * 2].view(o.Cn, o.p, 2), o.cols


def hpd_interval(x, prob=0.95, cols=None):
    """coda::HPDinterval of every chain on its own (HPDinterval.mcmc.list): x a DeviceChains (read in place), an Mcmc or a
    McmcList (uploaded first).  The device selects the two tails of every series that can hold an end of the interval, sorts
    them in LDS and finds the first shortest interval (csrc/raftery.hip: chain_hpd_kernel); the result has the bits of
    host_hpd_interval.  A tail holds at most 8192 rows: 163840 rows per chain at prob = 0.95."""
    dc = _as_device_chains(x)
    n = int(dc.nrows)
    gap = hpd_gap(n, prob)
    out, _work, cols = enqueue_hpd(dc, gap, cols)
    oh = out.cpu().numpy()
    _raise_non_finite(oh[:, :, 3], cols, "order")
    return HpdInterval(oh[:, :, 0].copy(), oh[:, :, 1].copy(), oh[:, :, 2].astype(np.int64), gap, n,
                       _names(dc, cols) if dc.names is not None else None)


# ------------------------------------------------------------------------------------------------ autocorrelation
DEFAULT_LAGS = (0, 1, 5, 10, 50)


def autocorr_lags(lags, niter, thin, relative=True):
    """coda::autocorr's lags: (labels, row lags).  With `relative` the lags count kept rows (label = lag thin); without, they are
    iteration labels and must be multiples of the thinning.  Labels that are not below niter thin are dropped."""
    lags = np.atleast_1d(np.asarray(lags, dtype=np.int64))
    thin = int(thin)
    if relative:
        labels = lags * thin
    elif np.any(lags % thin != 0):
        raise ValueError("Lags do not conform to thinning interval")
    else:
        labels = lags
    labels = labels[labels < int(niter) * thin]
    if labels.size < 1:
        raise ValueError("no lag below the %d rows of a chain" % int(niter))
    return labels, labels // thin


def host_autocov(series, lags):
    """series [..., n], row lags [nlags] -> (mean [...], c_0 [...], c_h [..., nlags]) as stats::acf(type = "covariance") forms
    them in float64: the series centred on its mean, sum of products, divisor n."""
    x = np.asarray(series, dtype=np.float64)
    n = x.shape[-1]
    mean = x.sum(axis=-1) / n
    xc = x - mean[..., None]
    c = np.stack([(xc[..., :n - h] * xc[..., h:]).sum(axis=-1) / n for h in (int(h) for h in lags)], axis=-1)
    return mean, (xc * xc).sum(axis=-1) / n, c


def host_autocorr(series, lags):
    """autocorr_diag() without the device: series [..., n], row lags [nlags] -> acf [..., nlags] = c_h / c_0 (NaN for a
    constant series)."""
    _, c0, c = host_autocov(series, lags)
    with np.errstate(divide="ignore", invalid="ignore"):
        return c / c0[..., None]


class AutocorrDiag:
    """coda::autocorr.diag: acov and acf [C][nlags][p] (c_h and c_h / c_0 of every chain), mean [nlags][p] (the chains' acf
    summed in chain order and divided by C: what coda reports for an mcmc.list), lags [nlags] (iteration labels; `rows`: the
    same lags in kept rows), c0 and chain_mean [C][p].  print(): the table of `mean` with coda's row names."""

    def __init__(self, acov, c0, lags, rows, varnames=None, chain_mean=None):
        self.acov = np.asarray(acov, dtype=np.float64)
        self.c0 = np.asarray(c0, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.acf = self.acov / self.c0[:, None, :]
        total = self.acf[0].copy()
        for c in range(1, self.acf.shape[0]):
            total = total + self.acf[c]
        self.mean = total / self.acf.shape[0]
        self.lags, self.rows = np.asarray(lags, dtype=np.int64), np.asarray(rows, dtype=np.int64)
        self.chain_mean = chain_mean
        self.varnames = list(varnames) if varnames is not None else _par_names(range(self.acov.shape[2]))

    rownames = property(lambda self: ["Lag %d" % l for l in self.lags])

    def __str__(self):
        return _fmt_table(self.rownames, self.varnames, self.mean)

    def __repr__(self):
        return "<AutocorrDiag nchain=%d nvar=%d lags=%s>" % (self.acov.shape[0], self.acov.shape[2], self.lags.tolist())


def enqueue_autocov(dc, lags, cols):
    """Enqueues one fmcmc_autocov_dev call on the kept rows of `dc` (current torch stream) at the row `lags` (1 to 32, distinct,
    each below the rows of a chain).  Returns the device tensors (out [C][p][3 + nlags] = mean, c_0, non-finite count, then c_h
    per lag; work [C][p], the non-finite counts) and the columns; nothing is synchronised."""
    o = _open(dc, cols, "correlate")
    lags = np.ascontiguousarray(lags, dtype=np.int64).ravel()
    nl = int(lags.size)
    work = _doubles(o, o.Cn * o.p)
    out = _doubles(o, max(o.L.fmcmc_autocov_out_len(o.Cn, o.p, nl), o.Cn * o.p * (3 + nl)))
    _windowed(o, o.L.fmcmc_autocov_dev, 0, dc.nrows, lags.ctypes.data_as(C.POINTER(C.c_int64)), nl, work.data_ptr(), out.data_ptr())
    return out[:o.Cn * o.p * (3 + nl)].view(o.Cn, o.p, 3 + nl), work.view(o.Cn, o.p), o.cols


def autocorr_diag(x, lags=DEFAULT_LAGS, relative=True, cols=None):
    """coda::autocorr.diag of a result: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first).  The device
    forms every chain's autocovariances at the lags asked for (csrc/summary.hip: summary_lag_kernel; summary() keeps them up to
    the AR order only); the division by c_0 and the mean over the chains are done here.  At most 32 lags per call."""
    dc = _as_device_chains(x)
    labels, rows = autocorr_lags(lags, dc.nrows, dc.thin, relative)
    out, _work, cols = enqueue_autocov(dc, rows, cols)
    oh = out.cpu().numpy()
    _raise_non_finite(oh[:, :, 2], cols, "correlate")
    return AutocorrDiag(np.ascontiguousarray(oh[:, :, 3:].transpose(0, 2, 1)), oh[:, :, 1].copy(), labels, rows,
                        _names(dc, cols) if dc.names is not None else None, chain_mean=oh[:, :, 0].copy())


# ------------------------------------------------------------------------------------------------ cross-correlation
def crosscorr_finish(partial, p, N):
    """The host finish of crosscorr(): a pure function of the partial vector of fmcmc_gelman_partial_dev (include/fmcmc_amd.h:
    m, sum xbar [p], sum xbar xbar^T [p][p], sum S_c [p][p], ...), p and the rows N of a chain.  The covariance of the m N pooled
    rows is ((N - 1) sum S_c + N (sum xbar xbar^T - m mu mu^T)) / (m N - 1) with mu = sum xbar / m (the means may be relative to
    any centre: a covariance does not move with it); the correlation is cov_ij / sqrt(cov_ii cov_jj), its diagonal exactly 1,
    and NaN in the row and column of a variable whose variance is 0 (R: NA, "the standard deviation is zero")."""
    P = np.ascontiguousarray(partial, dtype=np.float64)
    p, N = int(p), int(N)
    if p < 1 or N < 2 or P.size < 1 + p + 2 * p * p:
        raise ValueError("crosscorr: a partial of at least 1 + p + 2p^2 numbers, p >= 1 and N >= 2 rows are needed")
    m = float(P[0])
    if m < 1:
        raise ValueError("crosscorr: the partial holds no chain")
    sx = P[1:1 + p]
    sxx = P[1 + p:1 + p + p * p].reshape(p, p)
    sS = P[1 + p + p * p:1 + p + 2 * p * p].reshape(p, p)
    mu = sx / m
    cov = ((N - 1.0) * sS + N * (sxx - m * np.outer(mu, mu))) / (m * N - 1.0)
    var = cov.diagonal().copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        cor = cov / np.sqrt(np.outer(var, var))
    flat = ~(var > 0.0)
    cor[flat, :] = np.nan
    cor[:, flat] = np.nan
    cor[np.arange(p), np.arange(p)] = np.where(flat, np.nan, 1.0)
    return cor


def crosscorr(x, cols=None):
    """coda::crosscorr: the correlation matrix [p][p] of the pooled rows of all chains (p <= 256): x a DeviceChains (read in
    place), an Mcmc or a McmcList (uploaded first).  One fmcmc_gelman_partial_dev call over all kept rows sums every chain's
    mean and covariance; crosscorr_finish pools them.  One chain is enough."""
    dc = _as_device_chains(x)
    N = int(dc.nrows)
    partial, _work, cols = enqueue_gelman(dc, 0, N, cols)
    return crosscorr_finish(partial.cpu().numpy(), int(cols.size), N)


# ------------------------------------------------------------------------------------------------ rank-normalised split R-hat
class RhatDiag:
    """rhat() of a result: per column the rank-normalised split R-hat of Vehtari et al. (2021): bulk [p] (on the values), tail
    [p] (on |x - median|), rhat [p] = max(bulk, tail) (NaN when either is: a constant column), median [p] = the fold point, the
    mean of the two middle pooled values; nchains, niter = the chains and the rows of each the values came from, and the window
    [start, end] of iteration labels."""
    columns = ("Bulk", "Tail", "R-hat")

    def __init__(self, bulk, tail, median, nchains, niter, varnames=None, start=None, end=None):
        self.bulk = np.asarray(bulk, dtype=np.float64).reshape(-1)
        self.tail = np.asarray(tail, dtype=np.float64).reshape(-1)
        self.rhat = rhat_max(self.bulk, self.tail)
        self.median = np.asarray(median, dtype=np.float64).reshape(-1)
        self.nchains, self.niter = int(nchains), int(niter)
        self.varnames = list(varnames) if varnames is not None else _par_names(range(self.bulk.size))
        self.start, self.end = start, end

    def __str__(self):
        table = np.stack([self.bulk, self.tail, self.rhat], axis=1)
        return "\n".join(["Rank-normalised split R-hat (%d chains of %d rows, split in two):" % (self.nchains, self.niter), "",
                          _fmt_table(self.varnames, self.columns, table, _fmt_column_sig)]) + "\n"

    def __repr__(self):
        return "<RhatDiag nvar=%d max=%.4g>" % (self.bulk.size, np.max(self.rhat) if self.rhat.size else np.nan)


def rhat_max(bulk, tail):
    """max(bulk, tail), NaN where either is NaN."""
    return np.where(np.isnan(bulk) | np.isnan(tail), np.nan, np.maximum(bulk, tail))


def rhat_of_moments(means, variances, nh):
    """Step 4 of the definition on the means and unbiased variances [..., m] of the scores of m split
    chains of nh rows: B = nh var(means, ddof 1), W = mean(variances), sqrt((B / W + nh - 1) / nh), in np.longdouble, returned
    as float64; NaN where W == 0."""
    mu = np.asarray(means, dtype=np.longdouble)
    s2 = np.asarray(variances, dtype=np.longdouble)
    m, nh = mu.shape[-1], np.longdouble(nh)
    dev = mu - mu.sum(axis=-1, keepdims=True) / m
    B = nh * (dev * dev).sum(axis=-1) / (m - 1)
    W = s2.sum(axis=-1) / m
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt((B / W + nh - 1) / nh)
    return np.where(W == 0, np.nan, r).astype(np.float64)


def rhat_finish(out, nchains, nh):
    """The host finish of rhat(): `out` of fmcmc_rank_rhat_dev (per column the [2 C][2] means and variances of the bulk scores,
    those of the tail scores, the non-finite count, med) -> a namespace of bulk, tail, rhat, median, non_finite, each [p]."""
    m = 2 * int(nchains)
    o = np.asarray(out, dtype=np.float64).reshape(-1, 4 * m + 2)
    mom = o[:, :4 * m].reshape(-1, 2, m, 2)
    r = rhat_of_moments(mom[..., 0], mom[..., 1], nh)           # [p][2]
    return SimpleNamespace(bulk=r[:, 0], tail=r[:, 1], rhat=rhat_max(r[:, 0], r[:, 1]), median=o[:, 4 * m + 1].copy(),
                           non_finite=o[:, 4 * m].copy())


def _rank_window(dc, o, row0, N):
    if row0 < 0 or N < 4 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) needs at least four of the %d kept rows" % (row0, row0 + N, dc.nrows))
    return _doubles(o, o.L.fmcmc_rank_work_len(o.Cn, o.p, int(N)))


def enqueue_rank_rhat(dc, row0, N, cols):
    """Enqueues one fmcmc_rank_rhat_dev call on the window [row0, row0 + N) of the kept rows of `dc` (current torch stream).
    Returns the device tensors (out [p][8 C + 2], work) and the columns; nothing is synchronised."""
    o = _open(dc, cols, "rank")
    work = _rank_window(dc, o, row0, N)
    out = _doubles(o, o.L.fmcmc_rank_rhat_out_len(o.Cn, o.p)).view(o.p, 8 * o.Cn + 2)
    _windowed(o, o.L.fmcmc_rank_rhat_dev, row0, N, work.data_ptr(), out.data_ptr())
    return out, work, o.cols


def enqueue_rank_scores(dc, row0, N, cols, fold=False, what=0):
    """Enqueues one fmcmc_rank_scores_dev call (current torch stream): returns the device tensors (scores [p][2 C][N / 2]:
    z, or 2 r with what = 1; info [p][2] = non-finite count, med; work) and the columns; nothing is synchronised."""
    o = _open(dc, cols, "rank")
    work = _rank_window(dc, o, row0, N)
    out = _doubles(o, o.p * 2 * o.Cn * (int(N) // 2)).view(o.p, 2 * o.Cn, int(N) // 2)
    info = _doubles(o, 2 * o.p).view(o.p, 2)
    _windowed(o, o.L.fmcmc_rank_scores_dev, row0, N, int(bool(fold)), int(what), work.data_ptr(), out.data_ptr(), info.data_ptr())
    return out, info, work, o.cols


def rank_scores(x, fold=False, cols=None):
    """The rank-normalised scores z behind rhat(), for rank plots: a device tensor [p][2 C][N'] (split chain 2 c = the first
    N' = N // 2 rows of chain c, 2 c + 1 its last N'), of the values or, with `fold`, of |x - median|."""
    dc = _as_device_chains(x)
    out, info, _work, cols = enqueue_rank_scores(dc, 0, int(dc.nrows), cols, fold)
    _raise_non_finite(info[:, 0].cpu().numpy()[None, :], cols, "rank")
    return out


def rhat(x, autoburnin=False, cols=None):
    """Rank-normalised split R-hat (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; the `rhat` of Stan, posterior and
    ArviZ) of a result: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first); an McmcBatch gives a
    RhatDiagBatch, one RhatDiag per dataset from one grouped call (rhat_batch).  With `autoburnin` the rows are coda's window (the second half, as gelman_diag takes it).
    The device sorts the pooled values of every column through HBM, ranks them with ties averaged, and reduces the scores of
    every split chain to a mean and a variance (csrc/diag_rank.hpp); rhat_finish does the rest.  One chain is enough.  For an
    odd number of rows the middle row takes part in nothing, the median included (posterior and ArviZ keep it there)."""
    from .convergence import _window
    from .mcmc import McmcBatch
    if isinstance(x, McmcBatch):
        return rhat_batch(x, autoburnin, cols)
    dc = _as_device_chains(x)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    out, _work, cols = enqueue_rank_rhat(dc, row0, N, cols)
    Cn = int(dc._samples.shape[0])
    fin = rhat_finish(out.cpu().numpy(), Cn, N // 2)
    _raise_non_finite(fin.non_finite[None, :], cols, "rank")
    return RhatDiag(fin.bulk, fin.tail, fin.median, Cn, N, _names(dc, cols), int(dc.iters[row0]), int(dc.iters[-1]))


# ------------------------------------------------------------------------------------------------ R-hat of an McmcBatch
def rank_groups_fit(chains_per_group, N):
    """Does a group of chains_per_group chains x N rows fit the grouped call: M = 2 chains_per_group (N // 2) pooled values of
    a column at most fmcmc_rank_groups_max_values() (the keys of a group are sorted in LDS)."""
    return 2 * int(chains_per_group) * (int(N) // 2) <= int(abi.lib().fmcmc_rank_groups_max_values())


def enqueue_rank_rhat_groups(dc, ngroups, chains_per_group, row0, N, cols, active=None, want_scores=False):
    """The one call site of fmcmc_rank_rhat_groups_dev (current torch stream): the window [row0, row0 + N) of the rows of `dc`,
    whose chains are ngroups groups of chains_per_group consecutive chains (McmcBatch: a group = a dataset), each group ranked
    on its own.  active: None or an int32 device tensor [ngroups]; the rows of the groups whose entry is 0 keep their NaN
    prefill.  Returns the device tensors (out [ngroups][p][8 chains_per_group + 2], scores [ngroups][p][2][2 chains_per_group]
    [N // 2] or None, work) and the columns; nothing is synchronised."""
    import torch
    o = _open(dc, cols, "rank")
    ngroups, cpg = int(ngroups), int(chains_per_group)
    if ngroups < 1 or cpg < 1 or ngroups * cpg != o.Cn:
        raise ValueError("%d groups of %d chains are not the %d chains of the result" % (ngroups, cpg, o.Cn))
    if row0 < 0 or N < 4 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) needs at least four of the %d kept rows" % (row0, row0 + N, dc.nrows))
    if active is not None and (not torch.is_tensor(active) or active.dtype != torch.int32 or tuple(active.shape) != (ngroups,)
                               or not active.is_contiguous() or active.device != o.dev):
        raise ValueError("`active` must be a contiguous int32 tensor of shape [%d] on %s" % (ngroups, o.dev))
    nan = float("nan")
    out = torch.full((ngroups, o.p, 8 * cpg + 2), nan, dtype=torch.float64, device=o.dev)
    scores = torch.full((ngroups, o.p, 2, 2 * cpg, int(N) // 2), nan, dtype=torch.float64, device=o.dev) if want_scores else None
    work = _doubles(o, max(int(o.L.fmcmc_rank_rhat_groups_work_len(ngroups, cpg, o.p, int(N))), 1))
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_rank_rhat_groups_dev(o.smp.data_ptr(), ngroups, cpg, o.k, o.cap, int(row0), int(N), o.cols_d.data_ptr(), o.p,
                                            active.data_ptr() if active is not None else None, work.data_ptr(),
                                            scores.data_ptr() if want_scores else None, out.data_ptr(), _stream(o.dev))
    if rc != abi.OK:
        raise (NotImplementedError if rc == abi.ERR_UNSUPPORTED else ValueError if rc == abi.ERR_ARG else RuntimeError)(
            abi.last_error())
    return out, scores, work, o.cols


class RhatDiagBatch(list):
    """rhat() of an McmcBatch: a list of D RhatDiag, one per dataset (what rhat(ans[d]) returns), with the stacked arrays bulk,
    tail, rhat and median, each [D][p]."""

    def __init__(self, diags):
        super().__init__(diags)
        stack = lambda get: np.stack([get(r) for r in self]) if len(self) else np.zeros((0, 0))
        self.bulk, self.tail = stack(lambda r: r.bulk), stack(lambda r: r.tail)
        self.rhat, self.median = stack(lambda r: r.rhat), stack(lambda r: r.median)

    def __repr__(self):
        return "<RhatDiagBatch ndatasets=%d nvar=%d>" % (len(self), self.bulk.shape[1])


def rhat_groups_finish(out, chains_per_group, nh):
    """The host finish of the grouped call, pure numpy: out [D][p][8 chains_per_group + 2] as fmcmc_rank_rhat_groups_dev leaves
    it -> a namespace of bulk, tail, rhat, median, non_finite, each [D][p]: row d is rhat_finish(out[d])."""
    o = np.asarray(out, dtype=np.float64)
    D, p = o.shape[0], o.shape[1]
    fin = rhat_finish(o.reshape(D * p, -1), chains_per_group, nh)
    return SimpleNamespace(**{f: getattr(fin, f).reshape(D, p) for f in ("bulk", "tail", "rhat", "median", "non_finite")})


def rhat_batch(ans, autoburnin=False, cols=None):
    """rhat(ans[d]) for every dataset d of an McmcBatch from ONE grouped call (fmcmc_rank_rhat_groups_dev) and one copy back: the
    same moments bit for bit, the same host finish.  On a ragged result (MCMC_batch(stop_each = ...)) each dataset is ranked on
    its own rows (its own autoburnin window) with its own iteration labels, with one call per distinct row count.  A row count
    at which a dataset's pooled values do not fit the grouped call (rank_groups_fit) is served dataset by dataset."""
    import torch
    from .convergence import _window
    from .mcmc import McmcBatch
    if not isinstance(ans, McmcBatch):
        raise TypeError("rhat_batch() expects an McmcBatch (the result of MCMC_batch)")
    _single_process()
    full, D, Cm = ans.history, ans.nmodels, ans.nchains
    diags = [None] * D
    for nr, sel, mask in _batch_calls(ans):
        iters = full.iters[:nr]
        row0, N = _window(iters) if autoburnin else (0, nr)
        if N < 4 or not rank_groups_fit(Cm, N):           # (too few rows: the single form's text)
            for d in sel:
                try:
                    diags[d] = rhat(ans[int(d)], autoburnin, cols)
                except ValueError as e:
                    raise ValueError("dataset %d: %s" % (d, e)) from None
            continue
        active = None if mask is None else torch.as_tensor(mask).to(full._samples.device)
        out, _scores, _work, cs = enqueue_rank_rhat_groups(full, D, Cm, row0, N, cols, active)
        fin = rhat_groups_finish(out.cpu().numpy()[sel], Cm, N // 2)
        for i, d in enumerate(sel):
            try:
                _raise_non_finite(fin.non_finite[i][None, :], cs, "rank")
            except ValueError as e:
                raise ValueError("dataset %d: %s" % (d, e)) from None
            diags[d] = RhatDiag(fin.bulk[i], fin.tail[i], fin.median[i], Cm, N, _names(full, cs), int(iters[row0]), int(iters[-1]))
    return RhatDiagBatch(diags)


def rhat_batch_verdicts(rhat, threshold, tested=None):
    """The verdict of convergence_rhat per dataset, pure numpy: rhat [D][p] (max(bulk, tail) of every free column) -> (values
    [D], passed [D]): the value of a dataset is the largest of its row, NaN when any of them is; it passes when the value is
    below the threshold (a NaN never does).  Datasets outside `tested` (a bool mask [D]) have the value NaN and do not pass."""
    r = np.asarray(rhat, dtype=np.float64)
    r = r.reshape(r.shape[0], -1)
    with np.errstate(invalid="ignore"):
        vals = np.where(np.isnan(r).any(axis=1), np.nan, np.max(np.where(np.isnan(r), -np.inf, r), axis=1, initial=-np.inf))
        if tested is not None:
            vals = np.where(np.asarray(tested, dtype=bool), vals, np.nan)
        return vals, vals < float(threshold)


# ------------------------------------------------------------------------------------------------ rank-normalised bulk / tail ESS
ESS_KINDS = ("bulk", "q05", "q95", "mean")         # the four series of a column, in the order of fmcmc_rank_ess_dev's `out`
ESS_INFO = 7                                       # non-finite count, q05, q95, pooled mean, pooled sd, least, largest value


class LagsNeeded(ValueError):
    """geyer_tau was given fewer lags than its pair test asks for."""


def ess_lag_cap(n):
    """The number of lags 0 .. n - 3 the definition may use."""
    return int(n) - 2


def geyer_tau(S, m, n, means, variances=None):
    """The finish of the definition: S = S(0) .. S(L - 1), the autocovariances of m split chains of n rows
    summed over the chains, and the chains' means -> a namespace of tau, ess = m n / tau, K (the pairs kept), W, V.  Everything up
    to the cut is float64, plain IEEE operations in the written order: geyer_scan_kernel (csrc/diag_ess.hpp) evaluates the same
    expressions, so the device never stops before a lag this function asks for.  Raises LagsNeeded when it does need one that S
    does not hold.  `variances` (the chains' unbiased variances, which callers have at hand) take no part: W comes from S(0)."""
    S = np.asarray(S, dtype=np.float64).ravel()
    m, n, L = int(m), int(n), int(S.size)
    cap = ess_lag_cap(n)
    if n < 4 or L < 2 or L > cap:
        raise ValueError("geyer_tau: n = %d rows and %d lags; n >= 4 and between 2 and n - 2 lags are needed" % (n, L))
    dm, dn = np.float64(m), np.float64(n)
    grand = np.float64(0.0)
    for v in np.asarray(means, dtype=np.float64).ravel():
        grand = grand + v
    grand = grand / dm
    d2 = np.float64(0.0)
    for v in np.asarray(means, dtype=np.float64).ravel():
        d = v - grand
        d2 = d2 + d * d
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        W = S[0] / dm * dn / (dn - 1.0)
        V = S[0] / dm + d2 / (dm - 1.0) if m > 1 else S[0] / dm
        rho = 1.0 - (W - S / dm) / V
    rho[0] = 1.0
    have = L // 2                                   # pairs with both lags in S
    jcap = cap // 2                                 # the first j with 2 j + 1 > n - 3
    P = rho[0:2 * have:2] + rho[1:2 * have:2]
    upto = min(have, jcap)
    bad = np.flatnonzero(~(P[1:upto] >= 0.0))
    if bad.size:
        K = int(bad[0]) + 1
    elif have >= jcap:
        K = jcap
    else:
        raise LagsNeeded("geyer_tau: the pair test is undecided after %d lags of at most %d" % (L, cap))
    tau = -1.0 + 2.0 * np.sum(np.minimum.accumulate(P[:K]))
    if 2 * K <= n - 3:
        if 2 * K >= L:
            raise LagsNeeded("geyer_tau: lag %d is needed, %d lags were given" % (2 * K, L))
        if rho[2 * K] > 0.0:
            tau = tau + rho[2 * K]
    tau = max(tau, 1.0 / np.log10(dm * dn))
    if not V > 0.0:
        tau = np.float64(np.nan)
    return SimpleNamespace(tau=float(tau), ess=float(dm * dn / tau), K=K, W=float(W), V=float(V))


def ess_finish(out, nchains, N):
    """The host finish of ess(): `out` of fmcmc_rank_ess_dev -> a namespace of bulk, tail_q05, tail_q95, tail, mean, mcse_mean,
    tau_bulk, q05, q95, non_finite, pooled_mean, pooled_sd [p], lags, computed, device_lags [p][4] (K of geyer_tau, the lags L
    the device computed and the K it stopped at, per series in the order of ESS_KINDS).  A column whose values are all equal
    gives NaN for every ESS.  Raises LagsNeeded if the device stopped before a lag the finish needs."""
    m, n = 2 * int(nchains), int(N) // 2
    cap = ess_lag_cap(n)
    kl = 2 * m + 2 + cap
    o = np.asarray(out, dtype=np.float64).reshape(-1, len(ESS_KINDS) * kl + ESS_INFO)
    p = o.shape[0]
    info = o[:, len(ESS_KINDS) * kl:]
    ess = np.full((p, 4), np.nan)
    tau = np.full((p, 4), np.nan)
    lags = np.zeros((p, 4), dtype=np.int64)
    computed = np.zeros((p, 4), dtype=np.int64)
    device_lags = np.zeros((p, 4), dtype=np.int64)
    for j in range(p):
        if info[j, 0] != 0:
            continue                                 # non-finite values: the caller raises
        for kind in range(4):
            part = o[j, kind * kl:(kind + 1) * kl]
            L = int(part[2 * m])
            computed[j, kind], device_lags[j, kind] = L, int(part[2 * m + 1])
            g = geyer_tau(part[2 * m + 2:2 * m + 2 + L], m, n, part[0:2 * m:2], part[1:2 * m:2])
            lags[j, kind] = g.K
            if info[j, 5] != info[j, 6]:
                ess[j, kind], tau[j, kind] = g.ess, g.tau
    with np.errstate(invalid="ignore", divide="ignore"):
        mcse = info[:, 4] / np.sqrt(ess[:, 3])
    return SimpleNamespace(bulk=ess[:, 0], tail_q05=ess[:, 1], tail_q95=ess[:, 2], tail=np.minimum(ess[:, 1], ess[:, 2]),
                           mean=ess[:, 3], mcse_mean=mcse, tau_bulk=tau[:, 0], q05=info[:, 1].copy(), q95=info[:, 2].copy(),
                           non_finite=info[:, 0].copy(), pooled_mean=info[:, 3].copy(), pooled_sd=info[:, 4].copy(),
                           lags=lags, computed=computed, device_lags=device_lags)


class EssDiag:
    """ess() of a result, per column: bulk (the ESS of the rank-normalised values), tail = min(tail_q05, tail_q95) (the ESS of
    the indicators x <= q05, x <= q95; q05, q95 the type-7 quantiles of the pooled values), mean (the ESS of the values) and
    mcse_mean = pooled sd / sqrt(mean); tau_bulk = m n / bulk; lags [p][4] = the pairs K kept for bulk, q05, q95, mean; NaN for
    a constant column (and for an indicator that is constant).  nchains, niter = the chains and the rows of each the values came
    from, and the window [start, end] of iteration labels."""
    columns = ("Bulk", "Tail", "Mean", "MCSE")

    def __init__(self, fin, nchains, niter, varnames=None, start=None, end=None):
        for name in ("bulk", "tail", "tail_q05", "tail_q95", "mean", "mcse_mean", "tau_bulk", "q05", "q95"):
            setattr(self, name, np.asarray(getattr(fin, name), dtype=np.float64).reshape(-1))
        self.lags = np.asarray(fin.lags, dtype=np.int64).reshape(-1, 4)
        self.nchains, self.niter = int(nchains), int(niter)
        self.varnames = list(varnames) if varnames is not None else _par_names(range(self.bulk.size))
        self.start, self.end = start, end

    def __str__(self):
        table = np.stack([self.bulk, self.tail, self.mean, self.mcse_mean], axis=1)
        return "\n".join(["Rank-normalised effective sample size (%d chains of %d rows, split in two):"
                          % (self.nchains, self.niter), "",
                          _fmt_table(self.varnames, self.columns, table, _fmt_column_sig)]) + "\n"

    def __repr__(self):
        both = np.minimum(self.bulk, self.tail)
        return "<EssDiag nvar=%d min=%.4g>" % (self.bulk.size, np.min(both) if both.size else np.nan)


def enqueue_rank_ess(dc, row0, N, cols):
    """Enqueues one fmcmc_rank_ess_dev call on the window [row0, row0 + N) of the kept rows of `dc` (current torch stream).
    Returns the device tensors (out [p][4 (4 C + 2 + N // 2 - 2) + 7], work) and the columns; nothing is synchronised."""
    o = _open(dc, cols, "rank")
    if row0 < 0 or N < 8 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) needs at least eight of the %d kept rows" % (row0, row0 + N, dc.nrows))
    work = _doubles(o, o.L.fmcmc_rank_ess_work_len(o.Cn, o.p, int(N)))
    out = _doubles(o, o.L.fmcmc_rank_ess_out_len(o.Cn, o.p, int(N))).view(o.p, -1)
    _windowed(o, o.L.fmcmc_rank_ess_dev, row0, N, work.data_ptr(), out.data_ptr())
    return out, work, o.cols


def ess(x, autoburnin=False, cols=None):
    """Rank-normalised bulk and tail effective sample size (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; `ess_bulk`,
    `ess_tail`, `ess_mean`, `mcse_mean` of posterior) of a result, to be read beside rhat(): x a DeviceChains (read in place),
    an Mcmc or a McmcList (uploaded first); an McmcBatch gives an EssDiagBatch, one EssDiag per dataset from one grouped call (ess_batch).  With `autoburnin` the
    rows are coda's window (the second half).  The device sorts and ranks the pooled values as rhat() does, sums the
    autocovariances of every split chain at every lag up to Geyer's cut on the fp64 matrix cores and finds the cut itself
    (csrc/diag_ess.hpp); ess_finish does the rest.  At least 8 rows; one chain is enough."""
    from .convergence import _window
    from .mcmc import McmcBatch
    if isinstance(x, McmcBatch):
        return ess_batch(x, autoburnin, cols)
    dc = _as_device_chains(x)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    out, _work, cols = enqueue_rank_ess(dc, row0, N, cols)
    Cn = int(dc._samples.shape[0])
    fin = ess_finish(out.cpu().numpy(), Cn, N)
    _raise_non_finite(fin.non_finite[None, :], cols, "rank")
    return EssDiag(fin, Cn, N, _names(dc, cols), int(dc.iters[row0]), int(dc.iters[-1]))


# ------------------------------------------------------------------------------------------------ ESS of an McmcBatch
ESS_FIELDS = ("bulk", "tail_q05", "tail_q95", "tail", "mean", "mcse_mean", "tau_bulk", "q05", "q95", "non_finite", "pooled_mean",
              "pooled_sd", "lags", "computed", "device_lags")


def enqueue_rank_ess_groups(dc, ngroups, chains_per_group, row0, N, cols, active=None):
    """The one call site of fmcmc_rank_ess_groups_dev (current torch stream): the window [row0, row0 + N) of the rows of `dc`,
    whose chains are ngroups groups of chains_per_group consecutive chains (McmcBatch: a group = a dataset), each group on its
    own.  active: None or an int32 device tensor [ngroups]; the rows of the groups whose entry is 0 keep their NaN prefill.
    Returns the device tensors (out [ngroups][p][4 (4 chains_per_group + 2 + N // 2 - 2) + 7], NaN where the call wrote nothing;
    work) and the columns; nothing is synchronised."""
    import torch
    o = _open(dc, cols, "rank")
    ngroups, cpg = int(ngroups), int(chains_per_group)
    if ngroups < 1 or cpg < 1 or ngroups * cpg != o.Cn:
        raise ValueError("%d groups of %d chains are not the %d chains of the result" % (ngroups, cpg, o.Cn))
    if row0 < 0 or N < 8 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) needs at least eight of the %d kept rows" % (row0, row0 + N, dc.nrows))
    if active is not None and (not torch.is_tensor(active) or active.dtype != torch.int32 or tuple(active.shape) != (ngroups,)
                               or not active.is_contiguous() or active.device != o.dev):
        raise ValueError("`active` must be a contiguous int32 tensor of shape [%d] on %s" % (ngroups, o.dev))
    m, n = 2 * cpg, int(N) // 2
    out = torch.full((ngroups, o.p, len(ESS_KINDS) * (2 * m + 2 + ess_lag_cap(n)) + ESS_INFO), float("nan"), dtype=torch.float64,
                     device=o.dev)
    work = _doubles(o, o.L.fmcmc_rank_ess_groups_work_len(ngroups, cpg, o.p, int(N)))
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_rank_ess_groups_dev(o.smp.data_ptr(), ngroups, cpg, o.k, o.cap, int(row0), int(N), o.cols_d.data_ptr(), o.p,
                                           active.data_ptr() if active is not None else None, work.data_ptr(), out.data_ptr(),
                                           _stream(o.dev))
    if rc != abi.OK:
        raise (NotImplementedError if rc == abi.ERR_UNSUPPORTED else ValueError if rc == abi.ERR_ARG else RuntimeError)(
            abi.last_error())
    return out, work, o.cols


def geyer_tau_rows(S, L, m, n, means):
    """geyer_tau on many series at once: S [R][>= max(L)] (row r holds S(0) .. S(L[r] - 1); what lies beyond is not looked at),
    L [R] the lags each row holds, means [R][m] -> (tau, ess, K, W, V), each [R], row r bit for bit what
    geyer_tau(S[r, :L[r]], m, n, means[r]) returns.  Every step is the same IEEE operation element by element; the one reduction
    whose order depends on its length, np.sum over the K kept pairs, is taken over the rows that share K (a row of a C-contiguous
    [rows][K] array is summed as the 1-D array it is).  The first row, in order, at which geyer_tau would raise, raises the same."""
    S = np.asarray(S, dtype=np.float64)
    L = np.asarray(L, dtype=np.int64).reshape(-1)
    mu = np.asarray(means, dtype=np.float64).reshape(L.size, -1)
    R, m, n = int(L.size), int(m), int(n)
    cap = ess_lag_cap(n)
    if R == 0:
        return (np.zeros(0),) * 2 + (np.zeros(0, dtype=np.int64),) + (np.zeros(0),) * 2
    wrong = np.flatnonzero((L < 2) | (L > cap)) if n >= 4 else np.arange(R)
    # (errors: row -> text; the earliest row raises at the end of the steps that can find one)
    errors = {int(r): ValueError("geyer_tau: n = %d rows and %d lags; n >= 4 and between 2 and n - 2 lags are needed" % (n, L[r]))
              for r in wrong[:1]}
    ok = np.ones(R, dtype=bool)
    ok[wrong] = False
    Lmax = int(L[ok].max()) if ok.any() else 2
    Lmax += Lmax % 2                                 # (pairs: an even width, padded below)
    Sx = np.full((R, Lmax + 1), np.nan)
    w = min(Lmax + 1, S.shape[1])
    Sx[:, :w] = S[:, :w]
    Sx[np.arange(Lmax + 1)[None, :] >= L[:, None]] = np.nan
    dm, dn = np.float64(m), np.float64(n)
    grand = np.zeros(R)
    for s in range(m):
        grand = grand + mu[:, s]
    grand = grand / dm
    d2 = np.zeros(R)
    for s in range(m):
        d = mu[:, s] - grand
        d2 = d2 + d * d
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        W = Sx[:, 0] / dm * dn / (dn - 1.0)
        V = Sx[:, 0] / dm + d2 / (dm - 1.0) if m > 1 else Sx[:, 0] / dm
        rho = 1.0 - (W[:, None] - Sx / dm) / V[:, None]
    rho[:, 0] = 1.0
    have = L // 2
    jcap = cap // 2
    P = rho[:, 0:Lmax:2] + rho[:, 1:Lmax:2]          # [R][Lmax / 2]; row r is geyer_tau's P below have[r]
    upto = np.minimum(have, jcap)
    jj = np.arange(P.shape[1])[None, :]
    fails = ~(P >= 0.0) & (jj >= 1) & (jj < upto[:, None])
    cut = fails.any(axis=1)
    K = np.where(cut, fails.argmax(axis=1), jcap).astype(np.int64)
    for r in np.flatnonzero(ok & ~cut & (have < jcap))[:1]:
        errors.setdefault(int(r), LagsNeeded("geyer_tau: the pair test is undecided after %d lags of at most %d" % (L[r], cap)))
    ok &= cut | (have >= jcap)
    for r in np.flatnonzero(ok & (2 * K <= n - 3) & (2 * K >= L))[:1]:
        errors.setdefault(int(r), LagsNeeded("geyer_tau: lag %d is needed, %d lags were given" % (2 * K[r], L[r])))
    if errors:
        raise errors[min(errors)]
    tau = np.empty(R)
    run = np.minimum.accumulate(P, axis=1)
    for Kv in np.unique(K):
        rows = np.flatnonzero(K == Kv)
        tau[rows] = -1.0 + 2.0 * np.sum(np.ascontiguousarray(run[rows, :Kv]), axis=1)
    end = 2 * K <= n - 3
    at = np.where(end, 2 * K, 0)
    last = rho[np.arange(R), np.minimum(at, Lmax)]
    with np.errstate(invalid="ignore"):
        tau = np.where(end & (last > 0.0), tau + last, tau)
        floor = 1.0 / np.log10(dm * dn)
        tau = np.where(floor > tau, floor, tau)
        tau = np.where(V > 0.0, tau, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        return tau, dm * dn / tau, K, W, V


def ess_rows_finish(out, nchains, N):
    """ess_finish on any number of columns at once through geyer_tau_rows: out [R][.] (the layout of fmcmc_rank_ess_dev's
    column) -> the namespace of ess_finish, each field with R rows and bit for bit what ess_finish(out[r]) gives.  A row that is
    still its NaN prefill (a masked group) gives NaN in every float field and 0 in the integer ones."""
    m, n = 2 * int(nchains), int(N) // 2
    cap = ess_lag_cap(n)
    kl = 2 * m + 2 + cap
    o = np.asarray(out, dtype=np.float64).reshape(-1, len(ESS_KINDS) * kl + ESS_INFO)
    R = o.shape[0]
    info = o[:, len(ESS_KINDS) * kl:]
    ess = np.full((R, 4), np.nan)
    tau = np.full((R, 4), np.nan)
    lags = np.zeros((R, 4), dtype=np.int64)
    computed = np.zeros((R, 4), dtype=np.int64)
    device_lags = np.zeros((R, 4), dtype=np.int64)
    live = np.flatnonzero(info[:, 0] == 0)           # (non-finite values: the caller raises; NaN: the row was not written)
    if live.size:
        # series (row, kind), row after row; only the lags below the largest L are gathered from the wide rows
        ol = o if live.size == R else o[live]
        piece = lambda a, b: np.stack([ol[:, kind * kl + a:kind * kl + b] for kind in range(4)], axis=1).reshape(live.size * 4, b - a)
        head = piece(0, 2 * m + 2)
        L = head[:, 2 * m].astype(np.int64)
        Lmax = int(min(max(int(L.max()), 2), cap))
        g_tau, g_ess, g_K, _W, _V = geyer_tau_rows(piece(2 * m + 2, min(2 * m + 2 + Lmax + 2, kl)), L, m, n, head[:, 0:2 * m:2])
        computed[live], device_lags[live] = L.reshape(-1, 4), head[:, 2 * m + 1].astype(np.int64).reshape(-1, 4)
        lags[live] = g_K.reshape(-1, 4)
        varies = (info[live, 5] != info[live, 6])[:, None]
        ess[live] = np.where(varies, g_ess.reshape(-1, 4), np.nan)
        tau[live] = np.where(varies, g_tau.reshape(-1, 4), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        mcse = info[:, 4] / np.sqrt(ess[:, 3])
    return SimpleNamespace(bulk=ess[:, 0], tail_q05=ess[:, 1], tail_q95=ess[:, 2], tail=np.minimum(ess[:, 1], ess[:, 2]),
                           mean=ess[:, 3], mcse_mean=mcse, tau_bulk=tau[:, 0], q05=info[:, 1].copy(), q95=info[:, 2].copy(),
                           non_finite=info[:, 0].copy(), pooled_mean=info[:, 3].copy(), pooled_sd=info[:, 4].copy(),
                           lags=lags, computed=computed, device_lags=device_lags)


def ess_groups_finish(out, chains_per_group, N):
    """The host finish of the grouped call, pure numpy: out [D][p][.] as fmcmc_rank_ess_groups_dev leaves it -> the fields of
    ess_finish with a leading [D] axis: row d is ess_finish(out[d]), to the bit (ess_rows_finish)."""
    o = np.asarray(out, dtype=np.float64)
    D, p = o.shape[0], o.shape[1]
    fin = ess_rows_finish(o.reshape(D * p, -1), chains_per_group, N)
    return SimpleNamespace(**{f: getattr(fin, f).reshape((D, p) + getattr(fin, f).shape[1:]) for f in ESS_FIELDS})


def _ess_row(fin, i):
    """dataset i of ess_groups_finish as the namespace ess_finish gives"""
    return SimpleNamespace(**{f: getattr(fin, f)[i] for f in ESS_FIELDS})


class EssDiagBatch(list):
    """ess() of an McmcBatch: a list of D EssDiag, one per dataset (what ess(ans[d]) returns), with the stacked arrays bulk,
    tail, tail_q05, tail_q95, mean, mcse_mean, tau_bulk, q05, q95, each [D][p], and lags [D][p][4]."""
    fields = ("bulk", "tail", "tail_q05", "tail_q95", "mean", "mcse_mean", "tau_bulk", "q05", "q95", "lags")

    def __init__(self, diags):
        super().__init__(diags)
        for name in self.fields:
            setattr(self, name, np.stack([getattr(r, name) for r in self]) if len(self) else np.zeros((0, 0)))

    def __repr__(self):
        return "<EssDiagBatch ndatasets=%d nvar=%d>" % (len(self), self.bulk.shape[1])


def ess_batch(ans, autoburnin=False, cols=None):
    """ess(ans[d]) for every dataset d of an McmcBatch from ONE grouped call (fmcmc_rank_ess_groups_dev) and one copy back: the
    same `out` bit for bit, and a host finish that equals ess_finish to the bit.  On a ragged result (MCMC_batch(stop_each = ...))
    each dataset has its own rows (its own autoburnin window) and iteration labels, with one call per distinct row count.  A row
    count with fewer than 8 rows, or at which a dataset's pooled values do not fit the grouped call (rank_groups_fit), is served
    dataset by dataset."""
    import torch
    from .convergence import _window
    from .mcmc import McmcBatch
    if not isinstance(ans, McmcBatch):
        raise TypeError("ess_batch() expects an McmcBatch (the result of MCMC_batch)")
    _single_process()
    full, D, Cm = ans.history, ans.nmodels, ans.nchains
    diags = [None] * D
    for nr, sel, mask in _batch_calls(ans):
        iters = full.iters[:nr]
        row0, N = _window(iters) if autoburnin else (0, nr)
        if N < 8 or not rank_groups_fit(Cm, N):           # (too few rows: the single form's text)
            for d in sel:
                try:
                    diags[d] = ess(ans[int(d)], autoburnin, cols)
                except ValueError as e:
                    raise ValueError("dataset %d: %s" % (d, e)) from None
            continue
        active = None if mask is None else torch.as_tensor(mask).to(full._samples.device)
        out, _work, cs = enqueue_rank_ess_groups(full, D, Cm, row0, N, cols, active)
        if mask is not None:                              # (only the rows of the datasets of this call are copied back)
            out = out[torch.as_tensor(sel).to(out.device)]
        fin = ess_groups_finish(out.cpu().numpy(), Cm, N)
        names, start, end = _names(full, cs), int(iters[row0]), int(iters[-1])
        for i, d in enumerate(sel):
            try:
                _raise_non_finite(fin.non_finite[i][None, :], cs, "rank")
            except ValueError as e:
                raise ValueError("dataset %d: %s" % (d, e)) from None
            diags[d] = EssDiag(_ess_row(fin, i), Cm, N, names, start, end)
    return EssDiagBatch(diags)


# ------------------------------------------------------------------------------------------------ WAIC
WAIC_POINT = ("elpd_waic", "p_waic", "lppd", "mean")           # the columns of `pointwise`, in the order of fmcmc_waic_dev's `point`
WAIC_TOTAL = ("elpd_waic", "p_waic", "lppd", "waic", "se_elpd", "se_p", "se_lppd", "n_high", "bad_draws", "bad_points")
WAIC_HIGH = 0.4                                                 # loo's warning threshold for p_waic_i
WAIC_PART_ROWS, WAIC_MAX_PARTS, WAIC_MAX_PARTS_SMALL, WAIC_SMALL_N = 512, 64, 256, 1024   # csrc/diag_waic.hpp


def waic_parts(nchains, N, n):
    """(units a part, parts) of fmcmc_waic_dev's split of the draws (include/fmcmc_amd.h): a unit is one tile of 16 rows of one
    chain, chain after chain."""
    U = int(nchains) * ((int(N) + 15) // 16)
    cap = WAIC_MAX_PARTS_SMALL if n <= WAIC_SMALL_N else WAIC_MAX_PARTS
    upp = max(WAIC_PART_ROWS // 16, -(-U // cap))
    return upp, -(-U // upp)


def _waic_model(model):
    """a closed-form family or a PointwiseFun, as it is; anything else has no pointwise form"""
    from .models import LogPosterior, PointwiseFun
    if not isinstance(model, (LogPosterior, PointwiseFun)):
        raise TypeError("waic() and loo() need one of the closed-form families (gaussian_linreg, logistic, iid_normal) or a "
                        "pointwise_fun(fn, n, k): a %s returns the summed log-posterior and has no pointwise form; give the "
                        "log-likelihood of every observation as a pointwise_fun." % type(model).__name__)
    return model


def _pointwise_loglik(model, th, dtype):
    """fn of a PointwiseFun on CPU tensors: l [S][n] in `dtype` (fn itself computes in float64)"""
    import torch
    t = torch.as_tensor(np.ascontiguousarray(th, dtype=np.float64))
    l = model.fn(t)
    if not torch.is_tensor(l) or l.dtype != torch.float64 or tuple(l.shape) != (t.shape[0], model.n) or l.device != t.device:
        raise ValueError("pointwise_fun: fn(theta) must return a float64 tensor of shape [%d, %d] on %s; got %s"
                         % (t.shape[0], model.n, t.device, _describe_tensor(l)))
    return l.detach().numpy().astype(dtype)


def _describe_tensor(t):
    import torch
    return ("%s %s on %s" % (t.dtype, tuple(t.shape), t.device)) if torch.is_tensor(t) else type(t).__name__


def waic_loglik(model, draws, dtype=np.float64):
    """The pointwise log-likelihood l [S][n] of the definition for draws [S][k], in `dtype`: the likelihood
    alone, without the prior_div term and without the guard.  A PointwiseFun is evaluated by its fn on CPU tensors."""
    from .models import PointwiseFun
    model = _waic_model(model)
    th = np.asarray(draws, dtype=dtype)
    if th.ndim != 2 or th.shape[1] != model.k:
        raise ValueError("draws must be [S][%d] for this %s; got shape %s"
                         % (model.k, "model" if isinstance(model, PointwiseFun) else "family", th.shape))
    if isinstance(model, PointwiseFun):
        return _pointwise_loglik(model, th, dtype)
    ic, p, n = int(model.intercept), model.p, int(model.y.shape[0])
    y = model.y.astype(dtype)
    eta = np.zeros((th.shape[0], n), dtype=dtype)
    if model.family == abi.FAM_IID_NORMAL:
        eta = eta + th[:, :1]
        sigma = th[:, 1]
    else:
        if ic:
            eta = eta + th[:, :1]
        if p:
            eta = eta + th[:, ic:ic + p] @ model.X.astype(dtype).T
        sigma = th[:, ic + p] if model.family == abi.FAM_GAUSSIAN_LINREG else None
    with np.errstate(all="ignore"):
        if model.family == abi.FAM_LOGISTIC:
            t = np.where(y[None, :] != 0, eta, -eta)
            return np.where(t < 0, t, dtype(0)) - np.log1p(np.exp(-np.abs(t)))
        r = y[None, :] - eta
        half_log_2pi = np.log(np.sqrt(dtype(2) * np.arccos(dtype(-1))))
        return -(np.log(sigma) + half_log_2pi)[:, None] - dtype(0.5) * r * r / (sigma * sigma)[:, None]


def _bad_draws(model, th):
    """the draws with a parameter that is not finite, or (Gaussian families) a sigma that is not > 0"""
    from .models import PointwiseFun
    bad = ~np.isfinite(th).all(axis=1)
    if not isinstance(model, PointwiseFun) and model.family != abi.FAM_LOGISTIC:
        bad |= ~(th[:, -1] > 0)
    return int(bad.sum())


def _se(v):
    """sqrt(n var(v)) with divisor n - 1 (NaN for n = 1), in the dtype of v"""
    n = v.shape[-1]
    with np.errstate(all="ignore"):
        d = v - v.mean(axis=-1, keepdims=True)
        return np.sqrt(n * ((d * d).sum(axis=-1) / v.dtype.type(n - 1)))


def waic_host_matrix(l, dtype=np.float64, bad_draws=0):
    """waic_host on the matrix l [S][n] of pointwise log-likelihoods itself, in `dtype`: what waic_host computes once it has
    evaluated the model.  bad_draws is passed through (a matrix knows nothing of the draws)."""
    l = np.ascontiguousarray(np.asarray(l, dtype=dtype).T)           # [n][S]: the sums run along a row (numpy: pairwise)
    if l.ndim != 2:
        raise ValueError("l must be a matrix [S][n]; got shape %s" % (l.T.shape,))
    S = l.shape[1]
    if S < 2:
        raise ValueError("WAIC needs at least 2 draws; got %d" % S)
    with np.errstate(all="ignore"):
        top = l.max(axis=1)
        lppd = top + np.log(np.exp(l - top[:, None]).sum(axis=1) / dtype(S))
        mean = l[:, 0] + (l - l[:, :1]).sum(axis=1) / dtype(S)       # (shifted by the first draw: equal draws give it back)
        p_waic = ((l - mean[:, None]) ** 2).sum(axis=1) / dtype(S - 1)
    point = np.stack([lppd - p_waic, p_waic, lppd, mean], axis=1)
    tot = point[:, :3].sum(axis=0)
    se = [_se(point[:, q]) for q in range(3)]
    return SimpleNamespace(pointwise=point, elpd_waic=tot[0], p_waic=tot[1], lppd=tot[2], waic=dtype(-2) * tot[0], se_elpd=se[0],
                           se_p=se[1], se_lppd=se[2], n_high=int((point[:, 1] > WAIC_HIGH).sum()), bad_draws=int(bad_draws),
                           bad_points=int((~np.isfinite(point).all(axis=1)).sum()))


def waic_host(model, draws, dtype=np.float64):
    """The plain numpy restatement of waic() on draws [S][k]: the CPU reference and the documentation of the definition.  With
    dtype = np.longdouble it is the truth the tests hold the device to.  Returns a namespace with pointwise [n][4] = {elpd_i,
    p_waic_i, lppd_i, mean_i} and the totals elpd_waic, p_waic, lppd, waic, se_elpd, se_p, se_lppd, n_high, bad_draws,
    bad_points, all in `dtype`.  model: a family, or a PointwiseFun whose fn runs on CPU tensors; it is waic_loglik followed by
    waic_host_matrix."""
    model = _waic_model(model)
    th = np.asarray(draws, dtype=dtype)
    return waic_host_matrix(waic_loglik(model, th, dtype), dtype, _bad_draws(model, th))


class WaicResult:
    """waic() of a result: elpd_waic, p_waic, lppd, waic = -2 elpd_waic, their standard errors se_elpd, se_p, se_lppd (se_waic =
    2 se_elpd), n_high = the observations with p_waic_i > 0.4, and pointwise [n][4] = {elpd_i, p_waic_i, lppd_i, mean_i} (numpy;
    pointwise_dev is the device tensor it was copied from, or None).  ndraws = the S draws, nobs = the n observations."""

    def __init__(self, pointwise, total, ndraws, pointwise_dev=None):
        self.pointwise = np.asarray(pointwise, dtype=np.float64).reshape(-1, 4)
        self.pointwise_dev = pointwise_dev
        total = np.asarray(total, dtype=np.float64).reshape(10)
        for name, v in zip(WAIC_TOTAL[:7], total):
            setattr(self, name, float(v))
        self.se_waic = 2.0 * self.se_elpd
        self.n_high, self.bad_draws, self.bad_points = (int(v) if np.isfinite(v) else -1 for v in total[7:])
        self.ndraws, self.nobs = int(ndraws), int(self.pointwise.shape[0])

    def __str__(self):
        rows = [("elpd_waic", self.elpd_waic, self.se_elpd), ("p_waic", self.p_waic, self.se_p), ("waic", self.waic, self.se_waic)]
        out = ["", "Computed from %d by %d log-likelihood matrix" % (self.ndraws, self.nobs), "",
               "%-9s %9s %6s" % ("", "Estimate", "SE")]
        out += ["%-9s %9.1f %6.1f" % r for r in rows]
        if self.n_high > 0:
            out += ["", "%d (%.1f%%) p_waic estimates greater than 0.4. We recommend trying loo instead."
                    % (self.n_high, 100.0 * self.n_high / self.nobs)]
        return "\n".join(out) + "\n"

    def __repr__(self):
        return "<WaicResult elpd_waic=%.4g p_waic=%.4g n=%d>" % (self.elpd_waic, self.p_waic, self.nobs)


class WaicBatch(list):
    """waic() of an McmcBatch: a list of D WaicResult, one per dataset (what waic(ans[d], models[d]) returns), with the stacked
    arrays elpd_waic, p_waic, lppd, waic, se_elpd, se_p, se_lppd, se_waic, n_high, each [D], and pointwise [D][n][4]."""
    fields = WAIC_TOTAL[:8] + ("se_waic",)

    def __init__(self, results):
        super().__init__(results)
        for name in self.fields:
            setattr(self, name, np.array([getattr(r, name) for r in self]))
        self.pointwise = np.stack([r.pointwise for r in self]) if len(self) else np.zeros((0, 0, 4))

    def __repr__(self):
        return "<WaicBatch ndatasets=%d n=%d>" % (len(self), self.pointwise.shape[1])


def _waic_rc(rc):
    if rc != abi.OK:
        raise (NotImplementedError if rc == abi.ERR_UNSUPPORTED else ValueError if rc == abi.ERR_ARG else RuntimeError)(
            abi.last_error())


def enqueue_waic_groups(dc, dm, ngroups, chains_per_group, row0, N, active=None):
    """The one call site of fmcmc_waic_groups_dev (current torch stream): the window [row0, row0 + N) of the rows of `dc`, whose
    chains are ngroups groups of chains_per_group consecutive chains, group g on dataset g of the device model dm (a DeviceModel
    for one group, a DeviceModelBatch beyond).  active: None or an int32 device tensor [ngroups]; the rows of the groups whose
    entry is 0 keep their NaN prefill.  Returns the device tensors (point [ngroups][n][4], total [ngroups][10], work); nothing
    is synchronised."""
    import torch
    o = _open(dc, None, "score")
    ngroups, cpg = int(ngroups), int(chains_per_group)
    if ngroups < 1 or cpg < 1 or ngroups * cpg != o.Cn:
        raise ValueError("%d groups of %d chains are not the %d chains of the result" % (ngroups, cpg, o.Cn))
    if getattr(dm, "nmodels", 1) != ngroups:
        raise ValueError("%d datasets for %d groups of chains" % (getattr(dm, "nmodels", 1), ngroups))
    if dm.device != o.dev and (dm.device.index is not None or dm.device.type != o.dev.type):
        raise ValueError("the model's data are on %s, the draws on %s" % (dm.device, o.dev))
    if o.k != dm.k:
        raise ValueError("the result has k = %d parameters, the model's family has %d" % (o.k, dm.k))
    if row0 < 0 or N < 1 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    if cpg * int(N) < 2:
        raise ValueError("WAIC needs at least 2 draws; got %d" % (cpg * int(N)))
    if active is not None and (not torch.is_tensor(active) or active.dtype != torch.int32 or tuple(active.shape) != (ngroups,)
                               or not active.is_contiguous() or active.device != o.dev):
        raise ValueError("`active` must be a contiguous int32 tensor of shape [%d] on %s" % (ngroups, o.dev))
    cm = dm.c()
    point = torch.full((ngroups, dm.n, 4), float("nan"), dtype=torch.float64, device=o.dev)
    total = torch.full((ngroups, 10), float("nan"), dtype=torch.float64, device=o.dev)
    work = _doubles(o, o.L.fmcmc_waic_work_len(C.byref(cm), ngroups, cpg, int(N)))
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_waic_groups_dev(C.byref(cm), getattr(dm, "x_stride", 0), getattr(dm, "y_stride", 0), o.smp.data_ptr(),
                                       ngroups, cpg, o.k, o.cap, int(row0), int(N),
                                       active.data_ptr() if active is not None else None, work.data_ptr(), point.data_ptr(),
                                       total.data_ptr(), _stream(o.dev))
    _waic_rc(rc)
    return point, total, work


def _raise_bad_draws(total_row):
    if total_row[8] != 0:
        raise ValueError("%d draw(s) with a parameter that is not finite or a sigma that is not > 0 among the rows to score"
                         % int(total_row[8]))


def _pointwise_trampoline(model, dev, stream, view, caught):
    """model.fn as a fmcmc_pointwise_fn: the device buffers as tensors, fn under the call's stream as torch's current stream, its
    result copied into `ll`.  An exception raised in fn (or by the check of what it returned) is kept in `caught` and the
    trampoline returns non-zero: the library abandons the call (FMCMC_ERR_FUN) and the caller raises the exception itself."""
    import torch
    fn = model.fn

    def trampoline(theta_p, B, k, n, ll_p, stream_p, user):
        try:
            with torch.cuda.stream(stream):
                l = fn(view(theta_p, (B, k)))
                if not torch.is_tensor(l) or l.dtype != torch.float64 or l.device != dev or tuple(l.shape) != (B, n):
                    raise ValueError("pointwise_fun: fn(theta) must return a float64 tensor of shape [%d, %d] on %s; got %s"
                                     % (B, n, dev, _describe_tensor(l)))
                view(ll_p, (B, n)).copy_(l)
            return 0
        except BaseException as e:   # (nothing may unwind through the C frames)
            caught.append(e)
            return 1

    return abi.POINTWISE_FN(trampoline)


def enqueue_pointwise(dc, model, row0, N, block_rows=None, what="waic", want_tail=False):
    """The one call site of fmcmc_waic_fun_dev (what = "waic") and fmcmc_loo_fun_dev ("loo") on the current torch stream: the
    window [row0, row0 + N) of the rows of `dc` under the PointwiseFun `model`, in blocks of at most block_rows rows (rounded up
    to whole tiles of 16 rows; None: the library's choice).  Returns the device tensors (point [1][n][4], total [1][10], work)
    or (point [1][n][6], total [1][12], work, tail [1][n][M] or None), shaped as the grouped calls shape theirs.  The WAIC call
    only enqueues; the LOO call synchronises the stream once (include/fmcmc_amd.h)."""
    import torch
    from .engine import _Views
    o = _open(dc, None, "score")
    loo_ = what == "loo"
    n, Cn, N, row0 = model.n, o.Cn, int(N), int(row0)
    if o.k != model.k:
        raise ValueError("the result has k = %d parameters, the pointwise_fun has %d" % (o.k, model.k))
    if row0 < 0 or N < 1 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    if Cn * N < 2:
        raise ValueError("%s needs at least 2 draws; got %d" % ("LOO" if loo_ else "WAIC", Cn * N))
    br = 0 if block_rows is None else int(block_rows)
    if br < 0:
        raise ValueError("block_rows = %d: give a number of rows, or None for the library's choice" % br)
    M = loo_tail_len(Cn * N)
    if loo_ and M > LOO_MAX_TAIL:
        raise NotImplementedError("%d draws ask for a tail of %d; supported are tails up to %d" % (Cn * N, M, LOO_MAX_TAIL))
    nwork = (o.L.fmcmc_loo_fun_work_len if loo_ else o.L.fmcmc_waic_fun_work_len)(n, Cn, N, br)
    if nwork < 1:
        raise ValueError(abi.last_error())
    width = 6 if loo_ else 4
    point = torch.full((1, n, width), float("nan"), dtype=torch.float64, device=o.dev)
    total = torch.full((1, 12 if loo_ else 10), float("nan"), dtype=torch.float64, device=o.dev)
    tail = torch.full((1, n, M), float("nan"), dtype=torch.float64, device=o.dev) if loo_ and want_tail else None
    work = _doubles(o, nwork)
    stream = torch.cuda.current_stream(o.dev)
    caught = []
    cb = _pointwise_trampoline(model, o.dev, stream, _Views(o.dev), caught)
    head = (cb, None, n, o.smp.data_ptr(), Cn, o.k, o.cap, row0, N, br, work.data_ptr(), point.data_ptr())
    with torch.cuda.device(o.dev):
        if loo_:
            rc = o.L.fmcmc_loo_fun_dev(*head, tail.data_ptr() if tail is not None else None, total.data_ptr(),
                                       C.c_void_p(stream.cuda_stream))
        else:
            rc = o.L.fmcmc_waic_fun_dev(*head, total.data_ptr(), C.c_void_p(stream.cuda_stream))
    if caught:
        raise caught[0]
    _waic_rc(rc)
    return (point, total, work, tail) if loo_ else (point, total, work)


def _raise_bad_fun_draws(count):
    if count != 0:
        raise ValueError("%d draw(s) with a parameter that is not finite among the rows to score" % int(count))


def _no_batch_pointwise(x, model, what):
    from .mcmc import McmcBatch
    from .models import PointwiseFun
    if isinstance(x, McmcBatch) and isinstance(model, PointwiseFun):
        raise TypeError("%s() of an McmcBatch needs the model_batch the datasets came from: a pointwise_fun scores one dataset "
                        "(the grouped form is not implemented); call %s(ans[d], ...) per dataset." % (what, what))


def waic(x, model, autoburnin=False, block_rows=None):
    """The widely applicable information criterion (Watanabe 2010; Gelman, Hwang and Vehtari 2014; loo::waic) of a result under
    the model it was sampled from, or another one of the same parameters: x a DeviceChains (read in place), an Mcmc or a McmcList
    (uploaded first), model a gaussian_linreg / logistic / iid_normal object or a pointwise_fun (a user-defined model: its fn is
    called on blocks of at most block_rows draws; None: the library's choice); an McmcBatch with a model_batch gives a
    WaicBatch, one WaicResult per dataset from one grouped call (waic_batch).  With `autoburnin` the rows are coda's window (the
    second half).  The S x n matrix of pointwise log-likelihoods is never formed: the device turns tiles of it into four running
    numbers per observation (csrc/diag_waic.hpp, csrc/diag_pointwise.hpp)."""
    from .convergence import _window
    from .mcmc import McmcBatch
    from .models import PointwiseFun
    _no_batch_pointwise(x, model, "waic")
    if isinstance(x, McmcBatch):
        return waic_batch(x, model, autoburnin)
    model = _waic_model(model)
    if block_rows is not None and not isinstance(model, PointwiseFun):
        raise ValueError("block_rows applies to a pointwise_fun only: a family is evaluated inside the kernel")
    dc = _as_device_chains(x)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    Cn = int(dc._samples.shape[0])
    if isinstance(model, PointwiseFun):
        point, total, _work = enqueue_pointwise(dc, model, row0, N, block_rows, "waic")
        th = total[0].cpu().numpy()
        _raise_bad_fun_draws(th[8])
    else:
        point, total, _work = enqueue_waic_groups(dc, model.device_model(dc._samples.device), 1, Cn, row0, N)
        th = total[0].cpu().numpy()
        _raise_bad_draws(th)
    return WaicResult(point[0].cpu().numpy(), th, Cn * N, point[0])


def waic_batch(ans, models, autoburnin=False):
    """waic(ans[d], models[d]) for every dataset d of an McmcBatch from ONE grouped call (fmcmc_waic_groups_dev): the same bits.
    On a ragged result (MCMC_batch(stop_each = ...)) each dataset has its own rows, with one call per distinct row count."""
    import torch
    from .convergence import _window
    from .mcmc import McmcBatch
    from .models import ModelBatch
    if not isinstance(ans, McmcBatch):
        raise TypeError("waic_batch() expects an McmcBatch (the result of MCMC_batch)")
    if not isinstance(models, ModelBatch):
        raise TypeError("waic_batch() needs the model_batch the datasets came from (a %s has no pointwise form per dataset)"
                        % type(models).__name__)
    _single_process()
    full, D, Cm = ans.history, ans.nmodels, ans.nchains
    if models.nmodels != D:
        raise ValueError("%d datasets in the model batch, %d in the result" % (models.nmodels, D))
    dm = models.device_model(full._samples.device)
    out = [None] * D
    for nr, sel, mask in _batch_calls(ans):
        row0, N = _window(full.iters[:nr]) if autoburnin else (0, nr)
        active = None if mask is None else torch.as_tensor(mask).to(full._samples.device)
        point, total, _work = enqueue_waic_groups(full, dm, D, Cm, row0, N, active)
        ph, th = point.cpu().numpy(), total.cpu().numpy()
        for d in sel:
            try:
                _raise_bad_draws(th[d])
            except ValueError as e:
                raise ValueError("dataset %d: %s" % (d, e)) from None
            out[d] = WaicResult(ph[d], th[d], Cm * N, point[d])
    return WaicBatch(out)


def waic_compare(a, b):
    """The difference of two models on the same observations, as loo::loo_compare forms it: elpd_diff = sum_i (elpd_i of a - elpd_i
    of b) and se_diff = sqrt(n var of the pointwise differences) (divisor n - 1), from the pointwise arrays in longdouble.  Two
    WaicResult (or waic_host results) give two numbers, two WaicBatch arrays [D]."""
    pa, pb = (np.asarray(r.pointwise, dtype=np.longdouble) for r in (a, b))
    if pa.ndim != pb.ndim or pa.shape[:-2] != pb.shape[:-2]:
        raise ValueError("waic_compare: a single result against a batch, or batches of different sizes")
    if pa.shape[-2] != pb.shape[-2]:
        raise ValueError("waic_compare: the models score different numbers of observations (%d and %d)"
                         % (pa.shape[-2], pb.shape[-2]))
    d = pa[..., 0] - pb[..., 0]
    diff, se = d.sum(axis=-1), _se(d)
    if d.ndim == 1:
        return SimpleNamespace(elpd_diff=float(diff), se_diff=float(se))
    return SimpleNamespace(elpd_diff=diff.astype(np.float64), se_diff=se.astype(np.float64))


# ------------------------------------------------------------------------------------------------ PSIS-LOO
LOO_POINT = ("elpd_loo", "p_loo", "lppd", "pareto_k", "n_eff", "cutoff")     # the columns of `pointwise` (fmcmc_loo_dev's `point`)
LOO_TOTAL = ("elpd_loo", "p_loo", "lppd", "looic", "se_elpd", "se_p", "se_lppd", "n_k_bad", "n_k_very_bad", "max_k", "bad_draws",
             "bad_points")
LOO_MAX_TAIL = 16384                                             # csrc/diag_loo.hpp: LOO_MAX_M


def loo_tail_len(S):
    """M = ceil(min(0.2 S, 3 sqrt(S))) in integers: loo's tail length with r_eff = 1 (fmcmc_loo_tail_len)."""
    import math
    S = int(S)
    b = math.isqrt(9 * S)
    return min((S + 4) // 5, b + (b * b < 9 * S))


def loo_k_threshold(S):
    """tau(S) = min(1 - 1 / log10 S, 0.7): the Pareto k above which the estimate of an observation is not to be trusted"""
    import math
    return min(1.0 - 1.0 / math.log10(S), 0.7)


def loo_plan(nchains, N, n):
    """fmcmc_loo_plan as a namespace: M, ustride / sub_units / sub_rows (the subsample: every ustride-th unit of 16 rows), rank
    (the threshold's rank in the subsample), target (the draws expected above it), cap (an observation's buffer) and forms (the
    tail lengths at which a kernel or its launch changes form).  A function of (nchains, N, n) alone; no device needed."""
    out = (C.c_int64 * abi.LOO_PLAN_LEN)()
    _waic_rc(abi.lib().fmcmc_loo_plan(int(nchains), int(N), int(n), out))
    v = [int(x) for x in out]
    return SimpleNamespace(M=v[0], ustride=v[1], sub_units=v[2], sub_rows=v[3], rank=v[4], target=v[5], cap=v[6],
                           forms=tuple(v[8:8 + v[7]]))


def loo_gpdfit(x):
    """Zhang and Stephens' (2009) fit of the generalised Pareto distribution to x (ascending, >= 0) as loo::gpdfit forms it, with
    loo's weakly informative prior on k: (k, sigma), in the dtype of x."""
    import math
    x = np.asarray(x)
    dt = x.dtype.type
    M = x.shape[0]
    G = 30 + math.isqrt(M)
    with np.errstate(all="ignore"):
        xstar = x[(M + 2) // 4 - 1]
        j = np.arange(1, G + 1).astype(x.dtype)
        theta = dt(1) / x[-1] + (dt(1) - np.sqrt(dt(G) / (j - dt(0.5)))) / (dt(3) * xstar)
        kappa = np.log1p(-theta[:, None] * x[None, :]).sum(axis=1) / dt(M)
        ell = dt(M) * (np.log(-theta / kappa) - kappa - dt(1))
        w = np.exp(ell - ell.max())
        that = (theta * w).sum() / w.sum()
        kraw = np.log1p(-that * x).sum() / dt(M)
        return (dt(M) * kraw + dt(5)) / dt(M + 10), -kraw / that


def _loo_smooth(tl, cut):
    """The tail tl (log ratios after the shift, ascending, [M]) and the cutoff: (k, the smoothed tail), INTEGRATION.md 2.2 step
    2 and 3; k = +Inf and the tail as it is where nothing is smoothed."""
    dt = tl.dtype.type
    M = tl.shape[0]
    inf = dt(np.inf)
    if M < 5 or tl[-1] - tl[0] < dt(np.finfo(np.float64).eps) / dt(100):
        return inf, tl
    with np.errstate(all="ignore"):
        ecut = np.exp(cut)
        k, sigma = loo_gpdfit(np.exp(tl) - ecut)
        if not np.isfinite(k):
            return inf, tl
        p = (np.arange(1, M + 1).astype(tl.dtype) - dt(0.5)) / dt(M)
        return k, np.log(ecut + sigma * np.expm1(-k * np.log1p(-p)) / k)


def loo_host_matrix(l, dtype=np.float64, bad_draws=0):
    """loo_host on the matrix l [S][n] of pointwise log-likelihoods itself, in `dtype`: what loo_host computes once it has
    evaluated the model.  bad_draws is passed through (a matrix knows nothing of the draws)."""
    l = np.ascontiguousarray(np.asarray(l, dtype=dtype).T)           # [n][S]
    if l.ndim != 2:
        raise ValueError("l must be a matrix [S][n]; got shape %s" % (l.T.shape,))
    n, S = l.shape
    if S < 2:
        raise ValueError("LOO needs at least 2 draws; got %d" % S)
    M = loo_tail_len(S)
    point = np.zeros((n, 6), dtype=dtype)
    tail, smoothed = np.zeros((n, M), dtype=dtype), np.zeros((n, M), dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(n):
            r = np.partition(-l[i], S - M - 1)                       # [S - M - 1] the cutoff, behind it the tail
            rest, cutoff, tl = r[:S - M - 1], r[S - M - 1], np.sort(r[S - M:])
            R = tl[-1]
            tail[i] = tl
            k, sm = _loo_smooth(tl - R, cutoff - R)
            smoothed[i] = sm
            lw = np.concatenate([rest - R, [cutoff - R], np.minimum(sm, dtype(0))])
            ls = -np.concatenate([rest, [cutoff], tl])               # the l of the same draws
            a = ls + lw
            num = a.max() + np.log(np.exp(a - a.max()).sum())
            den = np.exp(lw).sum()                                   # (max lw = 0 up to the smoothing)
            top = l[i].max()
            lppd = top + np.log(np.exp(l[i] - top).sum() / dtype(S))
            elpd = num - np.log(den)
            point[i] = (elpd, lppd - elpd, lppd, k, den * den / np.exp(dtype(2) * lw).sum(), cutoff)
    tot = point[:, :3].sum(axis=0)
    se = [_se(point[:, q]) for q in range(3)]
    tau = loo_k_threshold(S)
    kk = point[:, 3]
    okp = np.isfinite(point[:, [0, 1, 2, 4]]).all(axis=1) & ~np.isnan(kk)
    return SimpleNamespace(pointwise=point, pareto_k=kk, n_eff=point[:, 4], tail=tail, smoothed=smoothed, elpd_loo=tot[0],
                           p_loo=tot[1], lppd=tot[2], looic=dtype(-2) * tot[0], se_elpd=se[0], se_p=se[1], se_lppd=se[2],
                           n_k_bad=int((kk > tau).sum()), n_k_very_bad=int((kk > 1).sum()), max_k=kk.max(),
                           bad_draws=int(bad_draws), bad_points=int((~okp).sum()), tail_len=M, k_threshold=tau)


def loo_host(model, draws, dtype=np.float64):
    """The plain numpy restatement of loo() on draws [S][k]: the CPU reference and the executable form of the definition
    (INTEGRATION.md 2.2).  With dtype = np.longdouble it is the truth the tests hold the device to.  Returns a namespace with
    pointwise [n][6] = {elpd_loo_i, p_loo_i, lppd_i, pareto_k_i, n_eff_i, cutoff_i}, pareto_k, n_eff, tail [n][M] (the M largest
    -l, ascending, before the smoothing), smoothed [n][M] (the tail's log weights after the shift and the smoothing, before the
    cap at 0), the totals of LOO_TOTAL and tail_len, k_threshold.  model: a family, or a PointwiseFun whose fn runs on CPU
    tensors; it is waic_loglik followed by loo_host_matrix."""
    model = _waic_model(model)
    th = np.asarray(draws, dtype=dtype)
    return loo_host_matrix(waic_loglik(model, th, dtype), dtype, _bad_draws(model, th))


class LooResult:
    """loo() of a result: elpd_loo, p_loo, lppd, looic = -2 elpd_loo, their standard errors se_elpd, se_p, se_lppd (se_looic =
    2 se_elpd), pareto_k [n] and n_eff [n], n_k_bad / n_k_very_bad = the observations with k > k_threshold = min(1 - 1 / log10 S,
    0.7) / with k > 1, max_k, and pointwise [n][6] = {elpd_i, p_loo_i, lppd_i, pareto_k_i, n_eff_i, cutoff_i} (numpy;
    pointwise_dev is the device tensor it was copied from, or None).  ndraws = the S draws, nobs = the n observations."""

    def __init__(self, pointwise, total, ndraws, pointwise_dev=None):
        self.pointwise = np.asarray(pointwise, dtype=np.float64).reshape(-1, 6)
        self.pointwise_dev = pointwise_dev
        total = np.asarray(total, dtype=np.float64).reshape(12)
        for name, v in zip(LOO_TOTAL[:7], total):
            setattr(self, name, float(v))
        self.se_looic = 2.0 * self.se_elpd
        self.max_k = float(total[9])
        self.n_k_bad, self.n_k_very_bad, self.bad_draws, self.bad_points = (
            int(v) if np.isfinite(v) else -1 for v in (total[7], total[8], total[10], total[11]))
        self.pareto_k, self.n_eff = self.pointwise[:, 3], self.pointwise[:, 4]
        self.ndraws, self.nobs = int(ndraws), int(self.pointwise.shape[0])
        self.tail_len, self.k_threshold = loo_tail_len(self.ndraws), loo_k_threshold(self.ndraws)

    def k_table(self):
        """loo's table: (label, count, percent, least n_eff) for k <= threshold (good), (threshold, 1] (bad), > 1 (very bad)"""
        k, tau = self.pareto_k, self.k_threshold
        rows = []
        for label, sel in (("(-Inf, %.2g]   (good)" % tau, k <= tau), ("(%.2g, 1]   (bad)" % tau, (k > tau) & (k <= 1)),
                           ("(1, Inf)   (very bad)", k > 1)):
            c = int(sel.sum())
            rows.append((label, c, 100.0 * c / max(1, self.nobs), float(self.n_eff[sel].min()) if c else float("nan")))
        return rows

    def __str__(self):
        rows = [("elpd_loo", self.elpd_loo, self.se_elpd), ("p_loo", self.p_loo, self.se_p), ("looic", self.looic, self.se_looic)]
        out = ["", "Computed from %d by %d log-likelihood matrix" % (self.ndraws, self.nobs), "",
               "%-9s %9s %6s" % ("", "Estimate", "SE")]
        out += ["%-9s %9.1f %6.1f" % r for r in rows]
        out += ["------", "MCSE and r_eff are not computed (r_eff = 1).", ""]
        if self.n_k_bad == 0:
            out += ["All Pareto k estimates are good (k < %.2g)." % self.k_threshold]
        else:
            out += ["Pareto k diagnostic values:", "%-26s %6s %6s %10s" % ("", "Count", "Pct.", "Min. n_eff")]
            out += ["%-26s %6d %5.1f%% %10s" % (lab, c, pct, "<NA>" if c == 0 else "%.0f" % ne)
                    for lab, c, pct, ne in self.k_table()]
        return "\n".join(out) + "\n"

    def __repr__(self):
        return "<LooResult elpd_loo=%.4g p_loo=%.4g max_k=%.3g n=%d>" % (self.elpd_loo, self.p_loo, self.max_k, self.nobs)


class LooBatch(list):
    """loo() of an McmcBatch: a list of D LooResult, one per dataset (what loo(ans[d], models[d]) returns), with the stacked
    arrays elpd_loo, p_loo, lppd, looic, se_elpd, se_p, se_lppd, se_looic, n_k_bad, n_k_very_bad, max_k, each [D], and
    pointwise [D][n][6], pareto_k [D][n], n_eff [D][n]."""
    fields = LOO_TOTAL[:10] + ("se_looic",)

    def __init__(self, results):
        super().__init__(results)
        for name in self.fields:
            setattr(self, name, np.array([getattr(r, name) for r in self]))
        self.pointwise = np.stack([r.pointwise for r in self]) if len(self) else np.zeros((0, 0, 6))
        self.pareto_k, self.n_eff = self.pointwise[..., 3], self.pointwise[..., 4]

    def __repr__(self):
        return "<LooBatch ndatasets=%d n=%d>" % (len(self), self.pointwise.shape[1])


def enqueue_loo_groups(dc, dm, ngroups, chains_per_group, row0, N, active=None, want_tail=False):
    """The one call site of fmcmc_loo_groups_dev (current torch stream), with the arguments of enqueue_waic_groups.  Returns the
    device tensors (point [ngroups][n][6], total [ngroups][12], work, tail [ngroups][n][M] or None); nothing is synchronised."""
    import torch
    o = _open(dc, None, "score")
    ngroups, cpg = int(ngroups), int(chains_per_group)
    if ngroups < 1 or cpg < 1 or ngroups * cpg != o.Cn:
        raise ValueError("%d groups of %d chains are not the %d chains of the result" % (ngroups, cpg, o.Cn))
    if getattr(dm, "nmodels", 1) != ngroups:
        raise ValueError("%d datasets for %d groups of chains" % (getattr(dm, "nmodels", 1), ngroups))
    if dm.device != o.dev and (dm.device.index is not None or dm.device.type != o.dev.type):
        raise ValueError("the model's data are on %s, the draws on %s" % (dm.device, o.dev))
    if o.k != dm.k:
        raise ValueError("the result has k = %d parameters, the model's family has %d" % (o.k, dm.k))
    if row0 < 0 or N < 1 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    if cpg * int(N) < 2:
        raise ValueError("LOO needs at least 2 draws; got %d" % (cpg * int(N)))
    M = loo_tail_len(cpg * int(N))
    if M > LOO_MAX_TAIL:
        raise NotImplementedError("%d draws ask for a tail of %d; supported are tails up to %d" % (cpg * int(N), M, LOO_MAX_TAIL))
    if active is not None and (not torch.is_tensor(active) or active.dtype != torch.int32 or tuple(active.shape) != (ngroups,)
                               or not active.is_contiguous() or active.device != o.dev):
        raise ValueError("`active` must be a contiguous int32 tensor of shape [%d] on %s" % (ngroups, o.dev))
    cm = dm.c()
    point = torch.full((ngroups, dm.n, 6), float("nan"), dtype=torch.float64, device=o.dev)
    total = torch.full((ngroups, 12), float("nan"), dtype=torch.float64, device=o.dev)
    tail = torch.full((ngroups, dm.n, M), float("nan"), dtype=torch.float64, device=o.dev) if want_tail else None
    work = _doubles(o, o.L.fmcmc_loo_work_len(C.byref(cm), ngroups, cpg, int(N)))
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_loo_groups_dev(C.byref(cm), getattr(dm, "x_stride", 0), getattr(dm, "y_stride", 0), o.smp.data_ptr(),
                                      ngroups, cpg, o.k, o.cap, int(row0), int(N),
                                      active.data_ptr() if active is not None else None, work.data_ptr(), point.data_ptr(),
                                      tail.data_ptr() if tail is not None else None, total.data_ptr(), _stream(o.dev))
    _waic_rc(rc)
    return point, total, work, tail


def _raise_bad_loo_draws(total_row):
    if total_row[10] != 0:
        raise ValueError("%d draw(s) with a parameter that is not finite or a sigma that is not > 0 among the rows to score"
                         % int(total_row[10]))


def loo(x, model, autoburnin=False, block_rows=None):
    """Pareto-smoothed importance-sampling leave-one-out cross-validation (Vehtari, Gelman and Gabry 2017; loo::loo with r_eff =
    1) of a result under the model it was sampled from, or another one of the same parameters, with the Pareto k of every
    observation: the arguments of waic(); a LooResult, or a LooBatch for an McmcBatch with a model_batch.  The S x n matrix of
    pointwise log-likelihoods is never formed: the device selects the M largest importance ratios of every observation exactly
    (csrc/diag_loo.hpp; a pointwise_fun: csrc/diag_pointwise.hpp, its fn sweeps a subsample and then all draws once, and nine
    more times where an observation needs the exact fallback)."""
    from .convergence import _window
    from .mcmc import McmcBatch
    from .models import PointwiseFun
    _no_batch_pointwise(x, model, "loo")
    if isinstance(x, McmcBatch):
        return loo_batch(x, model, autoburnin)
    model = _waic_model(model)
    if block_rows is not None and not isinstance(model, PointwiseFun):
        raise ValueError("block_rows applies to a pointwise_fun only: a family is evaluated inside the kernel")
    dc = _as_device_chains(x)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    Cn = int(dc._samples.shape[0])
    if isinstance(model, PointwiseFun):
        point, total, _work, _tail = enqueue_pointwise(dc, model, row0, N, block_rows, "loo")
        th = total[0].cpu().numpy()
        _raise_bad_fun_draws(th[10])
    else:
        point, total, _work, _tail = enqueue_loo_groups(dc, model.device_model(dc._samples.device), 1, Cn, row0, N)
        th = total[0].cpu().numpy()
        _raise_bad_loo_draws(th)
    return LooResult(point[0].cpu().numpy(), th, Cn * N, point[0])


def loo_batch(ans, models, autoburnin=False):
    """loo(ans[d], models[d]) for every dataset d of an McmcBatch from ONE grouped call (fmcmc_loo_groups_dev): the same bits.
    On a ragged result (MCMC_batch(stop_each = ...)) each dataset has its own rows, with one call per distinct row count."""
    import torch
    from .convergence import _window
    from .mcmc import McmcBatch
    from .models import ModelBatch
    if not isinstance(ans, McmcBatch):
        raise TypeError("loo_batch() expects an McmcBatch (the result of MCMC_batch)")
    if not isinstance(models, ModelBatch):
        raise TypeError("loo_batch() needs the model_batch the datasets came from (a %s has no pointwise form per dataset)"
                        % type(models).__name__)
    _single_process()
    full, D, Cm = ans.history, ans.nmodels, ans.nchains
    if models.nmodels != D:
        raise ValueError("%d datasets in the model batch, %d in the result" % (models.nmodels, D))
    dm = models.device_model(full._samples.device)
    out = [None] * D
    for nr, sel, mask in _batch_calls(ans):
        row0, N = _window(full.iters[:nr]) if autoburnin else (0, nr)
        active = None if mask is None else torch.as_tensor(mask).to(full._samples.device)
        point, total, _work, _tail = enqueue_loo_groups(full, dm, D, Cm, row0, N, active)
        ph, th = point.cpu().numpy(), total.cpu().numpy()
        for d in sel:
            try:
                _raise_bad_loo_draws(th[d])
            except ValueError as e:
                raise ValueError("dataset %d: %s" % (d, e)) from None
            out[d] = LooResult(ph[d], th[d], Cm * N, point[d])
    return LooBatch(out)


def loo_compare(a, b):
    """The difference of two models on the same observations, as loo::loo_compare forms it: the arithmetic of waic_compare on
    column 0 (elpd_loo_i) of the pointwise arrays.  Two LooResult (or loo_host results) give two numbers, two LooBatch arrays [D]."""
    return waic_compare(a, b)


# ------------------------------------------------------------------------------------------------ predict()
PREDICT_KINDS = {"linpred": abi.PREDICT_LINPRED, "epred": abi.PREDICT_EPRED}
PREDICT_POINT = ("mean", "sd", "sd_pred", "mean_eta")           # the head of a row of `point`, before the quantiles


def _predict_model(model):
    """a gaussian_linreg or logistic object, as it is; anything else cannot be predicted from"""
    from .models import BatchedFun, LogPosterior, PointwiseFun
    if isinstance(model, (BatchedFun, PointwiseFun)):
        raise TypeError("predict() needs one of the regression families (gaussian_linreg, logistic): a %s says nothing of a new "
                        "point, and a prediction callback is not implemented." % type(model).__name__)
    if not isinstance(model, LogPosterior):
        raise TypeError("predict() needs a gaussian_linreg or logistic object; got a %s" % type(model).__name__)
    if model.family == abi.FAM_IID_NORMAL:
        raise ValueError("iid_normal has no covariates to predict at: its mean and sd are columns of summary().")
    return model


def _predict_probs(probs):
    probs = tuple(float(q) for q in np.atleast_1d(np.asarray(() if probs is None else probs, dtype=np.float64)))
    if len(probs) > abi.SUMMARY_MAX_PROBS:
        raise ValueError("at most %d probs per call; got %d" % (abi.SUMMARY_MAX_PROBS, len(probs)))
    for q in probs:
        if not (np.isfinite(q) and 0.0 <= q <= 1.0):
            raise ValueError("probs must lie in [0, 1]; got %r" % q)
    return probs


def _predict_kind(kind):
    if kind not in PREDICT_KINDS:
        raise ValueError("kind must be \"linpred\" or \"epred\"; got %r" % (kind,))
    return kind


def _predict_newdata(model, newdata):
    """newdata as a float64 matrix [m][p], the model's own X for None"""
    if newdata is None:
        return model.X if model.p else np.zeros((int(model.y.shape[0]), 0))
    Xn = np.asarray(newdata, dtype=np.float64)
    if Xn.ndim == 1:
        Xn = Xn[:, None] if model.p == 1 else Xn[None, :]
    if Xn.ndim != 2 or Xn.shape[1] != model.p:
        raise ValueError("newdata has %s column(s) but the model has p = %d covariates"
                         % (Xn.shape[1] if Xn.ndim == 2 else "shape %s, not" % (Xn.shape,), model.p))
    if Xn.shape[0] < 1:
        raise ValueError("newdata has no rows")
    return Xn


def _expit(eta):
    """1 / (1 + exp(-eta)) in the branch form of the device: exp of a non-positive argument only"""
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(eta))
        return np.where(eta >= 0, 1 / (1 + e), e / (1 + e))


def predict_host(model, draws, newdata=None, probs=(0.025, 0.5, 0.975), kind="epred", dtype=np.float64):
    """The plain numpy restatement of predict() on draws [S][k]: the CPU reference and the documentation of the definition
    (INTEGRATION.md §2.2).  With dtype = np.longdouble it is the truth the tests hold the device to.  Returns a namespace with
    mean, sd, sd_pred (None for the logistic family), mean_eta, quantiles [m][nprobs], point [m][4 + nprobs] (the device's
    layout), eta [S][m], ndraws and bad_draws, all in `dtype`."""
    model, kind, probs = _predict_model(model), _predict_kind(kind), _predict_probs(probs)
    Xn = _predict_newdata(model, newdata).astype(dtype)
    th = np.asarray(draws, dtype=dtype)
    if th.ndim != 2 or th.shape[1] != model.k:
        raise ValueError("draws must be [S][%d] for this family; got shape %s" % (model.k, th.shape))
    S, m = th.shape[0], Xn.shape[0]
    if S < 2:
        raise ValueError("a prediction needs at least 2 draws; got %d" % S)
    ic, p = int(model.intercept), model.p
    gauss = model.family == abi.FAM_GAUSSIAN_LINREG
    eta = np.zeros((S, m), dtype=dtype)
    if ic:
        eta = eta + th[:, :1]
    if p:
        eta = eta + th[:, ic:ic + p] @ Xn.T
    sig = not gauss and kind == "epred"
    q = _expit(eta) if sig else eta

    def moments(v):
        with np.errstate(all="ignore"):
            mean = v[0] + (v - v[:1]).sum(axis=0) / dtype(S)       # (shifted by the first draw: equal draws give it back)
            return mean, ((v - mean[None, :]) ** 2).sum(axis=0) / dtype(S - 1)

    mean, var = moments(q)
    mean_eta, var_eta = moments(eta) if sig else (mean, var)
    with np.errstate(all="ignore"):
        sd = np.sqrt(var)
        sd_pred = np.sqrt(var_eta + (th[:, -1] ** 2).sum() / dtype(S)) if gauss else None
    quant = np.zeros((m, len(probs)), dtype=dtype)
    if probs:
        srt = np.sort(eta, axis=0)
        index, lo, hi = type7_ranks(S, probs)
        os_ = np.stack([srt[lo - 1].T, srt[hi - 1].T], axis=-1)     # [m][nprobs][2]
        if sig:
            os_ = _expit(os_)
        if dtype is np.float64:
            quant = type7_quantiles(os_, S, probs)
        else:                                                        # type7_quantiles' rule in `dtype`
            h = (index - lo).astype(dtype)
            with np.errstate(invalid="ignore", over="ignore"):
                mixed = (1 - h) * os_[..., 0] + h * os_[..., 1]
            quant = np.where((index > lo) & (os_[..., 1] != os_[..., 0]), mixed, os_[..., 0])
    third = sd_pred if gauss else np.full(m, np.nan, dtype=dtype)
    point = np.concatenate([np.stack([mean, sd, third, mean_eta], axis=1), quant], axis=1)
    return SimpleNamespace(mean=mean, sd=sd, sd_pred=sd_pred, mean_eta=mean_eta, quantiles=quant, point=point, eta=eta, probs=probs,
                           kind=kind, ndraws=S, bad_draws=_bad_draws(model, th))


class PredictResult:
    """predict() of a result: per point mean and sd of the fitted value (kind "epred": E[y | x], "linpred": the linear predictor),
    sd_pred = the sd of the posterior predictive of a new y at the point (Gaussian family; None for the logistic one), quantiles
    [m][nprobs] at probs (the credible band), mean_eta; ndraws = the S draws, npoints = m.  point_dev is the device tensor
    [m][4 + nprobs] = {mean, sd, sd_pred, mean of eta, quantiles} they were copied from."""

    def __init__(self, point, probs, kind, ndraws, gauss, point_dev=None):
        self.probs = tuple(float(q) for q in probs)
        point = np.asarray(point, dtype=np.float64).reshape(-1, 4 + len(self.probs))
        self.mean, self.sd, self.mean_eta = point[:, 0].copy(), point[:, 1].copy(), point[:, 3].copy()
        self.sd_pred = point[:, 2].copy() if gauss else None
        self.quantiles = point[:, 4:].copy()
        self.kind, self.ndraws, self.npoints, self.point_dev = kind, int(ndraws), int(point.shape[0]), point_dev

    quantile_names = property(lambda self: ["%g%%" % (100.0 * q) for q in self.probs])

    def __str__(self):
        m = self.npoints
        rows = np.arange(m) if m <= 20 else np.concatenate([np.arange(10), np.arange(m - 10, m)])
        cols, names = [self.mean, self.sd], ["Mean", "SD"]
        if self.sd_pred is not None:
            cols.append(self.sd_pred)
            names.append("SD pred")
        matrix = np.concatenate([np.stack(cols, axis=1), self.quantiles], axis=1)[rows]
        table = _fmt_table(["[%d]" % (i + 1) for i in rows], names + self.quantile_names, matrix).split("\n")
        if m > 20:
            table.insert(11, "...")
        out = ["", "Prediction (%s) at %d point%s from %d draws" % (self.kind, m, "" if m == 1 else "s", self.ndraws), ""]
        return "\n".join(out + table) + "\n"

    def __repr__(self):
        return "<PredictResult kind=%s npoints=%d nprobs=%d>" % (self.kind, self.npoints, len(self.probs))


def enqueue_predict(dc, dm, row0, N, kind, probs):
    """The one call site of fmcmc_predict_dev (current torch stream): the window [row0, row0 + N) of the rows of `dc` at the
    points of the device model dm (its X; y is not read).  Returns the device tensors (point [m][4 + nprobs], total [4], work);
    nothing is synchronised."""
    import torch
    o = _open(dc, None, "predict from")
    if dm.device != o.dev and (dm.device.index is not None or dm.device.type != o.dev.type):
        raise ValueError("the model's data are on %s, the draws on %s" % (dm.device, o.dev))
    if o.k != dm.k:
        raise ValueError("the result has k = %d parameters, the model's family has %d" % (o.k, dm.k))
    if row0 < 0 or N < 1 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    if o.Cn * int(N) < 2:
        raise ValueError("a prediction needs at least 2 draws; got %d" % (o.Cn * int(N)))
    cm = dm.c()
    probs_h = np.ascontiguousarray(probs, dtype=np.float64)
    nwork = o.L.fmcmc_predict_work_len(C.byref(cm), o.Cn, int(N), len(probs))
    if nwork < 1:
        _waic_rc(abi.ERR_ARG)
    point = torch.full((dm.n, 4 + len(probs)), float("nan"), dtype=torch.float64, device=o.dev)
    total = torch.full((4,), float("nan"), dtype=torch.float64, device=o.dev)
    work = _doubles(o, nwork)
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_predict_dev(C.byref(cm), o.smp.data_ptr(), o.Cn, o.k, o.cap, int(row0), int(N), PREDICT_KINDS[kind],
                                   probs_h.ctypes.data_as(C.POINTER(C.c_double)), len(probs), work.data_ptr(), point.data_ptr(),
                                   total.data_ptr(), _stream(o.dev))
    _waic_rc(rc)
    return point, total, work


def predict(x, model, newdata=None, probs=(0.025, 0.5, 0.975), kind="epred", autoburnin=False):
    """What the fitted model says at a point: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first), model the
    gaussian_linreg or logistic object it was sampled from (or another one of the same parameters), newdata [m][p] the new
    covariates (None: the model's own X, the fitted values).  Per point the mean and sd of the linear predictor (kind "linpred")
    or of E[y | x] ("epred": the same for the Gaussian family, the probability for the logistic one), the type-7 quantiles at
    probs (at most 16) and, Gaussian, the sd of the posterior predictive of a new y: a PredictResult.  With `autoburnin` the rows
    are coda's window (the second half).  The S x m matrix is never formed: the device folds tiles of it and selects the exact
    order statistics (csrc/diag_predict.hpp).  An McmcBatch is taken per dataset: predict(ans[d], models[d], ...)."""
    from .convergence import _window
    from .engine import DeviceModel
    from .mcmc import McmcBatch
    if isinstance(x, McmcBatch):
        raise TypeError("predict() takes one dataset at a time (the grouped form is not implemented): call "
                        "predict(ans[d], models[d], ...) per dataset.")
    model, kind, probs = _predict_model(model), _predict_kind(kind), _predict_probs(probs)
    Xn = None if newdata is None else _predict_newdata(model, newdata)
    dc = _as_device_chains(x)
    dev = dc._samples.device
    if Xn is None:
        dm = model.device_model(dev)
    else:                                              # (the model's constructor path; the user's model object is not touched)
        dm = DeviceModel(model.family, Xn if model.p else None, np.zeros(Xn.shape[0]), model.intercept, model.guard,
                         model.prior_div, device=dev)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    Cn = int(dc._samples.shape[0])
    point, total, _work = enqueue_predict(dc, dm, row0, N, kind, probs)
    th = total.cpu().numpy()
    if th[1] != 0:
        raise ValueError("%d draw(s) with a parameter that is not finite or a sigma that is not > 0 among the rows to predict from"
                         % int(th[1]))
    return PredictResult(point.cpu().numpy(), probs, kind, Cn * N, model.family == abi.FAM_GAUSSIAN_LINREG, point)


# ------------------------------------------------------------------------------------------------ predictive()
PREDICTIVE_BATCH = 8                    # csrc/diag_predictive.hpp: PDV_BATCH
PNORM_REL = 5.73e-16                         # include/fmh_detmath.h: FMH_PNORM_REL
NDTR_REL = 8 * 2.0 ** -52               # budget of scipy.special.ndtr in predictive_host (Cephes: a few ulp in either tail)
# The rounds of predictive(): passes enqueued before `total` is read (the one synchronisation of a round).  predictive_host on the
# families of tests/predictive_cases.py: a near-normal posterior finishes every (point, prob) in 2 to 4 passes, so the first round
# is 4; what is left then is a hard case (chains that disagree: up to about 30 passes), and later rounds take 8 at a time.
PREDICTIVE_ROUNDS = (4, 8)
_EPS = 2.0 ** -52


def predictive_tol(nchains, N, n, probs):
    """tol(p) = c eps min(p, 1 - p) of fmcmc_predictive_dev and c itself: csrc/diag_predictive.hpp: pdv_c, the same line"""
    upp, nparts = waic_parts(nchains, N, n)
    U = int(nchains) * ((int(N) + 15) // 16)
    c = 0.5 * (4 * min(upp, U) + 3 + (nparts - 1) + 2) + 2.0 * PNORM_REL / _EPS
    pr = np.asarray(probs, dtype=np.float64)
    return c * _EPS * np.where(pr > 0.5, 1.0 - pr, pr), c


def predictive_host_tol(S, probs):
    """the same for predictive_host's own sums: numpy adds the S rows of a column one after the other (S - 1 additions), then the
    division and the subtraction; a term carries NDTR_REL"""
    c = 0.5 * (int(S) - 1 + 2) + NDTR_REL / _EPS
    pr = np.asarray(probs, dtype=np.float64)
    return c * _EPS * np.where(pr > 0.5, 1.0 - pr, pr), c


def _predictive_model(model):
    from .models import BatchedFun, LogPosterior, PointwiseFun
    if isinstance(model, (BatchedFun, PointwiseFun)):
        raise TypeError("predictive() needs a gaussian_linreg object: a %s says nothing of a new observation, and a predictive "
                        "callback is not implemented; simulate y from to_host() draws instead." % type(model).__name__)
    if not isinstance(model, LogPosterior):
        raise TypeError("predictive() needs a gaussian_linreg object; got a %s" % type(model).__name__)
    if model.family == abi.FAM_LOGISTIC:
        raise ValueError("the predictive distribution of a logistic y is Bernoulli(q) with q the mean of E[y | x]: call "
                         "predict(x, model, newdata, kind=\"epred\") and read its mean.")
    if model.family == abi.FAM_IID_NORMAL:
        raise ValueError("iid_normal has no covariates to predict at: its mean and sd are columns of summary().")
    return model


def _predictive_probs(probs):
    probs = tuple(float(q) for q in np.atleast_1d(np.asarray(() if probs is None else probs, dtype=np.float64)))
    if len(probs) > abi.SUMMARY_MAX_PROBS:
        raise ValueError("at most %d probs per call; got %d" % (abi.SUMMARY_MAX_PROBS, len(probs)))
    for q in probs:
        if not (0.0 < q < 1.0):
            raise ValueError("probs must lie strictly inside (0, 1): the predictive distribution has no least or largest value; "
                             "got %r" % q)
    return probs


def _predictive_y(model, newdata, y, m):
    """the values to take the PIT at: the model's own y for the model's own points, else what was given (or None)"""
    if y is None:
        return np.asarray(model.y, dtype=np.float64) if newdata is None else None
    y = np.asarray(y, dtype=np.float64).ravel()
    if y.shape[0] != m:
        raise ValueError("y has %d entries but there are %d points" % (y.shape[0], m))
    return y


def predictive_cdf_host(eta, sigma, t, dtype=np.float64):
    """(F, 1 - F) [m][...] of the mixture at t [m][...]: Phi by scipy.special.ndtr per element in float64 (of u formed in
    `dtype`), the two means over the S draws in `dtype`, each a direct sum.  eta [S][m], sigma [S]."""
    from scipy.special import ndtr
    t = np.asarray(t, dtype=dtype)
    S, m = eta.shape
    lower, upper = np.zeros(t.shape, dtype=dtype), np.zeros(t.shape, dtype=dtype)
    tt = t.reshape(m, -1)
    lo2, up2 = lower.reshape(m, -1), upper.reshape(m, -1)
    rs = (1 / np.asarray(sigma, dtype=dtype))[:, None]
    with np.errstate(all="ignore"):
        for j in range(tt.shape[1]):
            u = ((tt[None, :, j] - np.asarray(eta, dtype=dtype)) * rs).astype(np.float64)
            lo2[:, j] = ndtr(u).astype(dtype).sum(axis=0) / dtype(S)
            up2[:, j] = ndtr(-u).astype(dtype).sum(axis=0) / dtype(S)
    return lower, upper


def predictive_host(model, draws, newdata=None, y=None, probs=(0.025, 0.5, 0.975), dtype=np.float64, max_passes=100):
    """The plain numpy restatement of predictive() on draws [S][k]: the executable definition, the same
    brackets, the same step rule and the same two stopping criteria as csrc/diag_predictive.hpp, with Phi from scipy.special.ndtr
    and the sums of numpy in `dtype`.  Returns a namespace: mean, sd_pred, quantiles [m][nprobs], pit, pit_upper (None without y),
    converged, passes, residual (g at the returned t), width (of the final bracket), lo0, hi0 (the bracket at pass 0), tol
    [nprobs], eta [S][m], sigma [S], ndraws, bad_draws."""
    from scipy.special import ndtr, ndtri
    model, probs = _predictive_model(model), _predictive_probs(probs)
    Xn = _predict_newdata(model, newdata).astype(dtype)
    th = np.asarray(draws, dtype=dtype)
    if th.ndim != 2 or th.shape[1] != model.k:
        raise ValueError("draws must be [S][%d] for this family; got shape %s" % (model.k, th.shape))
    S, m = th.shape[0], Xn.shape[0]
    if S < 2:
        raise ValueError("a prediction needs at least 2 draws; got %d" % S)
    yv = _predictive_y(model, newdata, y, m)
    ic, p, nprobs = int(model.intercept), model.p, len(probs)
    eta = np.zeros((S, m), dtype=dtype)
    if ic:
        eta = eta + th[:, :1]
    if p:
        eta = eta + th[:, ic:ic + p] @ Xn.T
    sigma = th[:, -1]
    with np.errstate(all="ignore"):
        rs = (1 / sigma)[:, None]
        mean = eta[0] + (eta - eta[:1]).sum(axis=0) / dtype(S)
        var = ((eta - mean[None, :]) ** 2).sum(axis=0) / dtype(S - 1)
        sd_pred = np.sqrt(var + (sigma ** 2).sum() / dtype(S))
    pr = np.asarray(probs, dtype=np.float64)
    upper_side = pr > 0.5
    side = np.where(upper_side, 1.0 - pr, pr).astype(dtype)
    tol = predictive_host_tol(S, pr)[0].astype(dtype)
    z = ndtri(pr).astype(dtype)
    mn, mx, smin, smax = eta.min(axis=0), eta.max(axis=0), sigma.min(), sigma.max()
    with np.errstate(all="ignore"):
        lo = mn[:, None] + z[None, :] * np.where(z < 0, smax, smin)[None, :]
        hi = mx[:, None] + z[None, :] * np.where(z < 0, smin, smax)[None, :]
        pad = dtype(2.0 ** -46) * (np.abs(z) * smax)[None, :] + dtype(2.0 ** -50) * np.maximum(np.abs(lo), np.abs(hi))
        lo, hi = lo - pad, hi + pad
        t = np.clip(mean[:, None] + sd_pred[:, None] * z[None, :], lo, hi)
    lo0, hi0 = lo.copy(), hi.copy()
    g = np.full((m, nprobs), np.nan, dtype=dtype)
    done = np.zeros((m, nprobs), dtype=np.int64)
    w1 = np.full((m, nprobs), np.inf, dtype=dtype)
    w2 = w1.copy()
    inv_sqrt_2pi = dtype(0.3989422804014327)
    with np.errstate(all="ignore"):
        for npass in range(1, int(max_passes) + 1):
            if nprobs == 0 or done.all():
                break
            for j in range(nprobs):
                a = np.flatnonzero(done[:, j] == 0)
                if a.size == 0:
                    continue
                u = (t[None, a, j] - eta[:, a]) * rs
                u64 = u.astype(np.float64)
                tail = ndtr(-u64 if upper_side[j] else u64).astype(dtype).sum(axis=0) / dtype(S)
                f = (np.exp(-0.5 * u * u) * inv_sqrt_2pi * rs).sum(axis=0) / dtype(S)
                gj = side[j] - tail if upper_side[j] else tail - side[j]
                gprev = g[a, j]
                g[a, j] = gj
                fin = np.abs(gj) <= tol[j]
                tj, loj, hij = t[a, j], lo[a, j], hi[a, j]
                loj = np.where(~fin & (gj < 0), tj, loj)
                hij = np.where(~fin & ~(gj < 0), tj, hij)
                w = hij - loj
                narrow = ~fin & (w <= 2 * np.spacing(np.maximum(np.abs(loj), np.abs(hij)).astype(np.float64)))
                tn = tj - gj / f
                stalled = (w > 0.5 * w2[a, j]) & (np.abs(gj) > 0.5 * np.abs(gprev))
                newton = (f > 0) & (tn > loj) & (tn < hij) & ~stalled
                tn = np.where(newton, tn, loj + 0.5 * w)
                go = ~fin & ~narrow
                lo[a, j], hi[a, j] = loj, hij
                tf = tj - gj / f                                     # (finished by |g| <= tol: the last correction is applied)
                t[a, j] = np.where(go, tn, np.where(fin & (f > 0) & (tf > loj) & (tf < hij), tf, tj))
                w2[a, j] = np.where(go, w1[a, j], w2[a, j])
                w1[a, j] = np.where(go, w, w1[a, j])
                done[a, j] = np.where(go, 0, npass)
    pit = pit_upper = None
    if yv is not None:
        pit, pit_upper = predictive_cdf_host(eta, sigma, yv.astype(dtype), dtype)
    return SimpleNamespace(mean=mean, sd_pred=sd_pred, quantiles=t, pit=pit, pit_upper=pit_upper, converged=done > 0, passes=done,
                           residual=g, width=hi - lo, lo0=lo0, hi0=hi0, tol=tol, eta=eta, sigma=sigma, probs=probs, ndraws=S,
                           bad_draws=_bad_draws(model, th), y=yv)


class PredictiveResult:
    """predictive() of a result: per point the mean and sd (sd_pred) of the posterior predictive distribution of a new observation
    y, its quantiles [m][nprobs] at probs (the prediction band), pit = F(y) and pit_upper = 1 - F(y) of the given y (None without
    y), and for every quantile converged, passes (the evaluation pass at which it finished, 0: not yet) and residual (g = F - p
    at the returned value); ndraws = the S draws, npoints = m, total_passes = the passes that were run.  point_dev is the device
    tensor [m][4 + 4 nprobs] they were copied from."""

    def __init__(self, point, probs, ndraws, y=None, total_passes=0, point_dev=None):
        self.probs = tuple(float(q) for q in probs)
        npr = len(self.probs)
        point = np.asarray(point, dtype=np.float64).reshape(-1, 4 + 4 * npr)
        self.mean, self.sd_pred = point[:, 0].copy(), point[:, 1].copy()
        self.y = None if y is None else np.asarray(y, dtype=np.float64).copy()
        self.pit = None if y is None else point[:, 2].copy()
        self.pit_upper = None if y is None else point[:, 3].copy()
        per = point[:, 4:].reshape(point.shape[0], npr, 4)
        self.quantiles, self.residual, self.width = per[:, :, 0].copy(), per[:, :, 1].copy(), per[:, :, 2].copy()
        self.passes = per[:, :, 3].astype(np.int64)
        self.converged = self.passes > 0
        self.ndraws, self.npoints, self.total_passes, self.point_dev = int(ndraws), int(point.shape[0]), int(total_passes), point_dev

    quantile_names = property(lambda self: ["%g%%" % (100.0 * q) for q in self.probs])

    def coverage(self, lower_prob, upper_prob):
        """the share of the given y inside [quantile at lower_prob, quantile at upper_prob] (both among probs)"""
        if self.y is None:
            raise ValueError("coverage() needs the y that predictive() was given")
        try:
            a, b = self.probs.index(float(lower_prob)), self.probs.index(float(upper_prob))
        except ValueError:
            raise ValueError("coverage(%r, %r): both must be among probs = %r" % (lower_prob, upper_prob, self.probs)) from None
        return float(((self.quantiles[:, a] <= self.y) & (self.y <= self.quantiles[:, b])).mean())

    def __str__(self):
        m = self.npoints
        rows = np.arange(m) if m <= 20 else np.concatenate([np.arange(10), np.arange(m - 10, m)])
        cols, names = [self.mean, self.sd_pred], ["Mean", "SD pred"]
        if self.pit is not None:
            cols.append(self.pit)
            names.append("PIT")
        matrix = np.concatenate([np.stack(cols, axis=1), self.quantiles], axis=1)[rows]
        table = _fmt_table(["[%d]" % (i + 1) for i in rows], names + self.quantile_names, matrix).split("\n")
        if m > 20:
            table.insert(11, "...")
        out = ["", "Posterior predictive of y at %d point%s from %d draws (%d pass%s)"
               % (m, "" if m == 1 else "s", self.ndraws, self.total_passes, "" if self.total_passes == 1 else "es"), ""]
        left = int((~self.converged).sum())
        tail = ["", "%d quantile(s) not converged" % left] if left else []
        return "\n".join(out + table + tail) + "\n"

    def __repr__(self):
        return "<PredictiveResult npoints=%d nprobs=%d passes=%d>" % (self.npoints, len(self.probs), self.total_passes)


def enqueue_predictive(dc, dm, row0, N, probs, npasses, with_y=True, state=None):
    """The one call site of fmcmc_predictive_dev (current torch stream): `npasses` evaluation passes on the window [row0, row0 + N)
    of the rows of `dc` at the points of the device model dm (its X; its y for the PIT when with_y).  state: the (point, total,
    work) that a previous call with the same arguments returned: the call resumes from it.  Returns the device tensors (point
    [m][4 + 4 nprobs], total [6], work); nothing is synchronised."""
    import torch
    o = _open(dc, None, "predict from")
    if dm.device != o.dev and (dm.device.index is not None or dm.device.type != o.dev.type):
        raise ValueError("the model's data are on %s, the draws on %s" % (dm.device, o.dev))
    if o.k != dm.k:
        raise ValueError("the result has k = %d parameters, the model's family has %d" % (o.k, dm.k))
    if row0 < 0 or N < 1 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    if o.Cn * int(N) < 2:
        raise ValueError("a prediction needs at least 2 draws; got %d" % (o.Cn * int(N)))
    cm = dm.c()
    if not with_y:
        cm.y = None
    probs_h = np.ascontiguousarray(probs, dtype=np.float64)
    if state is None:
        nwork = o.L.fmcmc_predictive_work_len(C.byref(cm), o.Cn, int(N), len(probs))
        if nwork < 1:
            _waic_rc(abi.ERR_ARG)
        point = torch.full((dm.n, 4 + 4 * len(probs)), float("nan"), dtype=torch.float64, device=o.dev)
        total = torch.full((6,), float("nan"), dtype=torch.float64, device=o.dev)
        work = _doubles(o, nwork)
    else:
        point, total, work = state
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_predictive_dev(C.byref(cm), o.smp.data_ptr(), o.Cn, o.k, o.cap, int(row0), int(N),
                                      probs_h.ctypes.data_as(C.POINTER(C.c_double)), len(probs), int(npasses),
                                      0 if state is None else 1, work.data_ptr(), point.data_ptr(), total.data_ptr(),
                                      _stream(o.dev))
    _waic_rc(rc)
    return point, total, work


def predictive(x, model, newdata=None, y=None, probs=(0.025, 0.5, 0.975), autoburnin=False, max_passes=100):
    """What the fitted model says of a new OBSERVATION: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first),
    model the gaussian_linreg object it was sampled from, newdata [m][p] the new covariates (None: the model's own X), y the
    values to take the probability integral transform at (None: the model's own y for the model's own points, no PIT for
    newdata).  Per point the mean and sd of the posterior predictive distribution, its quantiles at probs (at most 16, strictly
    inside (0, 1)): R's predict(lm, interval = "prediction") for the posterior, the PIT of y and, through
    PredictiveResult.coverage(), the share of y inside an interval.  The predictive distribution is the mixture of the S normals
    N(eta_si, sigma_s^2); its quantiles are found by a bracketed Newton iteration on the device (csrc/diag_predictive.hpp), the
    S x m matrix is never formed and nothing is simulated.  The passes are enqueued in rounds (PREDICTIVE_ROUNDS); after each the
    count of unfinished quantiles is read; what is unfinished after max_passes is returned with converged = False and a
    warning.  An McmcBatch is taken per dataset: predictive(ans[d], models[d], ...)."""
    import warnings
    from .convergence import _window
    from .engine import DeviceModel
    from .mcmc import McmcBatch
    if isinstance(x, McmcBatch):
        raise TypeError("predictive() takes one dataset at a time (the grouped form is not implemented): call "
                        "predictive(ans[d], models[d], ...) per dataset.")
    model, probs = _predictive_model(model), _predictive_probs(probs)
    if int(max_passes) < 1:
        raise ValueError("max_passes must be at least 1; got %r" % (max_passes,))
    Xn = None if newdata is None else _predict_newdata(model, newdata)
    m = int(model.y.shape[0]) if Xn is None else int(Xn.shape[0])
    yv = _predictive_y(model, newdata, y, m)
    dc = _as_device_chains(x)
    dev = dc._samples.device
    if Xn is None and y is None:
        dm = model.device_model(dev)
    else:                                              # (the model's constructor path; the user's model object is not touched)
        Xp = (model.X if Xn is None else Xn) if model.p else None
        dm = DeviceModel(model.family, Xp, np.zeros(m) if yv is None else yv, model.intercept, model.guard, model.prior_div,
                         device=dev)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    Cn = int(dc._samples.shape[0])
    state, used, left = None, 0, None
    while used < int(max_passes) and left != 0:
        n = min(PREDICTIVE_ROUNDS[0] if state is None else PREDICTIVE_ROUNDS[1], int(max_passes) - used)
        state = enqueue_predictive(dc, dm, row0, N, probs, n, yv is not None, state)
        used += n
        th = state[1].cpu().numpy()
        if th[1] != 0:
            raise ValueError("%d draw(s) with a parameter that is not finite or a sigma that is not > 0 among the rows to predict "
                             "from" % int(th[1]))
        left = int(th[5])
    if left:
        warnings.warn("predictive(): %d of %d quantiles had not converged after max_passes = %d evaluation passes; they are "
                      "returned with converged = False" % (left, m * len(probs), int(max_passes)), RuntimeWarning, stacklevel=2)
    return PredictiveResult(state[0].cpu().numpy(), probs, Cn * N, yv, used, state[0])


# ------------------------------------------------------------------------------------------------ loo_predictive()
LOO_PREDICTIVE_POINT = ("mean", "sd", "pit", "pareto_k", "n_eff", "elpd_loo")   # the columns of fmcmc_loo_predictive_dev's `point`


def _loo_predictive_model(model):
    """a gaussian_linreg or logistic object, as it is; anything else has no leave-one-out predictive here"""
    from .models import BatchedFun, LogPosterior, PointwiseFun
    if isinstance(model, (BatchedFun, PointwiseFun)):
        raise TypeError("loo_predictive() needs one of the regression families (gaussian_linreg, logistic): a %s says nothing of "
                        "the mean or the distribution of an observation, and a predictive callback is not implemented."
                        % type(model).__name__)
    if not isinstance(model, LogPosterior):
        raise TypeError("loo_predictive() needs a gaussian_linreg or logistic object; got a %s" % type(model).__name__)
    if model.family == abi.FAM_IID_NORMAL:
        raise ValueError("iid_normal has no covariates to predict at: its mean and sd are columns of summary().")
    return model


def _loo_run_means(rs, w, first):
    """w [S] (the weights of the ascending rs by rank) made a function of the value: over every run of equal rs that reaches
    rank `first` or beyond, the mean of w (summed in rank order); the ranks below such runs keep their w"""
    a = int(np.searchsorted(rs, rs[first], side="left"))
    seg = rs[a:]
    starts = np.flatnonzero(np.concatenate([[True], seg[1:] != seg[:-1]]))
    cnt = np.diff(np.append(starts, seg.size))
    out = w.copy()
    out[a:] = np.repeat(np.add.reduceat(w[a:], starts) / cnt.astype(w.dtype), cnt)
    return out


def loo_predictive_host_matrix(l, d, sigma=None, dtype=np.float64, y=None):
    """loo_predictive_host on the matrices themselves, in `dtype`: l [S][n] the pointwise log-likelihoods, d [S][n] = eta - y_i
    with sigma [S] (Gaussian family; y [n] is added to the mean, 0 without it), or d = eta with sigma None (logistic).
    Everything up to the smoothing is loo_host_matrix's; the weights are then a function of the VALUE of r = -l (INTEGRATION.md
    2.2): below the cutoff exp(r - R), above it the mean of exp(min(smoothed_j, 0)) over the tail ranks of that value, at it
    the mean over the whole run that straddles the boundary.  Returns a namespace: mean, sd, pit (NaN for the logistic family),
    pareto_k, n_eff, elpd_i (loo's), point [n][6] (the device's layout), sum_w [n] (the sum of the weights), weights [n][S] (in
    the order of the draws) and loo (loo_host_matrix's result)."""
    from scipy.special import ndtr
    l = np.asarray(l, dtype=dtype)
    d = np.asarray(d, dtype=dtype)
    if l.ndim != 2 or d.shape != l.shape:
        raise ValueError("l and d must be matrices [S][n] of one shape; got %s and %s" % (l.shape, d.shape))
    S, n = l.shape
    gauss = sigma is not None
    if gauss:
        sigma = np.asarray(sigma, dtype=dtype)
        if sigma.shape != (S,):
            raise ValueError("sigma must be [%d]; got shape %s" % (S, sigma.shape))
    lo = loo_host_matrix(l, dtype)
    M = lo.tail_len
    nan = dtype(np.nan)
    mean, sd, pit = (np.full(n, nan, dtype=dtype) for _ in range(3))
    sum_w, weights = np.zeros(n, dtype=dtype), np.zeros((n, S), dtype=dtype)
    with np.errstate(all="ignore"):
        for i in range(n):
            r = -l[:, i]
            order = np.argsort(r, kind="stable")
            rs = r[order]
            R = lo.tail[i, -1]
            lam = np.minimum(lo.smoothed[i], dtype(0))
            w = _loo_run_means(rs, np.exp(np.concatenate([rs[:S - M] - R, lam])), S - M)
            om = np.empty(S, dtype=dtype)
            om[order] = w
            weights[i] = om
            den = om.sum()
            sum_w[i] = den
            di = d[:, i]
            if gauss:
                e_d = (om * di).sum() / den
                e_q = (om * (di * di + sigma * sigma)).sum() / den
                mean[i] = e_d
                sd[i] = np.sqrt(e_q - e_d * e_d)
                phi = ndtr(((-di) * (1 / sigma)).astype(np.float64)).astype(dtype)
                pit[i] = (om * phi).sum() / den
            else:
                q = (om * _expit(di)).sum() / den
                mean[i] = q
                sd[i] = np.sqrt(q * (1 - q))
        if gauss and y is not None:
            mean = np.asarray(y, dtype=dtype) + mean
    bad = np.isnan(lo.pointwise[:, [0, 3, 4, 5]]).any(axis=1)
    mean[bad], sd[bad], pit[bad] = nan, nan, nan
    point = np.stack([mean, sd, pit, lo.pareto_k, lo.n_eff, lo.pointwise[:, 0]], axis=1)
    return SimpleNamespace(mean=mean, sd=sd, pit=pit, pareto_k=lo.pareto_k, n_eff=lo.n_eff, elpd_i=lo.pointwise[:, 0], point=point,
                           sum_w=sum_w, weights=weights, loo=lo, bad_points=int((~np.isfinite(point[:, :2]).all(axis=1)).sum()))


def loo_predictive_host(model, draws, dtype=np.float64):
    """The plain numpy restatement of loo_predictive() on draws [S][k]: the CPU reference and the executable form of the
    definition.  With dtype = np.longdouble it is the truth the tests hold the device to.  It is
    waic_loglik and the linear predictor followed by loo_predictive_host_matrix, whose namespace it returns, with y and
    bad_draws."""
    model = _loo_predictive_model(model)
    th = np.asarray(draws, dtype=dtype)
    l = waic_loglik(model, th, dtype)
    ic, p = int(model.intercept), model.p
    y = model.y.astype(dtype)
    eta = np.zeros(l.shape, dtype=dtype)
    if ic:
        eta = eta + th[:, :1]
    if p:
        eta = eta + th[:, ic:ic + p] @ model.X.astype(dtype).T
    if model.family == abi.FAM_GAUSSIAN_LINREG:
        out = loo_predictive_host_matrix(l, eta - y[None, :], th[:, -1], dtype, y)
    else:
        out = loo_predictive_host_matrix(l, eta, None, dtype)
    out.y, out.bad_draws = y, _bad_draws(model, th)
    out.loo.bad_draws = out.bad_draws
    return out


class LooPredictiveResult:
    """loo_predictive() of a result: per observation the leave-one-out predictive mean and sd, pit (the LOO probability integral
    transform of y_i; NaN for the logistic family, whose mean is the LOO probability of y_i = 1), pareto_k and n_eff, the y they
    are held against, residuals = y - mean, loo (the LooResult of the same call) and bad_points (the rows that are not
    finite).  family is "gaussian_linreg" or "logistic"; point_dev the device tensor [n][6] the arrays were copied from."""

    def __init__(self, point, loo_point, total, ndraws, y, family, point_dev=None):
        point = np.asarray(point, dtype=np.float64).reshape(-1, 6)
        total = np.asarray(total, dtype=np.float64).reshape(13)
        self.point, self.point_dev, self.family = point, point_dev, family
        self.mean, self.sd, self.pit = point[:, 0].copy(), point[:, 1].copy(), point[:, 2].copy()
        self.pareto_k, self.n_eff = point[:, 3].copy(), point[:, 4].copy()
        self.loo = LooResult(loo_point, total[:12], ndraws)
        self.y = np.asarray(y, dtype=np.float64).copy()
        self.residuals = self.y - self.mean
        self.bad_points = int(total[12]) if np.isfinite(total[12]) else -1
        self.ndraws, self.nobs = int(ndraws), int(point.shape[0])

    def _need_pit(self, what):
        if self.family != "gaussian_linreg":
            raise ValueError("%s needs the PIT, which the logistic family has none of: its mean is the LOO probability of y = 1"
                             % what)

    def coverage(self, prob=0.9):
        """the share of the observations inside the central LOO predictive interval of probability `prob`: those whose pit lies
        in [(1 - prob) / 2, (1 + prob) / 2]"""
        self._need_pit("coverage()")
        prob = float(prob)
        if not (0.0 < prob < 1.0):
            raise ValueError("prob must lie strictly inside (0, 1); got %r" % prob)
        return float(((self.pit >= 0.5 * (1.0 - prob)) & (self.pit <= 0.5 * (1.0 + prob))).mean())

    def pit_hist(self, bins=10):
        """(counts, edges) of the LOO-PIT values over [0, 1] in `bins` equal bins: flat under a calibrated model"""
        self._need_pit("pit_hist()")
        return np.histogram(self.pit[np.isfinite(self.pit)], bins=int(bins), range=(0.0, 1.0))

    def metrics(self):
        """Gaussian family: rmse, mae and r2 = 1 - sum (y - mean)^2 / sum (y - ybar)^2 of the LOO means; logistic: brier = the
        mean of (mean - y)^2 and accuracy = the share of y on the side of 1/2 that the LOO probability is on"""
        e = self.residuals
        if self.family == "gaussian_linreg":
            return dict(rmse=float(np.sqrt((e * e).mean())), mae=float(np.abs(e).mean()),
                        r2=float(1.0 - (e * e).sum() / ((self.y - self.y.mean()) ** 2).sum()))
        return dict(brier=float((e * e).mean()), accuracy=float(((self.mean > 0.5) == (self.y != 0)).mean()))

    def __str__(self):
        out = ["", "Leave-one-out predictive checks of %d observations from %d draws (%s)" % (self.nobs, self.ndraws, self.family),
               ""]
        m = self.metrics()
        if self.family == "gaussian_linreg":
            out += ["%-12s %9.4g" % (k, m[k]) for k in ("rmse", "mae", "r2")]
            out += ["%-12s %9.3f" % ("coverage %d%%" % round(100 * p), self.coverage(p)) for p in (0.5, 0.9)]
        else:
            out += ["%-12s %9.4g" % (k, m[k]) for k in ("brier", "accuracy")]
        out += ["------", ""]
        lo = self.loo
        if lo.n_k_bad == 0:
            out += ["All Pareto k estimates are good (k < %.2g)." % lo.k_threshold]
        else:
            out += ["%d (%.1f%%) Pareto k estimates above %.2g: the LOO expectations of these observations are not to be trusted."
                    % (lo.n_k_bad, 100.0 * lo.n_k_bad / self.nobs, lo.k_threshold)]
        if self.bad_points > 0:
            out += ["%d observation(s) without a finite result" % self.bad_points]
        return "\n".join(out) + "\n"

    def __repr__(self):
        return "<LooPredictiveResult %s n=%d max_k=%.3g>" % (self.family, self.nobs, self.loo.max_k)


def enqueue_loo_predictive(dc, dm, row0, N):
    """The one call site of fmcmc_loo_predictive_dev (current torch stream): the window [row0, row0 + N) of the rows of `dc` under
    the device model dm.  Returns the device tensors (point [n][6], loo_point [n][6], total [13], work); nothing is
    synchronised."""
    import torch
    o = _open(dc, None, "score")
    if dm.device != o.dev and (dm.device.index is not None or dm.device.type != o.dev.type):
        raise ValueError("the model's data are on %s, the draws on %s" % (dm.device, o.dev))
    if o.k != dm.k:
        raise ValueError("the result has k = %d parameters, the model's family has %d" % (o.k, dm.k))
    if row0 < 0 or N < 1 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    if o.Cn * int(N) < 2:
        raise ValueError("LOO needs at least 2 draws; got %d" % (o.Cn * int(N)))
    M = loo_tail_len(o.Cn * int(N))
    if M > LOO_MAX_TAIL:
        raise NotImplementedError("%d draws ask for a tail of %d; supported are tails up to %d" % (o.Cn * int(N), M, LOO_MAX_TAIL))
    cm = dm.c()
    nwork = o.L.fmcmc_loo_predictive_work_len(C.byref(cm), o.Cn, int(N))
    if nwork < 1:
        _waic_rc(abi.ERR_ARG)
    point = torch.full((dm.n, 6), float("nan"), dtype=torch.float64, device=o.dev)
    loo_point = torch.full((dm.n, 6), float("nan"), dtype=torch.float64, device=o.dev)
    total = torch.full((13,), float("nan"), dtype=torch.float64, device=o.dev)
    work = _doubles(o, nwork)
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_loo_predictive_dev(C.byref(cm), o.smp.data_ptr(), o.Cn, o.k, o.cap, int(row0), int(N), work.data_ptr(),
                                          point.data_ptr(), loo_point.data_ptr(), total.data_ptr(), _stream(o.dev))
    _waic_rc(rc)
    return point, loo_point, total, work


def loo_predictive(x, model, autoburnin=False):
    """Leave-one-out predictive checks (loo::E_loo, bayesplot::ppc_loo_pit) of a result under the gaussian_linreg or logistic
    model it was sampled from: x a DeviceChains (read in place), an Mcmc or a McmcList (uploaded first).  Per observation the
    LOO predictive mean and sd and, for the Gaussian family, the LOO-PIT of y_i, all expectations under the Pareto-smoothed
    importance weights of loo(), which is computed in the same call (LooPredictiveResult.loo); coverage(), pit_hist() and
    metrics() (LOO-R2, RMSE, the Brier score) are derived on the host.  The S x n matrix is never formed
    (csrc/diag_loo_predictive.hpp).  An McmcBatch is taken per dataset: loo_predictive(ans[d], models[d])."""
    from .convergence import _window
    from .mcmc import McmcBatch
    if isinstance(x, McmcBatch):
        raise TypeError("loo_predictive() takes one dataset at a time (the grouped form is not implemented): call "
                        "loo_predictive(ans[d], models[d]) per dataset.")
    model = _loo_predictive_model(model)
    dc = _as_device_chains(x)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    Cn = int(dc._samples.shape[0])
    point, loo_point, total, _work = enqueue_loo_predictive(dc, model.device_model(dc._samples.device), row0, N)
    th = total.cpu().numpy()
    _raise_bad_loo_draws(th)
    family = "gaussian_linreg" if model.family == abi.FAM_GAUSSIAN_LINREG else "logistic"
    return LooPredictiveResult(point.cpu().numpy(), loo_point.cpu().numpy(), th, Cn * N, model.y, family, point)


# ------------------------------------------------------------------------------------------------ ppc()
PPC_NAMES = ("mean_rep", "sd_rep", "min_rep", "max_rep", "chisq_rep", "chisq_obs")   # the columns of fmcmc_ppc_dev's `stats`
PPC_STATS = abi.PPC_STATS
PPC_CAP = 1e-12                         # the project's cap for fixed-order means, in the metric |got - truth| / max(1, |truth|)


def _ppc_model(model, who="ppc"):
    """a gaussian_linreg or logistic object, as it is; anything else has no replicated data here"""
    from .models import BatchedFun, LogPosterior, PointwiseFun
    if isinstance(model, (BatchedFun, PointwiseFun)):
        raise TypeError("%s() needs one of the regression families (gaussian_linreg, logistic): a %s says nothing of a new "
                        "observation, and a predictive callback is not implemented." % (who, type(model).__name__))
    if not isinstance(model, LogPosterior):
        raise TypeError("%s() needs a gaussian_linreg or logistic object; got a %s" % (who, type(model).__name__))
    if model.family == abi.FAM_IID_NORMAL:
        raise ValueError("iid_normal has no covariates to predict at: its mean and sd are columns of summary().")
    return model


def _ppc_refuse_batch(x, who, call):
    from .mcmc import McmcBatch
    if isinstance(x, McmcBatch):
        raise TypeError("%s() takes one dataset at a time (the grouped form is not implemented): call %s per dataset." % (who, call))


def ppc_observed(model):
    """T(y) for mean, sd (divisor n - 1; NaN for n = 1), min and max: longdouble, rounded to float64 [4]"""
    y = np.asarray(model.y, dtype=np.longdouble).ravel()
    n = y.size
    mean = y.sum() / n
    with np.errstate(all="ignore"):
        sd = np.sqrt(((y - mean) ** 2).sum() / np.longdouble(n - 1)) if n > 1 else np.longdouble("nan")
    return np.array([mean, sd, y.min(), y.max()], dtype=np.float64)


def ppc_variates(model, chain_ids, ids, seed=1):
    """[S][n]: the variate of every element from fmcmc_ppc_elem_host (the device's own text, built for the host): z = fmh_qnorm(u)
    for the Gaussian family, u for the logistic one.  They do not depend on eta."""
    n = int(np.asarray(model.y).shape[0])
    chain_ids, ids = np.asarray(chain_ids, dtype=np.int64).ravel(), np.asarray(ids, dtype=np.int64).ravel()
    out = np.empty((ids.size, n), dtype=np.float64)
    eta, yrep = np.zeros(n), np.empty(n)
    L = abi.lib()
    for s in range(ids.size):
        rc = L.fmcmc_ppc_elem_host(int(model.family), int(seed), int(chain_ids[s]), int(ids[s]), n, eta.ctypes.data, 1.0,
                                   yrep.ctypes.data, out[s].ctypes.data)
        _waic_rc(rc)
    return out


def _fma64(a, b, c):
    """round(a b + c) with one rounding, element by element in float64 (exact rational arithmetic where all three are finite)"""
    from fractions import Fraction
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    with np.errstate(all="ignore"):
        out = a * b + c
    fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    one = getattr(math, "fma", None) or (lambda x, y, z: float(Fraction(x) * Fraction(y) + Fraction(z)))
    flat, fa, fb, fc = out.ravel(), a.ravel(), b.ravel(), c.ravel()
    for i in np.flatnonzero(fin.ravel()):
        try:
            flat[i] = one(float(fa[i]), float(fb[i]), float(fc[i]))
        except OverflowError:
            pass                                       # (the two roundings already gave the infinity)
    return flat.reshape(out.shape)


def ppc_fold(v, crep, cobs, dtype=np.float64):
    """The device's fold of a draw over its n observations, in `dtype` (csrc/diag_ppc.hpp): v, crep, cobs [S][n] -> [S][6] = mean,
    sd, min, max, chisq_rep, chisq_obs.  Lane c = 0 .. 15 takes i = c, c + 16, ... in that order, its sums shifted by the first
    value; the lanes are merged in lane order by Chan's update.  In float64 these are the device's operations one by one."""
    v, crep, cobs = (np.asarray(a, dtype=dtype) for a in (v, crep, cobs))
    S, n = v.shape
    acc = None
    with np.errstate(all="ignore"):
        for c in range(min(16, n)):
            idx = range(c, n, 16)
            cnt = dtype(len(idx))
            K = v[:, c]
            sd, sdd, cr, co = (np.zeros(S, dtype=dtype) for _ in range(4))
            mn, mx = K.copy(), K.copy()
            for i in idx:
                x = v[:, i]
                d = x - K
                sd = sd + d
                sdd = sdd + d * d
                mn = np.where((x < mn) | np.isnan(x), x, mn)
                mx = np.where((x > mx) | np.isnan(x), x, mx)
                cr = cr + crep[:, i]
                co = co + cobs[:, i]
            mean = K + sd / cnt
            M2 = sdd - sd * sd / cnt
            M2 = np.where(M2 < 0, dtype(0), M2)
            b = (cnt, mean, M2, mn, mx, cr, co)
            if acc is None:
                acc = b
                continue
            a = acc
            oc = a[0] + b[0]
            delta = b[1] - a[1]
            acc = (oc, a[1] + delta * (b[0] / oc), (a[2] + b[2]) + delta * delta * (a[0] * b[0] / oc),
                   np.where((b[3] < a[3]) | np.isnan(b[3]), b[3], a[3]), np.where((b[4] > a[4]) | np.isnan(b[4]), b[4], a[4]),
                   a[5] + b[5], a[6] + b[6])
        sd_all = np.sqrt(acc[2] / (dtype(n) - dtype(1)))
    return np.stack([acc[1], sd_all, acc[3], acc[4], acc[5], acc[6]], axis=1)


def ppc_counts(stats, tobs):
    """[5][3] integers: per statistic (mean, sd, min, max, chisq) the draws with T_rep > T_obs, T_rep == T_obs and a value that is
    not finite on either side; for chisq T_obs is the draw's own chisq_obs"""
    out = np.zeros((5, 3), dtype=np.int64)
    for j in range(5):
        rep = stats[:, j]
        obs = stats[:, 5] if j == 4 else np.full(rep.shape, tobs[j], dtype=stats.dtype)
        nf = ~(np.isfinite(rep) & np.isfinite(obs))
        out[j] = ((~nf & (rep > obs)).sum(), (~nf & (rep == obs)).sum(), nf.sum())
    return out


def ppc_host(model, draws, chain_ids, ids, seed=1, dtype=np.float64):
    """The host restatement of ppc() on draws [S][k] with their keys chain_ids [S] and ids [S]: the executable definition
    (INTEGRATION.md §2.2).  The variates come from fmcmc_ppc_elem_host, everything else is numpy in `dtype`; with dtype =
    np.longdouble it is the truth the tests hold the device to.  Returns a namespace with stats [S][6] (PPC_NAMES), yrep [S][n],
    variate, eta, observed [4] (float64), counts [5][3], pvalue and p_gt [5], ndraws, bad_draws and the a-priori bounds, from the
    inputs alone: e [S][n] = (k' + 2) 2^-53 (|b0| + sum |x beta|), the bound of the device's eta; d = e + 2^-53 |y_rep| and dmax
    [S] its largest value over i; flips: the (s, i) of the logistic family with |u - p| <= e / 4 + 4 x 2^-53, where the device's
    y_rep may be the other value; near [5]: per statistic the draws whose |T_rep - T_obs| is within that statistic's bound (min,
    max: dmax, and 0 for the logistic family, whose y_rep are exact where no flip is possible, so that a tie there is decided;
    mean, sd: PPC_CAP max(1, |T|); chisq: that for both sides, but for the draws whose two sums have the same terms, which are
    equal in any arithmetic), by which a device count may differ."""
    model = _ppc_model(model, "ppc_host")
    th = np.asarray(draws, dtype=dtype)
    if th.ndim != 2 or th.shape[1] != model.k:
        raise ValueError("draws must be [S][%d] for this family; got shape %s" % (model.k, th.shape))
    S = th.shape[0]
    if S < 2:
        raise ValueError("a prediction needs at least 2 draws; got %d" % S)
    ic, p = int(model.intercept), model.p
    gauss = model.family == abi.FAM_GAUSSIAN_LINREG
    X = _predict_newdata(model, None).astype(dtype)
    y = np.asarray(model.y, dtype=dtype).ravel()
    n = y.size
    eta = np.zeros((S, n), dtype=dtype)
    if ic:
        eta = eta + th[:, :1]
    if p:
        eta = eta + th[:, ic:ic + p] @ X.T
    var = ppc_variates(model, chain_ids, ids, seed)
    U = np.longdouble(2.0) ** -53
    tl = np.abs(np.asarray(draws, dtype=np.longdouble))
    e = (ic + p + 2) * U * ((tl[:, :1] if ic else 0) + tl[:, ic:ic + p] @ np.abs(np.asarray(X, dtype=np.longdouble)).T
                            + np.zeros((S, n), dtype=np.longdouble))
    with np.errstate(all="ignore"):
        if gauss:
            sigma = th[:, -1:]
            z = var.astype(dtype)
            yrep = _fma64(sigma + 0 * z, z, eta) if dtype is np.float64 else sigma * z + eta   # (the device's single rounding)
            crep = z * z
            r = (y[None, :] - eta) * (dtype(1) / sigma)
            cobs = r * r
            flips = np.zeros((0, 2), dtype=np.int64)
        else:
            pr = _expit(eta)
            yrep = (var.astype(dtype) < pr).astype(dtype)
            em, ep = np.exp(-eta), np.exp(eta)
            crep = np.where(yrep != 0, em, ep)
            cobs = np.where(y[None, :] != 0, em, ep) + np.zeros_like(eta)
            flips = np.argwhere(np.abs(var.astype(np.longdouble) - pr.astype(np.longdouble)) <= e / 4 + 4 * U)
        stats = ppc_fold(yrep, crep, cobs, dtype)
        tobs = ppc_observed(model)
        counts = ppc_counts(stats, tobs.astype(dtype))
        d = e + U * np.abs(yrep.astype(np.longdouble))
        dmax = d.max(axis=1)
        sl = stats.astype(np.longdouble)
        cap = lambda v: PPC_CAP * np.maximum(1, np.abs(v))
        bounds = [cap(sl[:, 0]), cap(sl[:, 1]), dmax if gauss else 0 * dmax, dmax if gauss else 0 * dmax, cap(sl[:, 4]) + cap(sl[:, 5])]
        near = np.zeros(5, dtype=np.int64)
        for j in range(5):
            obs = sl[:, 5] if j == 4 else np.longdouble(tobs[j])
            decided = (crep == cobs).all(axis=1) if j == 4 else False      # (the same terms in the same order: equal sums)
            near[j] = int(((np.abs(sl[:, j] - obs) <= bounds[j]) & (bounds[j] > 0) & ~decided).sum())
        usable = counts[:, 2] < S
        pvalue = np.where(usable, (counts[:, 0] + counts[:, 1]) / float(S), np.nan)
        p_gt = np.where(usable, counts[:, 0] / float(S), np.nan)
    return SimpleNamespace(stats=stats, yrep=yrep, variate=var, eta=eta, observed=tobs, counts=counts, pvalue=pvalue, p_gt=p_gt,
                           ndraws=S, bad_draws=_bad_draws(model, np.asarray(draws, dtype=np.float64)), e=e, d=d, dmax=dmax,
                           flips=flips, near=near)


class PpcResult:
    """ppc() of a result: stats, a DeviceChains [C][6][N] of the replicated statistics per draw (PPC_NAMES; summary(),
    hpd_interval(), ess() and rhat() apply to it), observed = T(y) per statistic (chisq: None, it is compared per draw), pvalue =
    (gt + eq) / S' and p_gt = gt / S' per statistic, counts [5][3] = {gt, eq, not finite}, ndraws = S', bad_draws."""

    def __init__(self, stats, observed, total, family):
        total = np.asarray(total, dtype=np.float64)
        self.stats, self.family = stats, family
        self.ndraws, self.bad_draws = int(total[0]), int(total[1])
        self.counts = total[2:2 + 15].astype(np.int64).reshape(5, 3)
        self.observed = dict(zip(PPC_STATS, [float(v) for v in observed] + [None]))
        S = float(self.ndraws)
        usable = self.counts[:, 2] < self.ndraws
        self.pvalue = {s: (float((c[0] + c[1]) / S) if u else float("nan")) for s, c, u in zip(PPC_STATS, self.counts, usable)}
        self.p_gt = {s: (float(c[0] / S) if u else float("nan")) for s, c, u in zip(PPC_STATS, self.counts, usable)}

    def table(self):
        """[5][4]: T(y), the mean and sd of T(y_rep) over the draws (summary() of stats), p; chisq: the mean of chisq_obs for T(y)"""
        try:
            st = summary(self.stats, quantiles=()).statistics
        except (ValueError, NotImplementedError):            # (fewer than 3 rows a chain: no summary)
            st = np.full((6, 4), np.nan)
        obs = [self.observed[s] for s in PPC_STATS[:4]] + [st[5, 0]]
        return np.array([[obs[j], st[j, 0], st[j, 1], self.pvalue[s]] for j, s in enumerate(PPC_STATS)], dtype=np.float64)

    def __str__(self):
        out = ["", "Posterior predictive check from %d draws (%s)" % (self.ndraws, self.family), ""]
        return "\n".join(out + [_fmt_table(list(PPC_STATS), ["T(y)", "Mean T(y_rep)", "SD T(y_rep)", "p"], self.table())]) + "\n"

    def __repr__(self):
        return "<PpcResult ndraws=%d %s>" % (self.ndraws, " ".join("p(%s)=%.3g" % kv for kv in self.pvalue.items()))


def _ppc_open(dc, dm, who):
    o = _open(dc, None, who)
    if dm.device != o.dev and (dm.device.index is not None or dm.device.type != o.dev.type):
        raise ValueError("the model's data are on %s, the draws on %s" % (dm.device, o.dev))
    if o.k != dm.k:
        raise ValueError("the result has k = %d parameters, the model's family has %d" % (o.k, dm.k))
    return o


def enqueue_ppc(dc, dm, row0, N, seed, tobs):
    """The one call site of fmcmc_ppc_dev (current torch stream): the window [row0, row0 + N) of the rows of `dc` under the device
    model dm, keyed by dc.chain_base, id0 = dc.iters[row0] and id_step = dc.thin.  Returns the device tensors (stats [C][6][N],
    total [17], work); nothing is synchronised."""
    import torch
    o = _ppc_open(dc, dm, "check")
    if row0 < 0 or N < 1 or row0 + N > dc.nrows:
        raise ValueError("the window [%d, %d) is outside the %d kept rows" % (row0, row0 + N, dc.nrows))
    if o.Cn * int(N) < 2:
        raise ValueError("a prediction needs at least 2 draws; got %d" % (o.Cn * int(N)))
    cm = dm.c()
    nwork = o.L.fmcmc_ppc_work_len(C.byref(cm), o.Cn, int(N))
    if nwork < 1:
        _waic_rc(abi.ERR_ARG)
    stats = torch.full((o.Cn, len(PPC_NAMES), int(N)), float("nan"), dtype=torch.float64, device=o.dev)
    total = torch.full((2 + 15,), float("nan"), dtype=torch.float64, device=o.dev)
    work = _doubles(o, nwork)
    tobs_h = np.ascontiguousarray(tobs, dtype=np.float64)
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_ppc_dev(C.byref(cm), o.smp.data_ptr(), o.Cn, o.k, o.cap, int(row0), int(N), int(seed), int(dc.chain_base),
                               int(dc.iters[row0]), int(dc.thin), tobs_h.ctypes.data_as(C.POINTER(C.c_double)), work.data_ptr(),
                               stats.data_ptr(), total.data_ptr(), _stream(o.dev))
    _waic_rc(rc)
    return stats, total, work


def ppc(x, model, seed=1, autoburnin=False):
    """The posterior predictive check of Gelman, Meng and Stern (bayesplot::ppc_stat): x a DeviceChains (read in place), an Mcmc
    or a McmcList (uploaded first), model the gaussian_linreg or logistic object it was sampled from.  Every draw replicates the
    data once, y_rep ~ p(y | theta_s), from a Philox stream keyed by (seed, chain id, the row's iteration label, i), so the same
    draw gives the same y_rep wherever it sits; per draw the mean, sd, min and max of y_rep and the chi-square discrepancy of
    y_rep and of y at the draw's own theta; p = the share of draws with T(y_rep) >= T(y).  The S x n matrix is never stored
    (csrc/diag_ppc.hpp).  Returns a PpcResult; its `stats` are a DeviceChains, a derived chain.  With `autoburnin` the rows are
    coda's window (the second half).  An McmcBatch is taken per dataset: ppc(ans[d], models[d])."""
    from .convergence import _window
    from .mcmc import DeviceChains
    _ppc_refuse_batch(x, "ppc", "ppc(ans[d], models[d])")
    model = _ppc_model(model)
    dc = _as_device_chains(x)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    observed = ppc_observed(model)
    stats, total, _work = enqueue_ppc(dc, model.device_model(dc._samples.device), row0, N, seed, observed)
    th = total.cpu().numpy()
    if th[1] != 0:
        raise ValueError("%d draw(s) with a parameter that is not finite or a sigma that is not > 0 among the rows to predict from"
                         % int(th[1]))
    derived = DeviceChains(stats, None, None, np.asarray(dc.iters)[row0:row0 + N], dc.thin, list(PPC_NAMES), dc.chain_base,
                           dc.nchains_total)
    return PpcResult(derived, observed, th, "gaussian_linreg" if model.family == abi.FAM_GAUSSIAN_LINREG else "logistic")


def posterior_predict_selection(nchains, N, ndraws):
    """The draws posterior_predict() takes of the nchains N draws of a window, chain after chain: draw j = 0 .. ndraws - 1 is the
    flat index floor(j nchains N / ndraws), i.e. (chain, row) = divmod(index, N); ndraws is cut to nchains N."""
    total = int(nchains) * int(N)
    nd = min(int(ndraws), total)
    if nd < 1:
        raise ValueError("ndraws = %d: at least one draw is needed" % int(ndraws))
    flat = (np.arange(nd, dtype=np.int64) * total) // nd
    return flat // int(N), flat % int(N)


def enqueue_ppc_yrep(dc, dm, seed, sel_chain, sel_row):
    """The one call site of fmcmc_ppc_yrep_dev (current torch stream): the replicated data sets of the draws (sel_chain[i], row
    sel_row[i] of dc's rows), a device tensor [nsel][n]; nothing is synchronised."""
    import torch
    o = _ppc_open(dc, dm, "replicate")
    sc, sr = np.ascontiguousarray(sel_chain, dtype=np.int64), np.ascontiguousarray(sel_row, dtype=np.int64)
    if sc.shape != sr.shape or sc.ndim != 1 or sc.size < 1:
        raise ValueError("sel_chain and sel_row must be two vectors of one length >= 1")
    if sr.min() < 0 or sr.max() >= dc.nrows:
        raise ValueError("a selected row is outside the %d kept rows" % dc.nrows)
    yrep = torch.full((int(sc.size), dm.n), float("nan"), dtype=torch.float64, device=o.dev)
    cm = dm.c()
    i64 = C.POINTER(C.c_int64)
    with torch.cuda.device(o.dev):
        rc = o.L.fmcmc_ppc_yrep_dev(C.byref(cm), o.smp.data_ptr(), o.Cn, o.k, o.cap, int(seed), int(dc.chain_base),
                                    int(dc.iters[0]), int(dc.thin), sc.ctypes.data_as(i64), sr.ctypes.data_as(i64), int(sc.size),
                                    yrep.data_ptr(), _stream(o.dev))
    _waic_rc(rc)
    return yrep


def posterior_predict(x, model, ndraws=50, seed=1, autoburnin=False):
    """Replicated data sets themselves, a device tensor [ndraws][n] (what bayesplot::ppc_dens_overlay plots): the y_rep of ndraws
    draws evenly spaced over the window, chain after chain (posterior_predict_selection), bit for bit what ppc() with the same
    seed folded for those draws.  At most 65535 draws a call."""
    from .convergence import _window
    _ppc_refuse_batch(x, "posterior_predict", "posterior_predict(ans[d], models[d])")
    model = _ppc_model(model, "posterior_predict")
    dc = _as_device_chains(x)
    row0, N = _window(dc.iters) if autoburnin else (0, int(dc.nrows))
    chain, row = posterior_predict_selection(int(dc._samples.shape[0]), N, ndraws)
    return enqueue_ppc_yrep(dc, model.device_model(dc._samples.device), seed, chain, row0 + row)
