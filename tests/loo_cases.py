"""The inputs, the raw device call and the comparison that tests/test_loo_host.py, tests/test_gpu_loo.py and
tests/test_gpu_batch_loo.py share: a plain module on top of tests/waic_cases.py (make_case, loglik_error, metric).  torch is
imported where it is used, so collecting needs no GPU.

The tolerances against loo_host(longdouble), in the metric |got - truth| / max(1, |truth|):
1e-12 for elpd_loo, p_loo, lppd, their totals and standard errors (WAIC's cap), 1e-10 for pareto_k, n_eff and max_k; the tail
and the cutoff within emax_i = the largest a-priori evaluation error of l for the observation (order statistics are 1-Lipschitz
in the sup norm); an infinite k on both sides or on none."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import fmcmc_amd as F
from fmcmc_amd import _abi as abi
from fmcmc_amd.summary import loo_plan, loo_tail_len, waic_loglik

import waic_cases as W

LD = np.longdouble
CAP_ELPD = 1e-12
CAP_K = 1e-10
GUARD = W.GUARD
TOTALS = ("elpd_loo", "p_loo", "lppd", "looic", "se_elpd", "se_p", "se_lppd")


def big_case(family, n, p, C_, N, seed, row0=3):
    """waic_cases.make_case without its limit of 5000 draws: samples [C][k][S] around a truth (coefficients + 0.1 N(0, 1), sigma
    times exp(0.1 N(0, 1))), the window at row0"""
    rng = np.random.default_rng(seed)
    ic = 1
    X = rng.uniform(-2.0, 2.0, (n, p))
    coef = rng.standard_normal(ic + p) / np.sqrt(max(1, p))
    sigma = rng.uniform(0.5, 2.0)
    eta = coef[0] + (X @ coef[ic:] if p else np.zeros(n))
    y = eta + sigma * rng.standard_normal(n)
    truth = np.concatenate([coef, [sigma]])
    model = F.iid_normal(y) if family == "iid" else F.gaussian_linreg(X if p else None, y, intercept=True)
    k = truth.size
    S = row0 + N + 2
    S += 1 - S % 2
    samples = np.ascontiguousarray(truth[None, :, None] + 0.1 * rng.standard_normal((C_, k, S)))
    # sigma with a relative spread: among 10^7 draws an absolute one comes within 10^-3 of zero, -l of such a draw lies thousands
    # above the rest, the ratios of the tail underflow in float64 and nothing is smoothed there, which longdouble does not share
    samples[:, -1, :] = sigma * np.exp(samples[:, -1, :] - sigma)
    return finish_case(SimpleNamespace(family=family, n=n, p=p, ic=ic, C=C_, N=N, k=k, S=S, row0=row0, model=model,
                                       samples=samples, name="%s n%d p%d C%d N%d" % (family, n, p, C_, N)))


def finish_case(case):
    """(re)derive draws [C N][k] from case.samples"""
    case.draws = np.ascontiguousarray(case.samples[:, :, case.row0:case.row0 + case.N].transpose(0, 2, 1).reshape(case.C * case.N,
                                                                                                                  case.k))
    return case


def sub_rows_mask(P, C_, N):
    """[C][N] bool: the rows of the subsample of the plan"""
    T = (N + 15) // 16
    m = np.zeros((C_, N), dtype=bool)
    for u in range(0, C_ * T, P.ustride):
        c, t = divmod(u, T)
        m[c, 16 * t:16 * t + 16] = True
    return m


def device_loo(case, samples=None, row0=None, run=None, model=None, want_tail=True, want_state=False):
    """One fmcmc_loo_dev call on the case's samples (or `samples` [C][k][S] with the window at row0): NaN-filled buffers GUARD
    doubles longer than documented, which must stay NaN.  Returns (point [n][6], tail [n][M], total [12]) as numpy, and with
    want_state the observations' state words [n][8] (int64) behind them.  run: as in tests/diag_dev.py: device_call."""
    import torch
    x = case.samples if samples is None else samples
    row0 = case.row0 if row0 is None else row0
    Cn, k, Srows = x.shape
    dm = (model or case.model).device_model("cuda")
    cm = dm.c()
    L = abi.lib()
    M = loo_tail_len(Cn * case.N)
    assert M == L.fmcmc_loo_tail_len(Cn * case.N)
    xd = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    lens = (L.fmcmc_loo_work_len(C.byref(cm), 1, Cn, case.N), dm.n * 6, dm.n * M, 12)
    assert lens[0] > 0, abi.last_error()
    bufs = [torch.full((int(v) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for v in lens]
    call = lambda stream: L.fmcmc_loo_dev(C.byref(cm), xd.data_ptr(), Cn, k, Srows, row0, case.N, bufs[0].data_ptr(),
                                          bufs[1].data_ptr(), bufs[2].data_ptr() if want_tail else None, bufs[3].data_ptr(), stream)
    rc = call(None) if run is None else run([xd], bufs, call)
    assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs[1:]]
    assert all(np.isnan(h[int(v):]).all() for h, v in zip(host, lens[1:]))      # nothing past the documented lengths
    assert torch.isnan(bufs[0][lens[0]:]).all()
    out = (host[0][:lens[1]].reshape(dm.n, 6), host[1][:lens[2]].reshape(dm.n, M), host[2][:12])
    if want_state:
        off = L.fmcmc_loo_state_offset(C.byref(cm), 1, Cn, case.N)
        assert off >= 0
        state = bufs[0][off:off + 8 * dm.n].cpu().numpy().view(np.int64).reshape(dm.n, 8)
        return out + (state,)
    return out


def truth_total(t):
    return np.array([getattr(t, f) for f in TOTALS], dtype=LD)


def emax_of(case):
    """the largest a-priori evaluation error of l per observation (waic_cases.loglik_error)"""
    l = waic_loglik(case.model, case.draws, LD)
    return W.loglik_error(case, l).max(axis=0)


def assert_matches(point, tail, total, truth, emax, what=""):
    """The device's (or float64 host's) results against loo_host(longdouble) within the tolerances of the module docstring.
    Prints the figures before it asserts; returns (largest error of elpd / p_loo / lppd and totals, largest of k / n_eff)."""
    n = truth.pointwise.shape[0]
    tp = truth.pointwise
    e3 = W.metric(point[:, :3], tp[:, :3])
    kinf = np.isinf(tp[:, 3].astype(np.float64))
    got_inf = np.isinf(np.asarray(point[:, 3], dtype=np.float64))
    fin = ~kinf
    ek = W.metric(point[fin, 3], tp[fin, 3]) if fin.any() else np.zeros(1)
    en = W.metric(point[:, 4], tp[:, 4])
    et = W.metric(np.asarray(total)[:7], truth_total(truth))
    ok_t = np.ones(7, dtype=bool) if n > 1 else np.array([1, 1, 1, 1, 0, 0, 0], dtype=bool)
    d_tail = np.abs(np.asarray(tail, dtype=LD) - truth.tail).max(axis=1) if truth.tail.shape[1] else np.zeros(n)
    d_cut = np.abs(np.asarray(point[:, 5], dtype=LD) - tp[:, 5])
    big = max(float(e3.max()), float(et[ok_t].max()))
    bigk = max(float(ek.max()), float(en.max()))
    print("%s: elpd/p/lppd and totals %.3g, k / n_eff %.3g, tail / emax %.3g, cutoff / emax %.3g, inf k %d"
          % (what, big, bigk, float((d_tail / emax).max()), float((d_cut / emax).max()), int(kinf.sum())))
    assert np.array_equal(kinf, got_inf), (what, "an infinite k on one side only")
    assert (e3 <= CAP_ELPD).all(), (what, float(e3.max()))
    assert (et[ok_t] <= CAP_ELPD).all(), (what, et)
    assert (ek <= CAP_K).all() and (en <= CAP_K).all(), (what, float(ek.max()), float(en.max()))
    assert (d_tail <= emax).all() and (d_cut <= emax).all(), (what, float((d_tail / emax).max()), float((d_cut / emax).max()))
    if len(total) > 7:
        tk = tp[:, 3].astype(np.float64)
        tolk = CAP_K * np.maximum(1.0, np.abs(np.where(kinf, 1.0, tk)))
        near_tau = int((fin & (np.abs(tk - truth.k_threshold) <= tolk)).sum())
        near_one = int((fin & (np.abs(tk - 1.0) <= tolk)).sum())
        assert abs(int(total[7]) - truth.n_k_bad) <= near_tau and abs(int(total[8]) - truth.n_k_very_bad) <= near_one, what
        if kinf.any():
            assert np.isinf(total[9])
        else:
            assert W.metric(total[9], truth.max_k) <= CAP_K
    if n == 1:
        assert np.isnan(np.asarray(total, dtype=np.float64)[4:7]).all()
    return big, bigk


def check_case(case, what=None, **kw):
    """device_loo of the case against the truth; the tail equals a sort of the device's own r exactly where the host's float64 l
    is the device's (not asserted here) -- what is asserted: it is ascending and within emax of the truth's order statistics."""
    got = device_loo(case, **kw)
    point, tail, total = got[:3]
    truth = F.loo_host(case.model, case.draws, LD)
    errs = assert_matches(point, tail, total, truth, emax_of(case), what or case.name)
    assert (np.diff(tail, axis=1) >= 0).all()
    assert total[10] == 0 and total[11] == 0
    return got, truth, errs


bits = W.bits
plan = loo_plan
