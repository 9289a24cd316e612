"""The inputs, the raw device call and the a-priori error bound that tests/test_waic_host.py, tests/test_gpu_waic.py and
tests/test_gpu_batch_waic.py share.  A plain module next to tests/diag_dev.py; torch is imported where it is used, so collecting
needs no GPU.

The input family: X uniform on [-2, 2]; coefficients (the intercept included) N(0, 1) / sqrt(max(1, p)); sigma uniform on
[0.5, 2]; y from the model; draws = truth + 0.1 N(0, 1); at most 5000 draws.

The bound (waic_bound) follows the order of operations of csrc/diag_waic.hpp; DESIGN.md §5.10 has the derivation.  It is computed
from the inputs alone, in longdouble, and never from what the device or waic_host return."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import fmcmc_amd as F
from fmcmc_amd import _abi as abi
from fmcmc_amd.summary import waic_loglik, waic_parts

LD = np.longdouble
U = LD(2.0) ** -53                   # unit roundoff of float64
CAP = 1e-12                          # what the bound itself may not exceed, in the metric |got - truth| / max(1, |truth|)
GUARD = 64
ROW0 = 5


def gamma(m):
    m = LD(m)
    return m * U / (1 - m * U)


def make_case(family, n, p, intercept, C_, N, seed, row0=ROW0):
    """A model of `family` ("linreg", "logistic", "iid") and samples [C][k][S] around its truth: S odd, the window [row0, row0 + N)
    holds the draws, the rows around it other values.  draws [C N][k]: the window, chain after chain."""
    rng = np.random.default_rng(seed)
    ic = 1 if family == "iid" else int(bool(intercept))
    X = rng.uniform(-2.0, 2.0, (n, p))
    coef = rng.standard_normal(ic + p) / np.sqrt(max(1, p))
    sigma = rng.uniform(0.5, 2.0)
    eta = (coef[0] if ic else 0.0) + (X @ coef[ic:] if p else np.zeros(n))
    if family == "logistic":
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        truth = coef
        model = F.logistic(X, y, intercept=bool(ic))
    else:
        y = eta + sigma * rng.standard_normal(n)
        truth = np.concatenate([coef, [sigma]])
        model = F.iid_normal(y) if family == "iid" else F.gaussian_linreg(X if p else None, y, intercept=bool(ic))
    k = truth.size
    assert k == model.k and C_ * N <= 5000
    S = row0 + N + 2
    S += 1 - S % 2
    samples = truth[None, :, None] + 0.1 * rng.standard_normal((C_, k, S))
    if family != "logistic":
        assert (samples[:, -1, :] > 0).all()
    samples = np.ascontiguousarray(samples)
    draws = np.ascontiguousarray(samples[:, :, row0:row0 + N].transpose(0, 2, 1).reshape(C_ * N, k))
    return SimpleNamespace(family=family, n=n, p=p, ic=ic, C=C_, N=N, k=k, S=S, row0=row0, model=model, samples=samples, draws=draws,
                           name="%s n%d p%d ic%d C%d N%d" % (family, n, p, ic, C_, N))


def metric(got, truth):
    truth = np.asarray(truth, dtype=LD)
    return np.abs(np.asarray(got, dtype=LD) - truth) / np.maximum(1, np.abs(truth))


def _lanes(C_, N, n):
    """The draws of every lane group of fmcmc_waic_dev in the order it meets them: a list over the parts of four index arrays
    (rows 4 r + kk of every tile of the part's units), and the number of parts."""
    upp, nparts = waic_parts(C_, N, n)
    T = (N + 15) // 16
    row = np.tile(np.arange(N), C_)
    unit = np.repeat(np.arange(C_), N) * T + row // 16
    part, kk = unit // upp, (row % 16) % 4
    idx = np.arange(C_ * N)
    return [[idx[(part == j) & (kk == g)] for g in range(4)] for j in range(nparts)], nparts


def loglik_error(case, l):
    """e [S][n] >= |computed l - l| for the device's evaluation of one element (include/fmcmc_amd.h): the fma chain of the matrix
    core over K terms (gamma(K + 1) sum |terms|), fmh_log / fmh_exp / fmh_log1p below one ulp (<= 2 u relative)."""
    m, th = case.model, case.draws.astype(LD)
    ic, p = case.ic, case.p
    X = m.X.astype(LD) if p else np.zeros((case.n, 0), dtype=LD)
    y = m.y.astype(LD)
    A = (np.abs(th[:, :1]) if ic else 0) + np.abs(th[:, ic:ic + p]) @ np.abs(X).T            # [S][n]
    absl = np.abs(l)
    if case.family == "logistic":
        dt = gamma(ic + p + 1) * A
        eta = (th[:, :1] if ic else 0) + th[:, ic:ic + p] @ X.T
        e = np.exp(-np.abs(eta))
        return U * absl + LD(2.01) * dt + 2 * U * (np.log1p(e) + e)
    K = ic + p + 1
    A = A + np.abs(y)[None, :]
    dr = gamma(K + 1) * A
    sigma = th[:, -1:]
    w = LD(0.5) / (sigma * sigma)
    r = y[None, :] - ((th[:, :1] if ic else 0) + th[:, ic:ic + p] @ X.T)
    return U * absl + 4 * U * (np.abs(np.log(sigma)) + LD(0.9189385332046727)) + 5 * U * w * r * r + 2 * w * np.abs(r) * dr \
        + w * dr * dr


SLACK = LD(1.01)                     # over the first-order terms below: what the products of two rounding errors can add


def _lane(ll, emax):
    """One lane group's draws ll [L][n] in the order the lane meets them: its exact statistics and the running bounds of what
    the lane computes from the evaluated l: the shifted sums (d = l - K rounded, the sum of d sequential, the sum of d^2 by
    fma), mean = K + sd / L, M2 = sdd - sd^2 / L, and the running maximum with E rescaled when it moves."""
    L, n = ll.shape
    d = ll - ll[0]
    sd, A1, Q = d.sum(axis=0), np.abs(d).sum(axis=0), (d * d).sum(axis=0)
    mean = ll.mean(axis=0)
    M2 = Q - sd * sd / L
    gl = gamma(L)
    em = (gl + U) * A1 / L + U * np.abs(mean)
    eM2 = gamma(L + 2) * Q + (2 * gl * np.abs(sd) * A1 + (gl * A1) ** 2 + 2 * U * sd * sd) / L + U * np.abs(M2)
    # every draw that comes within the evaluation error of the running maximum may rescale E: a rounded difference (u |x|), an
    # fmh_exp (2 u) and an fma (u) on all that was summed before
    before = np.vstack([np.full((1, n), -np.inf, dtype=LD), np.maximum.accumulate(ll, axis=0)[:-1]])
    nrec = (ll >= before - 2 * emax).sum(axis=0)
    Rl = ll.max(axis=0) - ll.min(axis=0) + 2 * emax
    rel = gl + (nrec + 1) * (3 * U + U * Rl)
    return SimpleNamespace(cnt=LD(L), mean=mean, M2=M2, em=em, eM2=eM2, top=ll.max(axis=0), rel=rel)


def _merge(a, b, emax):
    """waic_merge of csrc/diag_waic.hpp on the exact statistics, with the running bounds: Chan's update (delta rounded, the
    weight n_b / n, their product, the sum; M2: two sums, delta^2 c with c = n_a n_b / n in four roundings, delta itself off by
    the errors of both means) and the log-sum-exp (the side that holds the maximum is multiplied by exp(0) = 1 exactly; the
    other by an fmh_exp of a rounded difference; one product and one fma)."""
    n = a.cnt + b.cnt
    wa, wb, c = a.cnt / n, b.cnt / n, a.cnt * b.cnt / n
    delta = b.mean - a.mean
    ad = np.abs(delta)
    mean = a.mean + delta * wb
    M2 = a.M2 + b.M2 + delta * delta * c
    em = wa * a.em + wb * b.em + 3 * U * ad * wb + U * np.abs(mean)
    eM2 = a.eM2 + b.eM2 + 2 * U * M2 + c * (2 * ad * (a.em + b.em + U * ad) + (a.em + b.em) ** 2 + 4 * U * delta * delta)
    rel = np.maximum(a.rel, b.rel) + 4 * U + U * (np.abs(a.top - b.top) + 2 * emax)
    return SimpleNamespace(cnt=n, mean=mean, M2=M2, em=em, eM2=eM2, top=np.maximum(a.top, b.top), rel=rel)


def waic_bound(case):
    """The a-priori forward bound of the device's pointwise results and totals for a case, absolute: a namespace with
    point [n][4] (the columns of `pointwise`: elpd_i, p_waic_i, lppd_i, mean_i), total [7] (elpd_waic, p_waic, lppd, waic and the
    three standard errors) and truth = waic_host(..., longdouble).  Two parts each: what the errors e of the evaluated l can
    move the exact result by, and the rounding of the reduction itself, followed through the device's own tree of lanes, lane
    groups and parts (_lane, _merge)."""
    truth = F.waic_host(case.model, case.draws, LD)
    l = waic_loglik(case.model, case.draws, LD)
    S, n = l.shape
    e = loglik_error(case, l)
    emax = e.max(axis=0)
    lanes, _P = _lanes(case.C, case.N, case.n)
    acc = None
    for groups in lanes:
        pa = None
        for idx in groups:
            if idx.size:
                s = _lane(l[idx], emax)
                pa = s if pa is None else _merge(pa, s, emax)
        acc = pa if acc is None else _merge(acc, pa, emax)
    tp = truth.pointwise
    # lppd: |log sum w exp(eps)| <= log sum w exp(e) with w the softmax weights; then E / S, fmh_log (2 u relative, and the
    # relative error of its argument as it is), M + log
    wgt = np.exp(l - l.max(axis=0))
    wgt = wgt / wgt.sum(axis=0)
    logES = tp[:, 2] - l.max(axis=0)
    b_lppd = np.log1p((wgt * np.expm1(e)).sum(axis=0)) + SLACK * (acc.rel + U + 2 * U * np.abs(logES) + U * np.abs(tp[:, 2]))
    b_mean = e.mean(axis=0) + SLACK * acc.em
    data = (2 * np.abs(l - l.mean(axis=0)) * e + e * e).sum(axis=0)
    b_p = (data + SLACK * acc.eM2) / (S - 1) + 2 * U * tp[:, 1]
    b_elpd = b_lppd + b_p + U * np.abs(tp[:, 0])
    point = np.stack([b_elpd, b_p, b_lppd, b_mean], axis=1)
    # totals: the pointwise bounds add; a sum of n terms in any order; the standard error is a 2-norm of centred values
    sums = point[:, :3].sum(axis=0) + gamma(n + 8) * np.abs(tp[:, :3]).sum(axis=0)
    ses = np.array([truth.se_elpd, truth.se_p, truth.se_lppd], dtype=LD)
    with np.errstate(all="ignore"):
        b_se = np.sqrt(LD(n) / LD(n - 1)) * np.sqrt((point[:, :3] ** 2).sum(axis=0)) + gamma(2 * n + 16) * ses if n > 1 \
            else np.full(3, np.nan, dtype=LD)
    total = np.concatenate([sums, [2 * sums[0] + U * np.abs(truth.waic)], b_se])
    return SimpleNamespace(point=point, total=total, truth=truth)


def truth_total(truth):
    return np.array([truth.elpd_waic, truth.p_waic, truth.lppd, truth.waic, truth.se_elpd, truth.se_p, truth.se_lppd], dtype=LD)


def relative_bound(b):
    """The bound in the metric: (pointwise [n][4], totals [7])."""
    return b.point / np.maximum(1, np.abs(b.truth.pointwise)), b.total / np.maximum(1, np.abs(truth_total(b.truth)))


def assert_within(got_point, got_total, b, what=""):
    """got (pointwise [n][4], totals [>= 7]) is inside the bound, and never further than the cap: the tolerance is
    min(bound, CAP).  (tests/test_waic_host.py asserts that the bound itself stays below the cap on the host grid, p <= 62; at
    p = 254 the chain of the matrix core alone takes it to 1.9e-12 and the cap decides: DESIGN.md 5.10.)  Prints the figures
    before it asserts and returns the largest error / bound."""
    rp, rt = relative_bound(b)
    ep, et = metric(got_point, b.truth.pointwise), metric(np.asarray(got_total)[:7], truth_total(b.truth))
    n = b.point.shape[0]
    ok_t = np.ones(7, dtype=bool) if n > 1 else np.array([1, 1, 1, 1, 0, 0, 0], dtype=bool)
    tol_p, tol_t = np.minimum(rp, CAP), np.minimum(rt, CAP)
    worst = max(float((ep / rp).max()), float((et[ok_t] / rt[ok_t]).max()))
    print("%s: largest error %.3g, largest bound %.3g, largest error / bound %.3g"
          % (what, max(float(ep.max()), float(et[ok_t].max())), max(float(rp.max()), float(rt[ok_t].max())), worst))
    assert (ep <= tol_p).all(), (what, float((ep / tol_p).max()))
    assert (et[ok_t] <= tol_t[ok_t]).all(), (what, et, tol_t)
    if n == 1:
        assert np.isnan(np.asarray(got_total, dtype=np.float64)[4:7]).all()
    return worst


# ---------------------------------------------------------------------------------------------- the raw device call
def c_model(dm):
    return dm.c()


def device_waic(case, samples=None, row0=None, S=None, run=None, model=None):
    """One fmcmc_waic_dev call on the case's samples (or `samples` [C][k][S] with the window at row0): NaN-filled buffers GUARD
    doubles longer than documented, which must stay NaN.  Returns (point [n][4], total [10]) as numpy.  run: as in
    tests/diag_dev.py: device_call."""
    import torch
    x = case.samples if samples is None else samples
    row0 = case.row0 if row0 is None else row0
    Cn, k, Srows = x.shape
    dm = (model or case.model).device_model("cuda")
    cm = dm.c()
    L = abi.lib()
    xd = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    lens = (L.fmcmc_waic_work_len(C.byref(cm), 1, Cn, case.N), dm.n * 4, 10)
    assert lens[0] > 0, abi.last_error()
    bufs = [torch.full((int(v) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for v in lens]
    call = lambda stream: L.fmcmc_waic_dev(C.byref(cm), xd.data_ptr(), Cn, k, Srows, row0, case.N, *[b.data_ptr() for b in bufs],
                                           stream)
    rc = call(None) if run is None else run([xd], bufs, call)
    assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    assert all(np.isnan(h[int(v):]).all() for h, v in zip(host, lens))          # nothing past the documented lengths
    return host[1][:lens[1]].reshape(dm.n, 4), host[2][:10]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# The host grid of the issue: both kinds of family, S in {2, 33, 200, 5000}, (n, p) up to (130, 62).
HOST_CASES = [(fam, n, p, ic, C_, N) for fam in ("linreg", "logistic")
              for (n, p, ic) in ((1, 1, 1), (15, 2, 0), (17, 5, 1), (64, 3, 1), (130, 62, 1))
              for (C_, N) in ((1, 2), (1, 33), (2, 100), (5, 1000))] + [("iid", 65, 0, 1, 3, 67)]
