"""The inputs, the raw device call, the truth and the bounds that tests/test_pnorm_host.py, tests/test_predictive_host.py and
tests/test_gpu_predictive.py share: a plain module next to tests/predict_cases.py, whose make_case, eta_error, bits and metric it
uses.  torch is imported where it is used, so collecting needs no GPU.

The truth of a returned quantile t of point i at prob p is G(t) = F_i(t) - p (for p > 1/2: (1 - p) - (1 - F_i)(t)) with the mean
over the draws taken in longdouble of scipy.special.ndtr at u = (t - eta) / sigma formed in longdouble and rounded to float64.

The acceptance property of a returned (point, prob): |G(t)| <= tol(p) + B_F, or G changes sign within t +- 2 ulp.  tol(p) is the
code's own stopping bound (summary.py: predictive_tol for the device's order of operations, predictive_host_tol for numpy's).
B_F bounds |g computed - G| from the inputs alone, none of it measured on the code under test:
  side (tol(p) / side + NDTR_REL + 2 PNORM_REL)      the rounding of the code's sum (its own budget c eps, which is what tol is),
                                                     the error of the truth's ndtr and of the code's Phi, relative to the tail
                                                     mass side = min(p, 1 - p) (at a root the tail sum is side up to tol);
  2 d_i(t) (emax_i + 2^-52 |t|)                      the code forms u from its own eta, off by at most emax_i (predict_cases.
                                                     eta_error: a fused dot product in any order) and from t - eta and a product
                                                     with 1 / sigma, three roundings: a shift of every component by that much
                                                     changes F by the mixture's density d_i(t) times the shift to first order; 2
                                                     for the orders beyond;
  2^-52 mean_s |u_s| phi(u_s)                        the truth's own rounding of u to float64, and the code's of its u.
mean, sd_pred: predict_cases.CAP in predict_cases.metric, as for predict(), plus 2 emax_i (moment_bound): the mean of eta + delta
differs from the mean of eta by at most max |delta|, and so does its sd (the triangle inequality of the L2 norm, times
sqrt(S / (S - 1)) <= 2), and sd_pred = sqrt(var + mean sigma^2) moves by no more than the sd; family (e) has emax ~ 10^-7.  pit, pit_upper: B_F with side := the value itself
and tol := the sum's budget c eps side.  All GPU tests import numpy and scipy only."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import fmcmc_amd as F
from fmcmc_amd import _abi as abi
import importlib

SM = importlib.import_module("fmcmc_amd.summary")

import predict_cases as PC

LD = np.longdouble
EPS = 2.0 ** -52
PROBS = (1e-6, 0.001, 0.025, 0.5, 0.975, 1 - 1e-6)
GUARD = PC.GUARD
bits, metric, CAP = PC.bits, PC.metric, PC.CAP
MAX_PASSES = 100
FAMILIES = ("a", "b", "c", "d", "e")


def pnorm_grid():
    """The arguments of the Phi tests: 0, +-tiny, Cody's range breaks +- 1 ulp, the underflow edge, 10^4 log-spaced and 10^4
    uniform points of [-38, 9], +-inf, NaN."""
    br = []
    for b in (0.67448975, np.sqrt(32.0)):
        for v in (b, -b):
            br += [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]
    tiny = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300, -1e-300, 1.11e-16, -1.11e-16,
            1e-17, -1e-17]
    edge = np.linspace(-38.6, -37.5, 111)
    logs = np.concatenate([-np.exp(np.linspace(np.log(1e-30), np.log(38.0), 8000)), np.exp(np.linspace(np.log(1e-30), np.log(9.0), 2000))])
    uni = np.linspace(-38.0, 9.0, 10000)
    return np.ascontiguousarray(np.concatenate([tiny, br, edge, logs, uni, [np.inf, -np.inf, np.nan]]), dtype=np.float64)


def pnorm_breaks():
    return [s * b for b in (0.67448975, float(np.sqrt(32.0))) for s in (1.0, -1.0)]


def detmath_host(which, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    rc = abi.lib().fmcmc_detmath_host(which, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), x.size)
    assert rc == abi.OK, abi.last_error()
    return out


def family_case(name, m=17, p=3, C_=2, N=40, seed=0, ic=1):
    """(a) a near-normal posterior (predict_cases.make_case); (b) every draw equal; (c) two chains 100 sigma apart; (d) sigma
    spread over e^+-3; (e) eta offset by 10^8 (intercept), where only the bracket-width criterion can end the search."""
    case = PC.make_case("linreg", m, p, ic, C_, N, seed=4000 + seed + 17 * FAMILIES.index(name))
    x = case.samples
    rng = np.random.default_rng(seed + 5)
    if name == "b":
        x[:] = x[:1, :, :1]
    elif name == "c":
        assert C_ >= 2 and ic
        sig = float(np.median(x[:, -1, :]))
        x[:, 0, :] *= 1.0
        x[1::2, 0, :] += 100.0 * sig
    elif name == "d":
        x[:, -1, :] *= np.exp(rng.uniform(-3.0, 3.0, x[:, -1, :].shape))
    elif name == "e":
        assert ic
        x[:, 0, :] += 1e8
    case.family_name = name
    case.name = "family (%s) %s" % (name, case.name)
    case.y = np.asarray(case.model.y, dtype=np.float64)
    return PC.finish(case)


def points(case, newdata=None):
    """[m][p], float64: newdata, or the model's own X ([m][0] for a model without covariates)"""
    if newdata is not None:
        return np.asarray(newdata, dtype=np.float64).reshape(np.asarray(newdata).shape[0], case.p)
    return np.asarray(case.model.X, dtype=np.float64) if case.p else np.zeros((case.model.y.shape[0], 0))


def eta_error(case, newdata=None):
    """predict_cases.eta_error (emax [m]), also for a model without covariates"""
    th = case.draws.astype(LD)
    Xn = points(case, newdata).astype(LD)
    A = (np.abs(th[:, :1]) if case.ic else 0) + np.abs(th[:, case.ic:case.ic + case.p]) @ np.abs(Xn).T
    return ((case.ic + case.p + 2) * PC.U * A).max(axis=0)


def truth(case, t, probs, newdata=None):
    """G [m][nprobs] at t [m][nprobs], the density d [m][nprobs] and mean |u| phi(u), all in longdouble, from case.draws"""
    from scipy.special import ndtr
    th = case.draws.astype(LD)
    Xn = points(case, newdata).astype(LD)
    eta = (th[:, :1] if case.ic else LD(0)) + th[:, case.ic:case.ic + case.p] @ Xn.T
    rs = (1 / th[:, -1])[:, None]
    t = np.asarray(t, dtype=LD)
    G, d, uphi = (np.zeros(t.shape, dtype=LD) for _ in range(3))
    for j, pr in enumerate(probs):
        u = (t[None, :, j] - eta) * rs
        u64 = u.astype(np.float64)
        with np.errstate(all="ignore"):
            phi = np.exp(-0.5 * u * u) * LD(0.3989422804014326779399461)
            if pr > 0.5:
                G[:, j] = (LD(1) - LD(pr)) - ndtr(-u64).astype(LD).mean(axis=0)
            else:
                G[:, j] = ndtr(u64).astype(LD).mean(axis=0) - LD(pr)
            d[:, j] = (phi * rs).mean(axis=0)
            uphi[:, j] = (np.abs(u) * phi).mean(axis=0)
    return G, d, uphi


def b_f(tol, probs, t, d, uphi, emax):
    pr = np.asarray(probs, dtype=np.float64)
    side = np.where(pr > 0.5, 1.0 - pr, pr)
    return (tol + side * (SM.NDTR_REL + 2 * SM.PNORM_REL))[None, :] + 2 * d * (emax[:, None] + EPS * np.abs(t)) + EPS * uphi


def assert_accepted(case, t, probs, tol, emax, newdata=None, what=""):
    """the acceptance property of the module docstring for every (point, prob); prints the figures before it asserts"""
    t = np.asarray(t, dtype=np.float64)
    G, d, uphi = truth(case, t, probs, newdata)
    bound = np.asarray(tol, dtype=LD)[None, :] + b_f(np.asarray(tol, dtype=LD), probs, t, d, uphi, emax)
    ok = np.abs(G) <= bound
    worst = float((np.abs(G) / bound).max()) if G.size else 0.0
    if not ok.all():                                               # the other criterion: a sign change of G within t +- 2 ulp
        below, above = t.copy(), t.copy()
        for _ in range(2):
            below, above = np.nextafter(below, -np.inf), np.nextafter(above, np.inf)
        Gb, Ga = truth(case, below, probs, newdata)[0], truth(case, above, probs, newdata)[0]
        ok |= (Gb <= 0) & (Ga >= 0)
    print("%s: |G| / (tol + B_F) at most %.3g; %d of %d by the sign change" % (what or case.name, worst, int((np.abs(G) > bound).sum()), G.size))
    assert ok.all(), (what or case.name, np.argwhere(~ok)[:5].tolist(), worst)
    return worst


def device_tol(case, m, probs):
    return SM.predictive_tol(case.C, case.N, m, probs)[0]


def device_predictive(case, probs=PROBS, newdata=None, y="own", samples=None, row0=None, run=None, passes=(MAX_PASSES,)):
    """fmcmc_predictive_dev on the case's samples (or `samples` with the window at row0) at the model's own X and y (or newdata
    [m][p] and y [m] / None): one call per entry of `passes`, the first with resume = 0, the others resuming on the same
    buffers.  NaN-filled buffers GUARD doubles longer than documented, which must stay NaN.  Returns (point [m][4 + 4 nprobs],
    total [6]).  run: as in tests/diag_dev.py: device_call (wraps the first call)."""
    import torch
    from fmcmc_amd.engine import DeviceModel
    x = case.samples if samples is None else samples
    row0 = case.row0 if row0 is None else row0
    Cn, k, Srows = x.shape
    mo = case.model
    nd = points(case, newdata)
    m = nd.shape[0]
    yv = (np.asarray(mo.y, dtype=np.float64) if newdata is None else None) if isinstance(y, str) else y
    dm = DeviceModel(mo.family, nd if mo.p else None, np.zeros(m) if yv is None else np.asarray(yv, dtype=np.float64), mo.intercept,
                     mo.guard, mo.prior_div, device="cuda")
    cm = dm.c()
    if yv is None:
        cm.y = None
    L = abi.lib()
    probs_h = np.ascontiguousarray(probs, dtype=np.float64)
    nprobs = int(probs_h.size)
    xd = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    lens = (L.fmcmc_predictive_work_len(C.byref(cm), Cn, case.N, nprobs), dm.n * (4 + 4 * nprobs), 6)
    assert lens[0] > 0, abi.last_error()
    bufs = [torch.full((int(v) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for v in lens]
    for i, npasses in enumerate(passes):
        call = lambda stream: L.fmcmc_predictive_dev(C.byref(cm), xd.data_ptr(), Cn, k, Srows, row0, case.N,
                                                     probs_h.ctypes.data_as(C.POINTER(C.c_double)), nprobs, int(npasses),
                                                     int(i > 0), *[b.data_ptr() for b in bufs], stream)
        rc = call(None) if (run is None or i > 0) else run([xd], bufs, call)
        assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    assert all(np.isnan(h[int(v):]).all() for h, v in zip(host, lens))          # nothing past the documented lengths
    return host[1][:lens[1]].reshape(dm.n, 4 + 4 * nprobs), host[2][:6]


def split(point, nprobs):
    """(head [m][4], t, g, width, done [m][nprobs]) of a device `point`"""
    per = point[:, 4:].reshape(point.shape[0], nprobs, 4)
    return point[:, :4], per[:, :, 0], per[:, :, 1], per[:, :, 2], per[:, :, 3]


def closed_form_ulps(t, eta, sigma, probs):
    """the distance of t [m][nprobs] from eta_i + sigma qnorm(p) in ulp.  The closed form evaluated in float64 is itself only
    good to an ulp of its LARGEST term: where eta and sigma z nearly cancel, an ulp of the small sum is far below the rounding of
    the product and of eta that went into it.  So the ulp is that of max(|eta|, |sigma z|, |eta + sigma z|)."""
    from scipy.special import ndtri
    sz = float(sigma) * ndtri(np.asarray(probs, dtype=np.float64))[None, :]
    want = np.asarray(eta, dtype=np.float64)[:, None] + sz
    scale = np.maximum(np.abs(want), np.maximum(np.abs(np.asarray(eta, dtype=np.float64))[:, None], np.abs(sz)))
    return np.abs(np.asarray(t, dtype=np.float64) - want) / np.spacing(scale)


def moment_bound(want, emax):
    """the absolute bound of mean and sd_pred against predict_host(longdouble) (module docstring)"""
    return CAP * np.maximum(1, np.abs(want)) + 2 * emax
