"""The inputs, the raw device call and the tolerances that tests/test_predict_host.py and tests/test_gpu_predict.py share: a plain
module next to tests/waic_cases.py (metric, bits, GUARD) and tests/loo_cases.py (CAP_ELPD).  torch is imported where it is used,
so collecting needs no GPU.

The input family is waic_cases.make_case's: X uniform on [-2, 2]; coefficients (the intercept included) N(0, 1) / sqrt(max(1, p));
draws = truth + 0.1 N(0, 1); sigma uniform on [0.5, 2] with a relative spread (times exp(0.1 N(0, 1))), as loo_cases.big_case.

The tolerances against predict_host(longdouble), none of them measured on the code under test:
  e_is = (k' + 2) 2^-53 (|b0_s| + sum_j |Xn[i][j] beta_sj|), the bound of a fused dot product of k' terms in any order; emax_i = its
  largest value over the draws;
  quantiles of linpred (and of epred for the Gaussian family, which is the same number): emax_i + 2^-52 |q| (order statistics are
  1-Lipschitz in the sup norm, a type-7 quantile is a convex combination of two);
  quantiles of epred for the logistic family: a quarter of that (the slope of the logistic map) plus 4 x 2^-53;
  mean, sd, sd_pred and the mean of eta: 1e-12 in the metric |got - truth| / max(1, |truth|) (loo_cases.CAP_ELPD)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import fmcmc_amd as F
from fmcmc_amd import _abi as abi
from fmcmc_amd.summary import PREDICT_KINDS

import loo_cases as LC
import waic_cases as W

LD = np.longdouble
U = LD(2.0) ** -53
CAP = LC.CAP_ELPD
GUARD = W.GUARD
ROW0 = 3
PROBS = (0.025, 0.5, 0.975)
KINDS = ("linpred", "epred")
bits, metric = W.bits, W.metric


def make_case(family, m, p, intercept, C_, N, seed, row0=ROW0):
    """A model of `family` ("linreg", "logistic") on m points and samples [C][k][S] around its truth: S odd, the window
    [row0, row0 + N) holds the draws, the rows around it other values.  draws [C N][k]: the window, chain after chain."""
    rng = np.random.default_rng(seed)
    ic = int(bool(intercept))
    X = rng.uniform(-2.0, 2.0, (m, p))
    coef = rng.standard_normal(ic + p) / np.sqrt(max(1, p))
    sigma = rng.uniform(0.5, 2.0)
    eta = (coef[0] if ic else 0.0) + (X @ coef[ic:] if p else np.zeros(m))
    if family == "logistic":
        y = (rng.uniform(size=m) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        truth, model = coef, F.logistic(X, y, intercept=bool(ic))
    else:
        y = eta + sigma * rng.standard_normal(m)
        truth, model = np.concatenate([coef, [sigma]]), F.gaussian_linreg(X if p else None, y, intercept=bool(ic))
    k = truth.size
    assert k == model.k
    S = row0 + N + 2
    S += 1 - S % 2
    samples = np.ascontiguousarray(truth[None, :, None] + 0.1 * rng.standard_normal((C_, k, S)))
    if family != "logistic":
        samples[:, -1, :] = sigma * np.exp(samples[:, -1, :] - sigma)
    return finish(SimpleNamespace(family=family, m=m, p=p, ic=ic, C=C_, N=N, k=k, S=S, row0=row0, model=model, samples=samples,
                                  name="%s m%d p%d ic%d C%d N%d" % (family, m, p, ic, C_, N)))


def exact_case(family, m, p, C_, N, seed, row0=ROW0):
    """Integer covariates in [-3, 3] and integer draws in [-4, 4] (sigma in 1 .. 3): every eta is an exact double whatever the
    order of its sum.  Every row repeats its predecessor with probability 0.6 (a rejected step), row 1 of every second pair
    always: at least half of the rows do."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, (m, p)).astype(np.float64)
    y = np.zeros(m)
    model = F.logistic(X, y, intercept=True) if family == "logistic" else F.gaussian_linreg(X, y, intercept=True)
    k = model.k
    S = row0 + N + 2
    S += 1 - S % 2
    samples = rng.integers(-4, 5, (C_, k, S)).astype(np.float64)
    if family != "logistic":
        samples[:, -1, :] = rng.integers(1, 4, (C_, S))
    keep = rng.uniform(size=(C_, S)) < 0.6
    keep[:, 1::2] = True
    keep[:, row0] = False
    for s in range(1, S):
        samples[:, :, s] = np.where(keep[:, None, s], samples[:, :, s - 1], samples[:, :, s])
    case = finish(SimpleNamespace(family=family, m=m, p=p, ic=1, C=C_, N=N, k=k, S=S, row0=row0, model=model,
                                  samples=np.ascontiguousarray(samples), name="exact %s m%d p%d C%d N%d" % (family, m, p, C_, N)))
    win = case.samples[:, :, row0:row0 + N]
    repeats = (win[:, :, 1:] == win[:, :, :-1]).all(axis=1).sum()
    assert 2 * repeats >= C_ * (N - 1), (repeats, C_ * N)
    return case


def finish(case):
    """(re)derive draws [C N][k] from case.samples"""
    case.draws = np.ascontiguousarray(case.samples[:, :, case.row0:case.row0 + case.N].transpose(0, 2, 1).reshape(case.C * case.N,
                                                                                                                  case.k))
    return case


def eta_error(case, newdata=None):
    """emax [m]: the largest a-priori bound e_is of the device's eta over the draws, from the inputs alone, in longdouble"""
    th = case.draws.astype(LD)
    ic, p = case.ic, case.p
    Xn = np.asarray(case.model.X if newdata is None else newdata, dtype=LD).reshape(-1, p)
    A = (np.abs(th[:, :1]) if ic else 0) + np.abs(th[:, ic:ic + p]) @ np.abs(Xn).T
    return ((ic + p + 2) * U * A).max(axis=0)


def device_predict(case, kind="epred", probs=PROBS, newdata=None, samples=None, row0=None, run=None):
    """One fmcmc_predict_dev call on the case's samples (or `samples` [C][k][S] with the window at row0) at the model's own X (or
    newdata [m][p], through the model's constructor path): NaN-filled buffers GUARD doubles longer than documented, which must
    stay NaN.  Returns (point [m][4 + nprobs], total [4]) as numpy.  run: as in tests/diag_dev.py: device_call."""
    import torch
    from fmcmc_amd.engine import DeviceModel
    x = case.samples if samples is None else samples
    row0 = case.row0 if row0 is None else row0
    Cn, k, Srows = x.shape
    mo = case.model
    if newdata is None:
        dm = mo.device_model("cuda")
    else:
        nd = np.asarray(newdata, dtype=np.float64).reshape(-1, mo.p)
        dm = DeviceModel(mo.family, nd if mo.p else None, np.zeros(nd.shape[0]), mo.intercept, mo.guard, mo.prior_div, device="cuda")
    cm = dm.c()
    L = abi.lib()
    probs_h = np.ascontiguousarray(probs, dtype=np.float64)
    nprobs = int(probs_h.size)
    xd = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    lens = (L.fmcmc_predict_work_len(C.byref(cm), Cn, case.N, nprobs), dm.n * (4 + nprobs), 4)
    assert lens[0] > 0, abi.last_error()
    bufs = [torch.full((int(v) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for v in lens]
    call = lambda stream: L.fmcmc_predict_dev(C.byref(cm), xd.data_ptr(), Cn, k, Srows, row0, case.N, PREDICT_KINDS[kind],
                                              probs_h.ctypes.data_as(C.POINTER(C.c_double)), nprobs,
                                              *[b.data_ptr() for b in bufs], stream)
    rc = call(None) if run is None else run([xd], bufs, call)
    assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    assert all(np.isnan(h[int(v):]).all() for h, v in zip(host, lens))          # nothing past the documented lengths
    return host[1][:lens[1]].reshape(dm.n, 4 + nprobs), host[2][:4]


def quantile_tolerance(case, truth, emax, kind):
    """[m][nprobs], absolute"""
    base = emax[:, None] + 2 * U * np.abs(truth.quantiles)
    return base / 4 + 4 * U if (case.family == "logistic" and kind == "epred") else base


def assert_matches(case, point, truth, emax, kind, what=""):
    """point [m][4 + nprobs] of the device (or of predict_host in float64) against predict_host(longdouble) within the
    tolerances of the module docstring.  Prints the figures before it asserts; returns the largest moment error."""
    gauss = case.family != "logistic"
    cols = [0, 1, 3] + ([2] if gauss else [])
    em = metric(point[:, cols], truth.point[:, cols])
    print("%s %s: mean / sd / sd_pred / mean eta %.3g (cap %.3g)" % (what or case.name, kind, float(em.max()), CAP), end="")
    nprobs = truth.quantiles.shape[1]
    if nprobs:
        dq = np.abs(np.asarray(point[:, 4:], dtype=LD) - truth.quantiles)
        tol = quantile_tolerance(case, truth, emax, kind)
        print(", quantiles: largest error / tolerance %.3g" % float((dq / tol).max()))
        assert (dq <= tol).all(), (what, kind, float((dq / tol).max()))
    else:
        print()
    assert (em <= CAP).all(), (what, kind, float(em.max()))
    if not gauss:
        assert np.isnan(np.asarray(point[:, 2], dtype=np.float64)).all()
    return float(em.max())


# (family, m, p, intercept, chains, rows): the 16 points of a wavefront and the 64 of a workgroup on both sides; the last tile of
# a chain and S' = 2; 36 units in two parts and 66 units in three (a part: 32 units of 16 rows); the operand widths k' = ic + p one
# below, at and one above the switches of the B-tile form (8, 16 and 64 columns in registers; LDS beyond: k' = 100); no intercept.
FAMILIES = ("linreg", "logistic")
POINTS = [(f, m, 3, 1, 2, 33) for f in FAMILIES for m in (1, 63, 64, 65, 130)]
ROWS = [(f, 17, 2, 1, C_, N) for f in FAMILIES for C_ in (1, 3) for N in (2, 15, 16, 17, 33)]
PARTS = [(f, 65, 3, 1, 3, N) for f in FAMILIES for N in (181, 350)]
WIDTHS = [(f, 17, kw - 1, 1, 2, 17) for f in FAMILIES for kw in (7, 8, 9, 15, 16, 17, 63, 64, 65, 100)]
NO_INTERCEPT = [(f, 17, p, 0, 2, 33) for f in FAMILIES for p in (3, 8, 9)]
SHAPES = POINTS + ROWS + PARTS + WIDTHS + NO_INTERCEPT
PROB_SETS = {"none": (), "one": (0.3,), "sixteen": tuple(np.linspace(0.01, 0.99, 16)), "least-and-largest": (0.0, 1.0),
             "duplicate": (0.25, 0.5, 0.25)}


def shape_case(spec):
    return make_case(*spec, seed=2000 + SHAPES.index(spec))
