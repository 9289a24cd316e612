"""The inputs, the raw device calls and the tolerances that tests/test_ppc_host.py and tests/test_gpu_ppc.py share: a plain module
next to tests/predict_cases.py, whose make_case and exact_case give the inputs.  torch is imported where it is used, so collecting
needs no GPU.

The keys of a case: draw (c, r) of the window has chain id chain_base + c and id = id0 + id_step r; ID0 = 100 leaves room for the
rows before the window (fmcmc_ppc_yrep_dev counts rows from the start of the buffer, so its id0 is id0 - id_step row0 >= 0).

The tolerances against ppc_host(longdouble), none of them measured on the code under test (fmcmc_amd/summary.py: ppc_host returns
them): e_si = predict_cases.eta_error's bound per draw, d_si = e_si + 2^-53 |y_rep|, dmax_s its largest value over i: min and max
within dmax_s; mean, sd and the chisq pair within CAP = loo_cases.CAP_ELPD = 1e-12 in the metric |got - truth| / max(1, |truth|).
Logistic family: the host lists the elements with |u - p| <= e_si / 4 + 4 x 2^-53, where y_rep may flip; the cases have none, so the
device's y_rep are the host's and its mean, sd, min and max are those of ppc_host(float64) bit for bit (the same fold on the same
0 / 1 values).  Counts: a device count may differ from the host's by at most the draws whose |T_rep - T_obs| is within the
statistic's bound (ppc_host: near), which must be at most S' / 100.

A general logistic case takes a y whose number of ones a (1 or n // 2) is the one farther from the expected sum of y_rep (and
from n minus it, for the sd): with y drawn from the model, T(y_rep) = T(y) exactly for about a seventh of the draws at n = 33
(the mean of 0 / 1 data takes n + 1 values), which is a property of the statistic and not of the device, and no count could be
held to S' / 100.  For the same reason the general logistic cases have n >= 15, and their seeds are those at which the host finds
no draw near T_obs (SEED_STEP; tests/test_ppc_host.py asserts it); n = 1 and 2 of that family are exact cases, where every count
is held to equality."""
import ctypes as C

import numpy as np

import fmcmc_amd as F
from fmcmc_amd import _abi as abi
from fmcmc_amd.summary import ppc_observed

import predict_cases as P

LD = np.longdouble
CAP, GUARD = P.CAP, P.GUARD
bits, metric = P.bits, P.metric
SEED, ID0 = 11, 100
NSTAT, NTOTAL = 6, 17


def keys(case, chain_base=0, id0=ID0, id_step=1):
    """chain ids and ids of case.draws [C N], chain after chain"""
    c, r = np.divmod(np.arange(case.C * case.N), case.N)
    return chain_base + c, id0 + id_step * r


def host(case, dtype=np.float64, seed=SEED, **kw):
    return F.ppc_host(case.model, case.draws, *keys(case, **kw), seed=seed, dtype=dtype)


def general_case(spec, seed):
    """predict_cases.make_case(*spec); the logistic family with the y of the module docstring"""
    case = P.make_case(*spec, seed=seed)
    if case.family == "logistic":
        th = case.draws.mean(axis=0)
        X = np.asarray(case.model.X).reshape(case.m, case.p)
        ek = (1 / (1 + np.exp(-((th[0] if case.ic else 0.0) + X @ th[case.ic:])))).sum()
        a = max((1, case.m // 2), key=lambda a: min(abs(a - ek), abs(case.m - a - ek)))
        y = (np.arange(case.m) < a).astype(np.float64)
        case.model = F.logistic(X, y, intercept=bool(case.ic))
    return case


def exact_case(family, m, p, C_, N, seed):
    return P.exact_case(family, m, p, C_, N, seed)


def _buffers(lens):
    import torch
    return [torch.full((int(v) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for v in lens]


def _finish(bufs, lens):
    import torch
    torch.cuda.synchronize()
    hostb = [b.cpu().numpy() for b in bufs]
    assert all(np.isnan(h[int(v):]).all() for h, v in zip(hostb, lens))          # nothing past the documented lengths
    return [h[:int(v)] for h, v in zip(hostb, lens)]


def device_ppc(case, seed=SEED, chain_base=0, id0=ID0, id_step=1, samples=None, row0=None, N=None, chains=None, run=None):
    """One fmcmc_ppc_dev call on the case's samples (or `samples` [C][k][S]) with the window [row0, row0 + N) of the chains
    [0, chains): NaN-filled buffers GUARD doubles longer than documented, which must stay NaN.  Returns (stats [C][6][N], total
    [17]) as numpy.  run: as in tests/diag_dev.py: device_call."""
    import torch
    x = case.samples if samples is None else samples
    row0 = case.row0 if row0 is None else row0
    N = case.N if N is None else N
    x = x if chains is None else np.ascontiguousarray(x[:chains])
    Cn, k, Srows = x.shape
    cm = case.model.device_model("cuda").c()
    L = abi.lib()
    xd = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    lens = (L.fmcmc_ppc_work_len(C.byref(cm), Cn, N), Cn * NSTAT * N, NTOTAL)
    assert lens[0] > 0, abi.last_error()
    bufs = _buffers(lens)
    tobs = ppc_observed(case.model)
    call = lambda stream: L.fmcmc_ppc_dev(C.byref(cm), xd.data_ptr(), Cn, k, Srows, row0, N, seed, chain_base, id0, id_step,
                                          tobs.ctypes.data_as(C.POINTER(C.c_double)), *[b.data_ptr() for b in bufs], stream)
    rc = call(None) if run is None else run([xd], bufs, call)
    assert rc == abi.OK, (rc, abi.last_error())
    out = _finish(bufs, lens)
    return out[1].reshape(Cn, NSTAT, N), out[2]


def device_yrep(case, sel_chain, sel_row, seed=SEED, chain_base=0, id0=ID0, id_step=1, samples=None, row0=None):
    """One fmcmc_ppc_yrep_dev call: sel_row counts the rows of the WINDOW (as the ids do); the call itself counts rows of the
    buffer.  Returns yrep [nsel][n]."""
    import torch
    x = case.samples if samples is None else samples
    row0 = case.row0 if row0 is None else row0
    Cn, k, Srows = x.shape
    cm = case.model.device_model("cuda").c()
    L = abi.lib()
    xd = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    sc = np.ascontiguousarray(sel_chain, dtype=np.int64)
    sr = np.ascontiguousarray(np.asarray(sel_row) + row0, dtype=np.int64)
    lens = (sc.size * case.m,)
    bufs = _buffers(lens)
    i64 = C.POINTER(C.c_int64)
    rc = L.fmcmc_ppc_yrep_dev(C.byref(cm), xd.data_ptr(), Cn, k, Srows, seed, chain_base, id0 - id_step * row0, id_step,
                              sc.ctypes.data_as(i64), sr.ctypes.data_as(i64), sc.size, bufs[0].data_ptr(), None)
    assert rc == abi.OK, (rc, abi.last_error())
    return _finish(bufs, lens)[0].reshape(sc.size, case.m)


def flat(stats):
    """[C][6][N] -> [C N][6], chain after chain: the layout of ppc_host's stats"""
    return np.ascontiguousarray(stats.transpose(0, 2, 1).reshape(-1, NSTAT))


def counts_of(total):
    return np.asarray(total[2:], dtype=np.int64).reshape(5, 3)


def assert_general(case, stats, total, truth, what=""):
    """the device's stats [C][6][N] and total against ppc_host(longdouble) within the tolerances of the module docstring; prints
    the figures before it asserts"""
    got = flat(stats)
    S = case.C * case.N
    assert total[0] == S and total[1] == 0
    assert len(truth.flips) == 0, (what, "the case has elements that may flip", len(truth.flips))
    t = truth.stats
    ext = np.abs(got[:, 2:4].astype(LD) - t[:, 2:4])
    cols = [0, 4, 5] + ([1] if case.m > 1 else [])
    em = metric(got[:, cols], t[:, cols])
    diff = np.abs(counts_of(total) - truth.counts).max(axis=1)
    print("%s: mean / sd / chisq %.3g (cap %.3g), min / max error / dmax %.3g, counts differ by %s, near %s of %d"
          % (what or case.name, float(em.max()), CAP, float((ext / truth.dmax[:, None]).max()), diff.tolist(), truth.near.tolist(), S))
    assert (ext <= truth.dmax[:, None]).all(), what
    assert (em <= CAP).all(), (what, float(em.max()))
    if case.m == 1:
        assert np.isnan(got[:, 1]).all() and np.isnan(np.asarray(t[:, 1], dtype=np.float64)).all()
    assert (100 * truth.near <= S).all(), (what, "not a test: too many draws near T_obs", truth.near.tolist())
    assert (diff <= truth.near).all(), (what, diff.tolist(), truth.near.tolist())


# (family, m, p, intercept, chains, rows): the observation tiles of 16 on both sides (and n = 1: sd is NaN; n = 2); a partial last
# unit and S' = 2 ... 3 x 33; no covariates, no intercept (one operand step), two operand steps (k' = 5); the operand widths k' = ic
# + p at and above the switches of the A-tile form (8, 16 and 64 columns in registers; LDS beyond: k' = 65 and 100, k > 64)
GAUSS_POINTS = [("linreg", m, 3, 1, 3, 17) for m in (1, 2, 15, 16, 17, 33)]
LOGIT_POINTS = [("logistic", m, 3, 1, 3, 17) for m in (15, 16, 17, 33)]
ROWS = [(f, 17, 0, 1, C_, N) for f in ("linreg", "logistic") for C_, N in ((1, 2), (3, 15), (1, 16), (3, 17), (1, 33))]
WIDTHS = [(f, 17, kw - 1, 1, 2, 17) for f in ("linreg", "logistic") for kw in (5, 8, 9, 16, 17, 64, 65, 100)]
NO_INTERCEPT = [(f, 33, 3, 0, 3, 33) for f in ("linreg", "logistic")]
SHAPES = GAUSS_POINTS + LOGIT_POINTS + ROWS + WIDTHS + NO_INTERCEPT
KEYS = [dict(chain_base=0, id_step=1), dict(chain_base=7, id_step=5)]


SEED_STEP = {19: 1}                        # index in SHAPES -> steps of 100 added to the seed 3000 + index (see the docstring)


def shape_case(spec):
    i = SHAPES.index(spec)
    return general_case(spec, seed=3000 + i + 100 * SEED_STEP.get(i, 0)), KEYS[i % 2]


# (family, m, p, chains, rows) of predict_cases.exact_case (always with an intercept)
EXACT = [(f, m, p, C_, N) for f in ("linreg", "logistic")
         for m, p, C_, N in ((1, 3, 1, 33), (2, 3, 3, 17), (15, 3, 1, 16), (16, 4, 3, 15), (17, 3, 3, 33), (33, 7, 1, 50), (33, 3, 1, 3))]


def exact_shape_case(spec):
    i = EXACT.index(spec)
    return exact_case(*spec, seed=500 + i), KEYS[(i + 1) % 2]
