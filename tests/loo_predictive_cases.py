"""The inputs, the raw device call and the comparison that tests/test_loo_predictive_host.py and
tests/test_gpu_loo_predictive.py share: a plain module on top of tests/loo_cases.py and tests/waic_cases.py.  torch is imported
where it is used, so collecting needs no GPU.

The tolerance: mean, sd and pit against loo_predictive_host(longdouble) in the metric |got - truth| / max(1, |truth|)
(waic_cases.metric) within loo_cases.CAP_K = 1e-10, the cap that n_eff, the same kind of functional of the smoothed weights,
already meets.  Weights by rank are discontinuous where two distinct r swap their order, so every case has to satisfy a
precondition on the truth (precondition()): within the tail, at the cutoff and one rank below it, adjacent DISTINCT longdouble
values of r lie more than 4 emax_i apart (emax_i: loo_cases.emax_of, the a-priori evaluation error of l); repeated rows give
exactly equal values."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import fmcmc_amd as F
from fmcmc_amd import _abi as abi
from fmcmc_amd.summary import loo_tail_len, waic_loglik

import loo_cases as Lc
import waic_cases as W

LD = Lc.LD
CAP = Lc.CAP_K
GUARD = Lc.GUARD

# (family, n, p, intercept, chains, rows) of waic_cases.make_case (row0 = 5, S odd): the 64-observation tile and its 16-wide
# columns at n = 1, 63, 64, 65, 130 with N = 33 (no multiple of 16; S = 66: M = 0.2 S), one and three chains, S <= 20 (M < 5:
# nothing is smoothed), S = 513 (M = 3 sqrt S), 3 x 200 rows (39 units: two parts), one k per form of the B operand (k = 5, 12, 42
# in registers, k = 72 in LDS) and the logistic family.
SHAPES = [("linreg", n, 3, 1, 2, 33) for n in (1, 63, 64, 65, 130)] + \
         [("linreg", 17, 2, 1, 1, 35), ("linreg", 17, 2, 1, 3, 35), ("linreg", 17, 2, 1, 1, 2), ("linreg", 17, 2, 1, 1, 20),
          ("linreg", 17, 2, 1, 1, 513), ("linreg", 17, 2, 1, 3, 200), ("linreg", 17, 10, 1, 2, 33), ("linreg", 17, 40, 1, 2, 100),
          ("linreg", 65, 70, 1, 2, 300), ("logistic", 65, 5, 1, 2, 33), ("logistic", 17, 2, 0, 3, 200)]
SPECIAL = ["runs", "straddle", "fallback", "runs-logistic"]
NAMES = ["%s-n%d-p%d-ic%d-C%d-N%d" % s for s in SHAPES] + SPECIAL
TIE_FREE = NAMES[:len(SHAPES)]


def _repeat_rows(case, rng, most):
    """MH-like: every row of a chain's window repeated 1 .. most times"""
    win = case.samples[:, :, case.row0:case.row0 + case.N]
    for c in range(case.C):
        src = np.repeat(np.arange(case.N), rng.integers(1, most + 1, case.N))[:case.N]
        win[c] = win[c][:, src]
    return Lc.finish_case(case)


def _straddle_case():
    """S = 600 (M = 74): 70 % of the rows are ONE far-off row, 30 rows lie further off: the tail is those 30 and 44 copies of the
    one row, whose run of about 420 straddles the boundary (c(v) > c_T + 1)"""
    case = W.make_case("linreg", 65, 2, 1, 2, 300, seed=4101)
    rng = np.random.default_rng(9)
    win = case.samples[:, :, case.row0:case.row0 + case.N]
    sd = float(np.median(win[:, -1, :]))
    win[:, -1, :] = sd
    same = rng.uniform(size=(case.C, case.N)) < 0.7
    one = win[0, :, 11].copy()
    one[0] += 14.0 * sd
    for c in range(case.C):
        win[c][:, same[c]] = one[:, None]
    far = np.zeros(same.size, dtype=bool)
    far[rng.choice(np.flatnonzero(~same.ravel()), 30, replace=False)] = True
    far = far.reshape(same.shape)
    win[:, 0, :][far] += sd * rng.uniform(26.0, 28.0, 30) * rng.choice([-1.0, 1.0], 30)
    case = Lc.finish_case(case)
    case.n_far, case.name = 30, "straddle"
    return case


def _fallback_case():
    """S = 3 x 480 = 1440 (M = 114, every second unit in the subsample): more extreme draws than an observation's buffer holds,
    none of them in the subsample, so the threshold lands among the ordinary draws, the buffer overflows and the exact fallback
    (the radix select over all draws) serves every observation (the overflow kind of tests/test_gpu_loo.py, small)"""
    case = W.make_case("linreg", 17, 2, 1, 3, 480, seed=4102)
    P = Lc.plan(case.C, case.N, case.n)
    assert P.ustride == 2 and P.M == 114
    rng = np.random.default_rng(10)
    win = case.samples[:, :, case.row0:case.row0 + case.N]
    sd = float(np.median(win[:, -1, :]))
    win[:, -1, :] = sd
    insub = Lc.sub_rows_mask(P, case.C, case.N)
    cnt = P.cap + 50
    mask = np.zeros(insub.size, dtype=bool)
    mask[rng.choice(np.flatnonzero(~insub.ravel()), cnt, replace=False)] = True
    mask = mask.reshape(insub.shape)
    win[:, 0, :][mask] += sd * rng.uniform(8.0, 10.0, cnt) * rng.choice([-1.0, 1.0], cnt)
    case = Lc.finish_case(case)
    case.name, case.plan = "fallback", P
    return case


_cases = {}


def get_case(name):
    """the case of a name of NAMES, built once"""
    if name not in _cases:
        if name in SPECIAL:
            if name == "runs":
                case = _repeat_rows(W.make_case("linreg", 65, 3, 1, 3, 200, seed=4100), np.random.default_rng(8), 6)
            elif name == "runs-logistic":
                case = _repeat_rows(W.make_case("logistic", 17, 2, 1, 2, 100, seed=4103), np.random.default_rng(11), 6)
            elif name == "straddle":
                case = _straddle_case()
            else:
                case = _fallback_case()
            case.name = name
        else:
            i = NAMES.index(name)
            case = W.make_case(*SHAPES[i], seed=4000 + i)
            case.name = name
        _cases[name] = case
    return _cases[name]


_truths = {}


def truth_of(case):
    """loo_predictive_host in longdouble, computed once per case, with the precondition asserted on it"""
    if case.name not in _truths:
        t = F.loo_predictive_host(case.model, case.draws, LD)
        precondition(case, t)
        _truths[case.name] = t
    return _truths[case.name]


def precondition(case, truth=None):
    """asserts the precondition of the module docstring; returns the least gap / (4 emax) over the observations"""
    l = waic_loglik(case.model, case.draws, LD)
    S, n = l.shape
    M = loo_tail_len(S)
    emax = Lc.emax_of(case)
    top = -np.sort(l, axis=0)[:min(S, M + 2)]                       # the M + 2 largest r, descending
    gaps = -np.diff(top, axis=0)
    least = np.where(gaps > 0, gaps, np.inf).min(axis=0) / (4 * emax)
    assert (least > 1).all(), (case.name, float(least.min()))
    return float(least.min())


def errors(point, truth):
    """the metric of mean, sd and pit (NaN on both sides: 0), and of pareto_k (an infinite k on both sides: 0) and n_eff"""
    tp = truth.point
    out = []
    for q in range(5):
        g, t = np.asarray(point[:, q], dtype=LD), tp[:, q]
        same = (np.isnan(g) & np.isnan(t)) | (np.isinf(g) & np.isinf(t) & (np.sign(g) == np.sign(t)))
        with np.errstate(all="ignore"):
            e = W.metric(np.where(same, 0, g), np.where(same, 0, t))
        out.append(np.where(same, 0, e))
    return np.stack(out, axis=1)


def assert_matches(point, truth, what=""):
    """the device's (or the float64 host's) point [n][6] against the truth within CAP; prints the figures before it asserts and
    returns the largest error of (mean, sd, pit)"""
    e = errors(point, truth)
    worst = e.max(axis=0)
    print("%s: mean %.3g, sd %.3g, pit %.3g, k %.3g, n_eff %.3g" % ((what,) + tuple(float(v) for v in worst)))
    assert np.isfinite(e).all() and (e <= CAP).all(), (what, worst)
    assert (W.metric(point[:, 5], truth.point[:, 5]) <= Lc.CAP_ELPD).all(), what
    return float(worst[:3].max())


def device_loo_predictive(case, samples=None, row0=None, run=None, model=None, want_loo_point=True, want_state=False):
    """One fmcmc_loo_predictive_dev call on the case's samples (or `samples` [C][k][S] with the window at row0): NaN-filled buffers
    GUARD doubles longer than documented, which must stay NaN.  Returns (point [n][6], loo_point [n][6], total [13]) as numpy, and
    with want_state the observations' state words [n][8] of the selection behind them.  run: as in tests/diag_dev.py:
    device_call."""
    import torch
    x = case.samples if samples is None else samples
    row0 = case.row0 if row0 is None else row0
    Cn, k, Srows = x.shape
    dm = (model or case.model).device_model("cuda")
    cm = dm.c()
    L = abi.lib()
    xd = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    lens = (L.fmcmc_loo_predictive_work_len(C.byref(cm), Cn, case.N), dm.n * 6, dm.n * 6, 13)
    assert lens[0] > L.fmcmc_loo_work_len(C.byref(cm), 1, Cn, case.N) > 0, abi.last_error()
    bufs = [torch.full((int(v) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for v in lens]
    call = lambda stream: L.fmcmc_loo_predictive_dev(C.byref(cm), xd.data_ptr(), Cn, k, Srows, row0, case.N, bufs[0].data_ptr(),
                                                     bufs[1].data_ptr(), bufs[2].data_ptr() if want_loo_point else None,
                                                     bufs[3].data_ptr(), stream)
    rc = call(None) if run is None else run([xd], bufs, call)
    assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs[1:]]
    assert all(np.isnan(h[int(v):]).all() for h, v in zip(host, lens[1:]))      # nothing past the documented lengths
    assert torch.isnan(bufs[0][lens[0]:]).all()
    out = (host[0][:lens[1]].reshape(dm.n, 6), host[1][:lens[2]].reshape(dm.n, 6), host[2][:13])
    if want_state:
        off = L.fmcmc_loo_state_offset(C.byref(cm), 1, Cn, case.N)
        assert off >= 0
        return out + (bufs[0][off:off + 8 * dm.n].cpu().numpy().view(np.int64).reshape(dm.n, 8),)
    return out


def check_case(case, what=None, **kw):
    """device_loo_predictive of the case against the truth; every row finite, bad_points = 0"""
    got = device_loo_predictive(case, **kw)
    truth = truth_of(case)
    err = assert_matches(got[0], truth, what or case.name)
    assert got[2][12] == 0 and got[2][10] == 0 and got[2][11] == 0
    return got, truth, err


bits = W.bits
