"""Host-side tests of the device summary (no GPU): the C-ABI surface and its argument checks, the host finish of
fmcmc_amd/summary.py on hand-made numbers, and the reference-owned pin of the spectrum-at-zero path (the README's printed
`Naive SE` / `Time-series SE` columns reproduced by the host restatement of coda::spectrum0.ar)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "readme_summary.json")))
NEW = ("fmcmc_summary_work_len", "fmcmc_summary_pooled_len", "fmcmc_summary_dev")


def sig(x, d):
    return float("%.*g" % (d, x))


@pytest.fixture(scope="module")
def L():
    from fmcmc_amd import _abi as abi
    return abi.lib()


def test_new_symbols_declared_exported_and_bound(L):
    from fmcmc_amd import _abi as abi
    header = open(os.path.join(ROOT, "include", "fmcmc_amd.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in abi.EXPORTS, name
    assert "#define FMCMC_ABI_VERSION 6" in header
    assert L.fmcmc_abi_version() == 6 == abi.ABI_VERSION


def test_lengths(L):
    assert L.fmcmc_summary_pooled_len(3, 5) == 3 * 5 + 3 * 5 * 2
    assert L.fmcmc_summary_pooled_len(3, 0) == 15
    # per series: 72 doubles of autocovariances and friends + 4 of statistics; per target: 3 words of state + 256 counts
    assert L.fmcmc_summary_work_len(48, 3, 5) == 48 * 3 * (72 + 4) + 3 * 5 * 2 * (3 + 256)
    assert L.fmcmc_summary_work_len(48, 3, 0) == 48 * 3 * (72 + 4)
    assert L.fmcmc_summary_work_len(0, 3, 5) == 0


def _call(L, nchains=2, k=3, S=100, row0=0, N=100, p=3, probs=(0.5,), nprobs=None, null=()):
    """fmcmc_summary_dev with made-up device addresses: every call here must return before anything touches them."""
    fake = lambda name, addr: None if name in null else C.c_void_p(addr)
    pr = np.ascontiguousarray(probs, dtype=np.float64)
    nprobs = len(probs) if nprobs is None else nprobs
    return L.fmcmc_summary_dev(fake("samples", 4096), nchains, k, S, row0, N, fake("cols", 8192), p,
                               pr.ctypes.data_as(C.POINTER(C.c_double)) if "probs" not in null else None, nprobs,
                               fake("work", 12288), None, fake("pooled", 16384), None)


@pytest.mark.parametrize("kw, code, text", [
    (dict(p=0), "ERR_ARG", "p = 0"),
    (dict(N=2), "ERR_ARG", "N = 2"),
    (dict(row0=1), "ERR_ARG", "[1, 101)"),
    (dict(row0=-1, N=50), "ERR_ARG", "[-1, 49)"),
    (dict(probs=(0.5, 1.5)), "ERR_ARG", "probs[1] = 1.5"),
    (dict(probs=(-0.1,)), "ERR_ARG", "probs[0] = -0.1"),
    (dict(probs=(float("nan"),)), "ERR_ARG", "probs[0]"),
    (dict(probs=tuple(np.linspace(0, 1, 17))), "ERR_ARG", "nprobs = 17"),
    (dict(nprobs=-1), "ERR_ARG", "nprobs = -1"),
    (dict(nchains=0), "ERR_ARG", "nchains = 0"),
    (dict(null=("samples",)), "ERR_ARG", "null"),
    (dict(null=("probs",)), "ERR_ARG", "null"),
    (dict(S=3162278, N=3162278), "ERR_UNSUPPORTED", "AR order up to 65"),
])
def test_argument_errors_come_before_any_device_call(L, kw, code, text):
    from fmcmc_amd import _abi as abi
    assert _call(L, **kw) == getattr(abi, code)
    assert text in abi.last_error(), abi.last_error()


def test_largest_supported_window_passes_the_order_check(L):
    """N = 3162277 -> M = floor(10 log10 N) = 64 is the last supported length: the call gets past the AR-order check (here it
    stops at the next one, a prob outside [0, 1], still without a device)."""
    from fmcmc_amd import _abi as abi
    assert _call(L, S=3162277, N=3162277, probs=(2.0,)) == abi.ERR_ARG
    assert "probs[0]" in abi.last_error()


# ------------------------------------------------------------------------------------------------ host finish
def test_type7_on_hand_made_numbers():
    from fmcmc_amd.summary import type7_quantiles, type7_ranks
    # n = 5, probs 0 / .25 / .5 / 1: index = 1, 2, 3, 5 are integral -> x_(lo) itself, whatever x_(hi) holds
    idx, lo, hi = type7_ranks(5, [0.0, 0.25, 0.5, 1.0])
    assert list(idx) == [1.0, 2.0, 3.0, 5.0] and list(lo) == [1, 2, 3, 5] and list(hi) == [1, 2, 3, 5]
    q = type7_quantiles([[10.0, 99.0], [20.0, 99.0], [30.0, 99.0], [50.0, 99.0]], 5, [0.0, 0.25, 0.5, 1.0])
    assert list(q) == [10.0, 20.0, 30.0, 50.0]
    # n = 4, prob = .5: index = 2.5 -> halfway between x_(2) and x_(3); prob = .1: index = 1.3
    idx, lo, hi = type7_ranks(4, [0.5, 0.1])
    assert list(lo) == [2, 1] and list(hi) == [3, 2]
    q = type7_quantiles([[2.0, 4.0], [1.0, 2.0]], 4, [0.5, 0.1])
    assert q[0] == 3.0
    h = (1.0 + 3 * 0.1) - 1
    assert q[1] == (1.0 - h) * 1.0 + h * 2.0
    # x_(hi) == x_(lo): the value itself, bit for bit (a rejected step repeats its row), also for an infinite tie
    v = 0.1 + 0.2
    assert type7_quantiles([[v, v]], 4, [0.5])[0] == v
    assert type7_quantiles([[np.inf, np.inf]], 4, [0.5])[0] == np.inf
    # a leading (column) axis is carried along
    q = type7_quantiles(np.array([[[2.0, 4.0]], [[6.0, 7.0]]]), 4, [0.5])
    assert q.shape == (2, 1) and list(q[:, 0]) == [3.0, 6.5]


def test_se_formulas_with_several_chains():
    from fmcmc_amd.summary import finish_statistics
    st = finish_statistics([[1.5, 4.0, 9.0, 0, 0], [0.0, 0.25, 0.0, 0, 0]], nchain=4, niter=25)
    assert st.shape == (2, 4)
    assert list(st[0]) == [1.5, 2.0, np.sqrt(4.0 / 100), np.sqrt(9.0 / 100)]
    assert list(st[1]) == [0.0, 0.5, 0.05, 0.0]


def test_summary_prints_codas_layout():
    from fmcmc_amd.summary import McmcSummary
    stats = np.array([R["mean"], R["sd"], R["naive_se"], R["ts_se"]]).T
    s = McmcSummary(stats, R["quantiles"], R["probs"], R["varnames"], 1, 5000, 1, 1)
    assert s.niter == 5000
    want = """
Iterations = 1:5000
Thinning interval = 1
Number of chains = 1
Sample size per chain = 5000

1. Empirical mean and standard deviation for each variable,
   plus standard error of the mean:

      Mean      SD Naive SE Time-series SE
par1 3.113 0.17593 0.002488       0.024341
par2 1.975 0.10647 0.001506       0.022105
par3 4.093 0.07843 0.001109       0.005951

2. Quantiles for each variable:

      2.5%   25%   50%   75% 97.5%
par1 2.975 3.029 3.068 3.255 3.354
par2 1.749 1.907 1.980 2.020 2.145
par3 3.978 4.070 4.101 4.102 4.226
"""
    assert [line.rstrip() for line in str(s).split("\n")] == want.split("\n")   # (coda ends three header lines with a blank)
    s4 = McmcSummary(stats, R["quantiles"], R["probs"], R["varnames"], 501, 2999, 2, 48)
    assert "Iterations = 501:2999" in str(s4) and "Number of chains = 48 " in str(s4)
    assert "Sample size per chain = 1250 " in str(s4)


def test_package_exports():
    import fmcmc_amd
    from fmcmc_amd import DeviceChains
    for name in ("summary", "effective_size", "McmcSummary"):
        assert name in fmcmc_amd.__all__ and hasattr(fmcmc_amd, name)
    for name in ("summary", "effective_size", "geweke"):
        assert callable(getattr(DeviceChains, name))


# ------------------------------------------------------------------------------------------------ the yardstick
def test_host_spectrum0_reproduces_the_readme_standard_errors(O, readme_data):
    """README.md:191-194: Naive SE = sqrt(var / n), Time-series SE = sqrt(spectrum0.ar / n).  The oracle's first README run
    (R's Mersenne-Twister stream, canonical math) through the host restatement gives both printed columns at their 4 printed
    significant digits: the GPU tests hold the device to this restatement."""
    from fmcmc_amd.convergence import spectrum0_ar
    X, y = readme_data
    model = O.Model(O.FAM_LINREG, X, y, intercept=True, guard=True)
    r = O.run(model, O.Kernel(O.K_NORMAL, 3), [0, 0, O.r_sd(y)], nsteps=5000, rng_mode=O.RNG_RMT, math_mode=O.MATH_CANON,
              rng=O.RRng(1215))
    s = r.samples[0]
    n = s.shape[0]
    assert n == R["niter"]
    naive = np.sqrt(s.var(0, ddof=1) / n)
    ts = np.array([np.sqrt(spectrum0_ar(s[:, j])[0] / n) for j in range(3)])
    assert [sig(v, 4) for v in naive] == R["naive_se"]
    assert [sig(v, 4) for v in ts] == [sig(v, 4) for v in R["ts_se"]]
    assert [spectrum0_ar(s[:, j])[1] for j in range(3)] == [28, 35, 36]


# ------------------------------------------------------------------------------------------------ the edge tests' own references
# tests/test_gpu_summary_edges.py holds the device to references and inputs that are built there; what those tests rely on is
# proved here from the host alone (run with -s for the distances of the float64 family from longdouble).
@pytest.fixture(scope="module")
def T():
    import test_gpu_summary_edges
    return test_gpu_summary_edges


def test_edge_references_restate_the_yardstick(T):
    from test_gpu_summary import LD, ar1, host_series, spec0_tolerance
    rng = np.random.default_rng(1)
    series = [ar1(0.7, 700, rng, mu=2.0), T.seasonal(1300, 31, rng, mu=-1.0), ar1(0.9, 5, rng), np.full(50, 2.5)]
    for y in series:                              # the longdouble reference is host_series, bit for bit
        a, b = T.restate(y, LD, acov=True), host_series(y, LD)
        assert all(a[f] == b[f] for f in ("mean", "var", "spec0", "order", "gap"))
    tol, refs = T.edge_tolerance(series, "self-check")
    tol0, _ = spec0_tolerance(series, "self-check, two members")
    assert tol >= tol0 > 0 and [r["order"] for r in refs] == [host_series(y, LD)["order"] for y in series]
    # the autocovariances handed to check_acov are what their names say
    y = series[1]
    xc = y.astype(LD) - y.astype(LD).sum() / y.size
    assert np.array_equal(refs[1]["xc"], xc)
    for l in (0, 1, 30, 31):
        assert refs[1]["r"][l] == (xc[:y.size - l] * xc[l:]).sum() / LD(y.size)
        assert abs(refs[1]["absr"][l] - np.abs(xc[:y.size - l] * xc[l:]).sum()) <= 1e-12 * refs[1]["absr"][l]
    # strided_sum: element i joins chain i mod 512 in row order; the 512 chains join pairwise
    v = rng.standard_normal(512 * 300 + 77)
    chains = np.zeros(512)
    for i, x in enumerate(v):
        chains[i % 512] += x
    while chains.size > 1:
        chains = chains[0::2] + chains[1::2]
    assert T.strided_sum(v) == chains[0] and T.strided_sum(v[:5]) == (v[0] + v[1]) + (v[2] + v[3]) + v[4]
    # seasonal obeys its recurrence with unit innovations; key_sort is np.sort where np.sort is defined, and splits the zeros
    x = T.seasonal(40000, 42, np.random.default_rng(2), phi=0.6, mu=3.0) - 3.0
    e = x[42:] - 0.6 * x[:-42]
    assert abs(e.std() - 1.0) < 0.02 and abs(np.corrcoef(e[42:], e[:-42])[0, 1]) < 0.02 and abs(x.var() - 1 / 0.64) < 0.05
    w = np.concatenate([rng.standard_normal(1000) * 10.0 ** rng.integers(-300, 300, 1000), [5e-324, -5e-324, 1.7e308, -1.7e308]])
    assert np.array_equal(T.key_sort(w).view(np.uint64), np.sort(w).view(np.uint64))
    assert [str(z) for z in T.key_sort(np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0]))] == ["-1.0", "-0.0", "-0.0", "0.0", "0.0", "1.0"]
    assert [T.first_n_of_order(M) for M in (16, 40, 48, 63, 64, 65)] == [40, 10000, 63096, 1995263, 2511887, 3162278]


def _edge_cases(T, group):
    if group == "short":
        return [T.length_case(N, nchains=3) for N in T.SHORT + (20, 21, 40)]
    if group == "strides":
        return [T.length_case(N) for N in T.STRIDES]
    if group == "group-edges":
        return [T.length_case(n) for M in T.GROUP_EDGES for n in (T.first_n_of_order(M) - 1, T.first_n_of_order(M))]
    if group == "tile":
        return [T.length_case(N) for N in T.TILE_EDGES]
    if group == "width":
        return [(T.width_case(256), None), (T.width_case(65, seed=65), None)]
    return [T.big_case(int(group))]


@pytest.mark.parametrize("group", ["short", "strides", "group-edges", "tile", "width", "2511886", "2511887", "3162277"])
def test_edge_inputs_select_their_orders_with_a_clear_gap(T, group):
    """Every series of the series-length and width tests: the longdouble reference selects the order the input is built for
    (lag = M and M - 2: spec0 needs every lag), with an AIC gap of at least 1e-3, so check_series leaves out no series."""
    worst = 0.0
    for arr, orders in _edge_cases(T, group):
        C_, N, k = arr.shape
        label = "%s: %d x %d x %d" % (group, C_, N, k)
        tol, refs = T.edge_tolerance([arr[c, :, j] for c in range(C_) for j in range(k)], label, acov=False)
        T.check_reference(refs, orders, label)
        assert all(r["gap"] >= 1e-6 for r in refs)                 # check_series' own threshold for leaving a series out
        if orders is None:
            print("    AR(1) inputs: selected orders %d .. %d" % (min(r["order"] for r in refs), max(r["order"] for r in refs)))
        assert 0 < tol < 1e-11, (label, tol)
        worst = max(worst, tol)
    print("[%s] largest tolerance %.3g" % (group, worst))
