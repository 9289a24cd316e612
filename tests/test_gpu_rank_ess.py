"""The all-lag autocovariances, Geyer's cut and the rank-normalised bulk / tail effective sample size on the GPU
(csrc/diag_ess.hpp): S(t) of every series against np.longdouble under the bounds of tests/ess_cases.py (derived from the order
of the sums, never from what the kernel returns), the cut, the ESS against ess_host, the tail quantiles bit for bit, the
equalities a fixed order of summation owes, the refusals, and ess() / convergence_rhat(min_ess=) end to end.  The raw entry is
called with NaN-filled buffers GUARD elements longer than documented, which must stay NaN."""
import functools

import numpy as np
import pytest

import ess_cases as ec
from gelman_dev import GUARD

pytestmark = pytest.mark.gpu

T = 2048                            # rows of a tile of the autocovariance kernel in LDS (EA_T, csrc/diag_ess.hpp)
FRONT = 16                          # zeros in front of the series there: the tile's edge is at n + 16 = T
COLS = tuple(range(ec.NCOLS))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ raw calls
def raw(x, row0, N, cols, stream=None, stage=None, keep=None):
    """L.fmcmc_rank_ess_dev on x [C][k][S]: work and out NaN-filled and GUARD longer than documented; returns out [p][.] at its
    documented length.  stream / stage as in tests/test_gpu_rank_rhat.py; keep: a list that receives the device input."""
    import torch
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    Cn, k, S = x.shape
    p = len(cols)
    lens = [L.fmcmc_rank_ess_work_len(Cn, p, N), L.fmcmc_rank_ess_out_len(Cn, p, N)]
    assert lens[0] == L.fmcmc_rank_work_len(Cn, p, N) > 0 and lens[1] == p * (4 * (4 * Cn + 2 + N // 2 - 2) + 7)
    nan = lambda n: torch.full((int(n) + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    bufs = [nan(n) for n in lens]
    cd = torch.as_tensor(np.asarray(cols, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    xd = torch.as_tensor(x).cuda() if stage is None else stage()
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        if stage is not None:
            xd.copy_(torch.as_tensor(x).pin_memory(), non_blocking=True)
        rcode = L.fmcmc_rank_ess_dev(xd.data_ptr(), Cn, k, S, row0, N, cd.data_ptr(), p, *[b.data_ptr() for b in bufs],
                                     st.cuda_stream)
    assert rcode == abi.OK, (rcode, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    assert all(np.isnan(h[int(n):]).all() for h, n in zip(host, lens))          # nothing past the documented lengths
    if keep is not None:
        keep.append(xd.cpu().numpy())
    return host[1][:lens[1]].reshape(p, -1)


def parts(out, Cn, N):
    """out [p][.] -> per column a list of the four series' (means [m], variances [m], L, K, S [L]) and info [7]"""
    m, n = 2 * Cn, N // 2
    kl = 2 * m + 2 + n - 2
    res = []
    for o in out:
        kinds = []
        for kind in range(4):
            part = o[kind * kl:(kind + 1) * kl]
            L = int(part[2 * m])
            assert np.isnan(part[2 * m + 2 + L:]).all()             # S(t) is written below L only
            kinds.append((part[0:2 * m:2], part[1:2 * m:2], L, int(part[2 * m + 1]), part[2 * m + 2:2 * m + 2 + L]))
        res.append((kinds, o[4 * kl:]))
    return res


def split(x, row0, N, col):
    nh = N // 2
    w = x[:, col, row0:row0 + N]
    return np.stack([w[:, :nh], w[:, N - nh:]], axis=1).reshape(2 * x.shape[0], nh)


# (C, N): n = 4, the least; n = 19, 20 around a 16-row operand and the depth of four; n = 255 .. 257, the first lag tile and the
# first round's edge (the cap n - 2 is 253 .. 255); n = 515 just past the second round; several rounds' worth of rows; the LDS
# tile's edge n + 16 = T and the issue's n = T -+ 1 around the tile's length itself
SHAPES = [(1, 8), (2, 9), (3, 39), (3, 40), (2, 510), (2, 511), (2, 512), (2, 513), (2, 514), (2, 515), (3, 1030), (7, 4001),
          (1, 2 * T - 2), (1, 2 * T + 2), (1, 2 * (T - FRONT) - 2), (1, 2 * (T - FRONT)), (1, 2 * (T - FRONT) + 2)]


@functools.lru_cache(maxsize=None)
def case(Cn, N):
    """one fmcmc_rank_ess_dev call on the four columns of make_inputs, and the host's reference for every series of the columns
    that are not constant, shared by the tests"""
    x, row0 = ec.make_inputs(Cn, N, 100 * Cn + N)
    out = raw(x, row0, N, COLS)
    dev = parts(out, Cn, N)
    ref = {}
    for j in (0, 1, 3):
        series, q = ec.series_of(split(x, row0, N, j))
        for kind in range(4):
            ref[(j, kind)] = ec.host_case(series[kind], kind, L=dev[j][0][kind][2])
        ref[(j, "q")] = q
    return x, row0, out, dev, ref


@pytest.mark.parametrize("Cn, N", SHAPES)
def test_sums_against_longdouble(Cn, N):
    """the split chains' means under rhat_cases.moment_bounds, every S(t) the device reports under ess_cases.sum_bound"""
    x, row0, out, dev, ref = case(Cn, N)
    m, n = 2 * Cn, N // 2
    for j in (0, 1, 3):
        for kind in range(4):
            mean, var, L, K, S = dev[j][0][kind]
            r = ref[(j, kind)]
            assert L >= min(256, n - 2) and L == r.S.size and (np.abs(mean - r.mu) <= r.e_mean).all()
            err = np.abs(S - r.S).astype(np.float64)
            worst = int(np.argmax(err / np.maximum(r.ES.astype(np.float64), 1e-300)))
            print("col %d %s: L %d K %d  worst lag %d |S err| %.3g (bound %.3g)"
                  % (j, ec.KINDS[kind], L, K, worst, err[worst], r.ES[worst]))
            assert (err <= r.ES).all(), (j, kind, worst)
    for kind in range(4):                            # the constant column: nothing to sum
        mean, var, L, K, S = dev[2][0][kind]
        assert (S == 0.0).all() and K == 1 and L == min(256, n - 2) and (var == 0.0).all()


ESS_SHAPES = SHAPES + [(4, 2000)]


@pytest.mark.parametrize("Cn, N", ESS_SHAPES)
def test_ess_against_the_host(Cn, N):
    """ess_finish of the device's output against ess_host within ess_cases.ess_bound; the cut K is safe in every case: the
    smallest |P_j| - dP_j at and before it is positive on the host reference alone (checked for these seeds on the CPU: the
    smallest gap over all cases is 4.2e-05, at (1, 4062), the values' scores)."""
    from fmcmc_amd import ess_host
    from fmcmc_amd.summary import ess_finish
    x, row0, out, dev, ref = case(Cn, N)
    fin = ess_finish(out, Cn, N)
    host = ess_host(ec.window(x, row0, N))
    names = ("bulk", "tail_q05", "tail_q95", "mean")
    for j in range(ec.NCOLS):
        for kind, name in enumerate(names):
            have, want = getattr(fin, name)[j], getattr(host, name)[j]
            if j == 2 or np.isnan(want):
                assert np.isnan(have) and np.isnan(want), (j, name)
                continue
            r = ref[(j, kind)]
            assert r.gap > 0.0, (j, name, r.gap)
            assert fin.lags[j, kind] == host.lags[j, kind] == dev[j][0][kind][3] == r.g.K
            print("col %d %s: device %.17g host %.17g |diff| %.3g (bound %.3g) gap %.3g K %d"
                  % (j, name, have, want, abs(have - want), r.bound, r.gap, r.g.K))
            assert abs(have - want) <= r.bound, (j, name)
        both = np.minimum(fin.tail_q05[j], fin.tail_q95[j])
        assert _bits(fin.tail[j]) == _bits(both) or (np.isnan(fin.tail[j]) and np.isnan(both))
        if j != 2:
            sd, tol = ec.pooled_sd_bound(ref[(j, 3)], split(x, row0, N, j))
            print("col %d: pooled sd %.17g host %.17g (bound %.3g)" % (j, fin.pooled_sd[j], sd, tol))
            assert abs(fin.pooled_sd[j] - sd) <= tol
            assert fin.mcse_mean[j] == fin.pooled_sd[j] / np.sqrt(fin.mean[j])
    assert np.isnan(fin.mcse_mean[2]) and np.isnan(fin.tau_bulk[2])


@pytest.mark.parametrize("Cn, N", [(2, 9), (3, 40), (2, 513), (7, 4001), (1, 2 * T + 2)])
def test_tail_quantiles_and_counts_bit_for_bit(Cn, N):
    """q05, q95: the type-7 quantiles of np.sort of the pooled split values to the bit, the five-integer column included; the
    indicators' means times n add up to the counts np.sum(x <= q) gives; least and largest value; no non-finite values"""
    x, row0, out, dev, ref = case(Cn, N)
    n = N // 2
    for j in range(ec.NCOLS):
        v = split(x, row0, N, j) + 0.0
        q = ec.series_of(v)[1]
        info = dev[j][1]
        assert info[0] == 0.0 and _bits(info[1]) == _bits(q[0]) and _bits(info[2]) == _bits(q[1]), j
        assert _bits(info[5]) == _bits(v.min()) and _bits(info[6]) == _bits(v.max())
        for i in (0, 1):
            counts = np.rint(dev[j][0][1 + i][0] * n)
            assert np.array_equal(counts, (v <= q[i]).sum(axis=1)), (j, i)


# ------------------------------------------------------------------------------------------------ the cut
def _one_column(series, row0=3):
    """x [C][1][S] with the rows `series` [C][N] at row0 and guard rows around them"""
    Cn, N = series.shape
    S = row0 + N + 2
    S += 1 - S % 2
    x = np.full((Cn, 1, S), 1e9)
    x[:, 0, row0:row0 + N] = series
    return x, row0


def test_a_ramp_runs_every_round_to_the_cap():
    """rho stays positive: the cap sets K for the scores and the values, every round runs and L is the cap"""
    Cn, N = 7, 4001
    x, row0 = _one_column(ec.ramp(Cn, N, 61))
    (kinds, info), = parts(raw(x, row0, N, (0,)), Cn, N)
    n, cap = N // 2, N // 2 - 2
    series, _ = ec.series_of(split(x, row0, N, 0))
    for kind in range(4):
        mean, var, L, K, S = kinds[kind]
        r = ec.host_case(series[kind], kind, L=L)
        print(ec.KINDS[kind], "L", L, "K", K, "host K", r.g.K, "gap", r.gap)
        assert K == r.g.K and r.gap > 0.0 and (np.abs(S - r.S) <= r.ES).all()
        if kind in (0, 3):
            assert L == cap and K == cap // 2


ALTERNATING_SEED = 2                # (chosen on the CPU: P_1 of the scores and of the values is negative by more than 4e-3)


def test_an_alternating_series_is_cut_at_the_first_pair():
    """P_1 < 0: K = 1, and the device stops after the first round: L = 256 of the 598 lags it could go to"""
    Cn, N = 2, 1200
    x, row0 = _one_column(ec.alternating(Cn, N, ALTERNATING_SEED))
    (kinds, info), = parts(raw(x, row0, N, (0,)), Cn, N)
    series, _ = ec.series_of(split(x, row0, N, 0))
    for kind in (0, 3):
        mean, var, L, K, S = kinds[kind]
        r = ec.host_case(series[kind], kind, L=L)
        print(ec.KINDS[kind], "L", L, "K", K, "host K", r.g.K, "gap", r.gap)
        assert r.g.K == 1 and r.gap > 0.0 and K == 1 and L == 256


# ------------------------------------------------------------------------------------------------ equalities, bit for bit
EQ = (3, 2 * T + 15)                # two LDS tiles of rows, four tiles of the sort


def test_two_launches_agree_and_the_samples_are_not_written():
    x, row0 = ec.make_inputs(*EQ, seed=7)
    keep = []
    a = raw(x, row0, EQ[1], (0, 1, 3), keep=keep)
    b = raw(x, row0, EQ[1], (0, 1, 3))
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(keep[0]), _bits(x))


def test_the_window_elsewhere_in_another_history():
    Cn, N = EQ
    x, row0 = ec.make_inputs(Cn, N, seed=8)
    S2 = N + 40
    S2 += 1 - S2 % 2
    y = np.full((Cn, ec.NCOLS + 2, S2), np.nan)
    y[:, 1:1 + ec.NCOLS, 17:17 + N] = x[:, :, row0:row0 + N]
    y[:, :, :17] = 1e9
    y[:, :, 17 + N:] = -1e9
    a = raw(x, row0, N, (0, 1, 3))
    b = raw(y, 17, N, (1, 2, 4))
    assert x.shape[2] != S2 and S2 % 2 == 1 and np.array_equal(_bits(a), _bits(b))


def test_a_column_alone_and_among_three_in_another_order():
    x, row0 = ec.make_inputs(*EQ, seed=9)
    three = raw(x, row0, EQ[1], (3, 0, 1))
    for j, col in enumerate((3, 0, 1)):
        alone = raw(x, row0, EQ[1], (col,))
        assert np.array_equal(_bits(alone[0]), _bits(three[j])), col


def test_a_side_stream_behind_a_busy_stream():
    """the rows reach the device ON the side stream, behind a kernel that keeps it busy: a call that left its caller's stream
    would read the NaN prefill"""
    import torch
    x, row0 = ec.make_inputs(*EQ, seed=10)
    want = raw(x, row0, EQ[1], (0, 1, 3))
    side = torch.cuda.Stream()

    def stage():
        xd = torch.full(x.shape, float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(4_000_000)             # a few milliseconds
        return xd

    got = raw(x, row0, EQ[1], (0, 1, 3), stream=side, stage=stage)
    assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------ refusals
def test_non_finite_values_are_counted_and_refused():
    import diag_dev as dd
    import fmcmc_amd as f
    N = 1025
    x = dd.make_series(N, 77, non_finite=True)       # one NaN and one infinity in chain 1, column 2
    out = raw(x, dd.ROW0, N, dd.COLS)
    assert [p[1][0] for p in parts(out, dd.CHAINS, N)] == [2.0, 0.0, 0.0]          # COLS = (2, 0, 3)
    w = x[:, :, dd.ROW0:dd.ROW0 + N]
    ml = f.McmcList([f.Mcmc(w[c].T.copy(), start=1, end=N, thin=1) for c in range(dd.CHAINS)])
    with pytest.raises(ValueError, match=r"2 non-finite value\(s\) among the rows to rank \(columns \[2\]\)"):
        f.ess(ml)
    assert np.isfinite(f.ess(ml, cols=[0, 1, 3]).bulk).all()


def test_a_constant_column_gives_nan_and_no_error():
    import fmcmc_amd as f
    x = np.random.default_rng(22).standard_normal((2, 31, 2))
    x[:, :, 1] = 0.1                                 # (a value whose multiples are not exact)
    d = f.ess(f.McmcList([f.Mcmc(x[c], start=1, end=31, thin=1) for c in range(2)]))
    for name in ("bulk", "tail", "tail_q05", "tail_q95", "mean", "mcse_mean", "tau_bulk"):
        assert np.isnan(getattr(d, name)[1]) and (name.startswith("tail") or np.isfinite(getattr(d, name)[0])), name
    assert d.q05[1] == 0.1 and d.q95[1] == 0.1 and "NA" in str(d) and (d.nchains, d.niter) == (2, 31)


def test_short_windows_and_null_pointers_are_refused():
    import torch
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    assert L.fmcmc_rank_ess_work_len(2, 1, 7) == 0 and L.fmcmc_rank_ess_out_len(2, 1, 7) == 0
    assert L.fmcmc_rank_ess_work_len(2, 1, 8) > 0 and L.fmcmc_rank_ess_out_len(2, 1, 8) == 4 * (8 + 2 + 2) + 7
    x = torch.zeros((2, 1, 16), dtype=torch.float64, device="cuda")
    cols = torch.zeros(1, dtype=torch.int32, device="cuda")
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = lambda N, **kw: [kw.get("x", x.data_ptr()), 2, 1, 16, 0, N, kw.get("cols", cols.data_ptr()), 1,
                            kw.get("work", buf.data_ptr()), kw.get("out", buf.data_ptr()), st]
    assert L.fmcmc_rank_ess_dev(*args(7)) == abi.ERR_ARG and "shorter than 8 rows" in abi.last_error()
    for name in ("x", "cols", "work", "out"):
        assert L.fmcmc_rank_ess_dev(*args(8, **{name: None})) == abi.ERR_ARG and "null argument" in abi.last_error(), name
    assert L.fmcmc_rank_ess_dev(*args(17)) == abi.ERR_ARG and "outside" in abi.last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
def _linreg(nchains):
    import fmcmc_amd as f
    from conftest import synth_linreg
    X, y = synth_linreg(200, 3, 31)
    rng = np.random.default_rng(32)
    init = np.array([3.0, 2.0, -1.0, 0.5, 4.0])[None, :] + 1.5 * rng.standard_normal((nchains, 5))
    init[:, -1] = np.abs(init[:, -1]) + 1.0
    return f, f.gaussian_linreg(X, y), init


def _host_ess(data):
    """min(bulk, tail) [p] of ess_host on data [C][N][p], and per column the larger of the bounds of the three series behind
    it (a minimum of numbers moves by no more than they do); every cut must be safe"""
    from fmcmc_amd import ess_host
    from fmcmc_amd.convergence import split_chains
    host = ess_host(data)
    sp = split_chains(data)
    tol = np.zeros(data.shape[2])
    for j in range(data.shape[2]):
        series, _ = ec.series_of(sp[:, :, j])
        for kind in range(3):
            r = ec.host_case(series[kind], kind)
            assert r.gap > 0.0, (j, kind, r.gap)
            tol[j] = max(tol[j], r.bound)
    return host, np.minimum(host.bulk, host.tail), tol


def test_ess_of_a_run_equals_the_host():
    f, fun, init = _linreg(4)
    ans = f.MCMC(init, fun, 2000, seed=33, nchains=4, kernel=f.kernel_normal(scale=0.1), _return_device=True)
    d = f.ess(ans)
    assert (d.nchains, d.niter, d.start, d.end) == (4, 2000, 1, 2000) and d.bulk.shape == (5,) and d.lags.shape == (5, 4)
    data = ans.to_host().as_array()
    host, least, tol = _host_ess(data)
    print("device", d.bulk, d.tail, "host", host.bulk, host.tail, "bound", tol)
    assert (np.abs(d.bulk - host.bulk) <= tol).all() and (np.abs(d.tail - host.tail) <= tol).all()
    assert np.array_equal(d.lags, host.lags)
    assert np.array_equal(_bits(d.q05), _bits(host.q05)) and np.array_equal(_bits(d.q95), _bits(host.q95))
    assert np.allclose(d.mean, host.mean, rtol=1e-9) and np.allclose(d.mcse_mean, host.mcse_mean, rtol=1e-9)
    e = ans.ess()
    g = f.ess(ans.to_host())
    for name in ("bulk", "tail", "mean", "mcse_mean", "q05", "q95", "tau_bulk"):
        assert np.array_equal(_bits(getattr(e, name)), _bits(getattr(d, name))), name
        assert np.array_equal(_bits(getattr(g, name)), _bits(getattr(d, name))), name
    half = f.ess(ans, autoburnin=True)
    assert (half.niter, half.start, half.end) == (1000, 1001, 2000) and "Bulk" in str(half)


class _HostRecorder:
    """a checker that never stops: ess_host on the copied window after every bulk"""
    freq = 500

    def __init__(self):
        self.values, self.bounds, self.msg = [], [], ""

    def flush(self):
        pass

    def check_device(self, chains, cols, group=None):
        from fmcmc_amd.convergence import _window
        row0, N = _window(chains.iters)
        data = np.ascontiguousarray(chains.samples.cpu().numpy()[:, np.asarray(cols), row0:row0 + N].transpose(0, 2, 1))
        _, least, tol = _host_ess(data)
        at = int(np.argmin(least))
        self.values.append(float(least[at]))
        self.bounds.append(float(tol.max()))
        return False


def test_the_checker_stops_at_the_bulk_the_host_says():
    f, fun, init = _linreg(4)
    rec = _HostRecorder()
    kw = dict(seed=34, nchains=4)
    f.MCMC(init, fun, 2000, conv_checker=rec, kernel=f.kernel_normal(scale=0.1), **kw)
    v = rec.values
    assert len(v) == 4
    stop = next((b for b in range(1, 4) if v[b] > max(v[:b])), None)
    assert stop is not None, v                       # the window grows: so does its smallest ESS
    t = 0.5 * (v[stop] + max(v[:stop]))
    assert t - max(v[:stop]) > 10 * max(rec.bounds) and v[stop] - t > 10 * max(rec.bounds), (v, rec.bounds)
    chk = f.convergence_rhat(freq=500, threshold=1e6, min_ess=t)
    ans = f.MCMC(init, fun, 2000, conv_checker=chk, kernel=f.kernel_normal(scale=0.1), **kw)
    print("host", v, "device", [float(np.min(h[3])) for h in chk.history], "min_ess", t)
    assert len(chk.history) == stop + 1 and ans.niter == 500 * (stop + 1)
    for b, h in enumerate(chk.history):
        assert len(h) == 4 and h[0] == 500 * (b + 1) and abs(float(np.min(h[3])) - v[b]) <= rec.bounds[b], (b, h[3], v[b])
    assert chk.msg == "Rank-normalised split R-hat: %.4f. Smallest ESS: %.1f." % (chk.last, float(np.min(chk.history[-1][3])))
    # m n log10(m n) bounds every ESS (the floor of tau): a demand above it is never met
    never = f.convergence_rhat(freq=500, threshold=1e6, min_ess=8000.0 * np.log10(8000.0) + 1.0)
    ans = f.MCMC(init, fun, 2000, conv_checker=never, kernel=f.kernel_normal(scale=0.1), **kw)
    assert ans.niter == 2000 and len(never.history) == 4
    for b, h in enumerate(never.history):
        assert abs(float(np.min(h[3])) - v[b]) <= rec.bounds[b]
