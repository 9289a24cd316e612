"""The device-wide radix sort, the pooled ranks and the rank-normalised split R-hat on the GPU (csrc/diag_rank.hpp): ranks and
scores bit for bit against scipy's rankdata and the oracle's qnorm, the reduction against np.longdouble under the bounds of
tests/rhat_cases.py, the equalities a deterministic integer sort owes, and rhat() / convergence_rhat end to end.  The raw entries
are called with NaN-filled buffers GUARD elements longer than documented (tests/diag_dev.py), which must stay NaN."""
import functools

import numpy as np
import pytest

import rhat_cases as rc
from gelman_dev import GUARD

pytestmark = pytest.mark.gpu

T = 4096                            # elements of a tile of the sort (RT, csrc/diag_rank.hpp)
NCOLS = 6


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ raw calls
def raw(entry, x, row0, N, cols, mid=(), stream=None, stage=None):
    """L.fmcmc_rank_<entry>_dev on x [C][k][S]: (work, out[, info]) NaN-filled and GUARD longer than documented; returns out
    (and info) at their documented lengths.  stream: a torch stream to enqueue on; stage(): returns the device input, which is then filled
    on that stream in front of the call."""
    import torch
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    Cn, k, S = x.shape
    p, nh = len(cols), N // 2
    lens = [L.fmcmc_rank_work_len(Cn, p, N)] + ([p * 2 * Cn * nh, 2 * p] if entry == "scores"
                                                else [L.fmcmc_rank_rhat_out_len(Cn, p)])
    assert lens[0] > 0
    nan = lambda n: torch.full((int(n) + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    bufs = [nan(n) for n in lens]
    cd = torch.as_tensor(np.asarray(cols, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    xd = torch.as_tensor(x).cuda() if stage is None else stage()
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        if stage is not None:
            xd.copy_(torch.as_tensor(x).pin_memory(), non_blocking=True)
        rcode = getattr(L, "fmcmc_rank_%s_dev" % entry)(xd.data_ptr(), Cn, k, S, row0, N, cd.data_ptr(), p, *mid,
                                                        *[b.data_ptr() for b in bufs], st.cuda_stream)
    assert rcode == abi.OK, (rcode, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    assert all(np.isnan(h[int(n):]).all() for h, n in zip(host, lens))          # nothing past the documented lengths
    if entry == "scores":
        return host[1][:lens[1]].reshape(p, 2 * Cn, nh), host[2][:lens[2]].reshape(p, 2)
    return host[1][:lens[1]].reshape(p, 8 * Cn + 2)


def split(x, row0, N, col):
    """[2 C][N'] of column col of the window, as the definition splits it"""
    nh = N // 2
    w = x[:, col, row0:row0 + N]
    return np.stack([w[:, :nh], w[:, N - nh:]], axis=1).reshape(2 * x.shape[0], nh)


def twice_ranks(v):
    from scipy.stats import rankdata
    return (2.0 * rankdata(v.ravel() + 0.0, method="average")).reshape(v.shape)


def pooled_median(v):
    srt = np.sort(v.ravel() + 0.0)
    return (srt[v.size // 2 - 1] + srt[v.size // 2]) / 2.0


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(Cn, N, seed, row0=3):
    """x [C][6][S], S odd with rows on both sides of the window [row0, row0 + N), the columns:
    0  MH-like: a value is repeated while a step is rejected (runs of ties, the same values in no other chain)
    1  six values in ten are 0.25: one run of equal keys that covers six tenths of the sorted array (more than three tiles
       from M = 20480 on) and starts and ends inside tiles; the rest is noise around it
    2  all equal
    3  both signs, magnitudes from subnormals to 1e300: every digit pass moves keys
    4  1 + j 2^-52, j < 2^16: the six upper bytes of every key are the same, six passes see one digit
    5  -0.0 beside +0.0, and a few -1.0 / 1.0"""
    rng = np.random.default_rng(seed)
    S = row0 + N + 2
    S += 1 - S % 2
    x = np.empty((Cn, NCOLS, S))
    prop = rng.standard_normal((Cn, S))
    keep = rng.uniform(size=(Cn, S)) < 0.7
    keep[:, 0] = False
    idx = np.maximum.accumulate(np.where(keep, 0, np.arange(S)[None, :]), axis=1)
    x[:, 0] = np.take_along_axis(prop, idx, axis=1)
    x[:, 1] = np.where(rng.uniform(size=(Cn, S)) < 0.6, 0.25, 0.25 + rng.standard_normal((Cn, S)))
    x[:, 2] = -7.5
    x[:, 3] = rng.choice([-1.0, 1.0], size=(Cn, S)) * 10.0 ** rng.uniform(-320.0, 300.0, size=(Cn, S))
    x[:, 4] = 1.0 + rng.integers(0, 1 << 16, size=(Cn, S)) * 2.0 ** -52
    x[:, 5] = rng.choice([-0.0, 0.0, -0.0, 0.0, 1.0, -1.0], size=(Cn, S))
    return np.ascontiguousarray(x), row0


# (C, N): M = 2 C floor(N / 2) is even, so the edges of a tile are M = T - 2, T, T + 2 and 2 T + 2 (an odd M does not exist);
# M = 4 and 8; every C of {1, 2, 3, 7} with every N of {4, 5, 1025, 1026} at least once; 28000 values for the run of column 1
# over more than three tiles; 16 x 65537 = 2^20 + 16 values in 257 tiles, one more than a chunk of the scan of the tile table.
SHAPES = [(1, 4), (2, 4), (1, 5), (3, 5), (7, 4), (7, 5), (2, 1025), (3, 1026), (7, 1025), (7, 1026), (1, 1026), (1, T - 1),
          (2, T // 2), (3, (T + 2) // 3 + 1), (1, 2 * T + 2), (7, 4001), (8, 131075)]


def test_the_shapes_are_the_edges_they_claim():
    M = {2 * c * (n // 2) for c, n in SHAPES}
    assert {4, 8, T - 2, T, T + 2, 2 * T + 2, 28000, (1 << 20) + 16} <= M
    assert -(-((1 << 20) + 16) // T) == 257


@functools.lru_cache(maxsize=None)
def ranks_case(Cn, N):
    """one fmcmc_rank_scores_dev call per (what, fold) on the six columns: the device arrays and the input, shared by the tests"""
    x, row0 = make_inputs(Cn, N, 100 * Cn + N)
    cols = tuple(range(NCOLS))
    got = {(what, fold): raw("scores", x, row0, N, cols, (fold, what)) for what in (1, 0) for fold in (0, 1)
           if (Cn, N) != (8, 131075) or (what, fold) == (1, 0)}
    return x, row0, got


@pytest.mark.parametrize("Cn, N", SHAPES)
def test_ranks_bit_for_bit(Cn, N):
    x, row0, got = ranks_case(Cn, N)
    out, info = got[(1, 0)]
    for j in range(NCOLS):
        v = split(x, row0, N, j)
        assert np.array_equal(_bits(out[j]), _bits(twice_ranks(v))), j
        assert info[j, 0] == 0.0 and _bits(info[j, 1]) == _bits(pooled_median(v)), j


def test_ranks_of_make_series_bit_for_bit():
    """the inputs the other diagnostics share (column 0 has ties), at their own row0, odd S and column order"""
    import diag_dev as dd
    for N in (1025, 1367):
        x = dd.make_series(N, 5000 + N)
        out, _ = raw("scores", x, dd.ROW0, N, dd.COLS, (0, 1))
        for j, col in enumerate(dd.COLS):
            assert np.array_equal(_bits(out[j]), _bits(twice_ranks(split(x, dd.ROW0, N, col)))), (N, col)


SCORE_SHAPES = [(2, 4), (3, 5), (7, 1025), (3, (T + 2) // 3 + 1), (7, 4001)]


@pytest.mark.parametrize("Cn, N", SCORE_SHAPES)
def test_scores_bit_for_bit(O, Cn, N):
    """z against the oracle's fmh_qnorm (the same header, -ffp-contract=off) of (r - 0.375) / (M + 0.25) formed in float64"""
    x, row0, got = ranks_case(Cn, N)
    M = 2 * Cn * (N // 2)
    for fold in (0, 1):
        z, _ = got[(0, fold)]
        twice, _ = got[(1, fold)]
        arg = np.ascontiguousarray((0.5 * twice - 0.375) / (M + 0.25))
        want = np.empty_like(arg)
        O.lib().fmcmc_oracle_detmath(3, O._p(arg.ravel()), O._p(want.reshape(-1)), arg.size)
        assert np.array_equal(_bits(z), _bits(want)), fold


@pytest.mark.parametrize("Cn, N", SCORE_SHAPES)
def test_folded_ranks_bit_for_bit(Cn, N):
    x, row0, got = ranks_case(Cn, N)
    out, info = got[(1, 1)]
    for j in range(NCOLS):
        v = split(x, row0, N, j)
        med = pooled_median(v)
        assert _bits(info[j, 1]) == _bits(med), j
        assert np.array_equal(_bits(out[j]), _bits(twice_ranks(np.abs(v - med)))), j


# ------------------------------------------------------------------------------------------------ the reduction and R-hat
@pytest.mark.parametrize("Cn, N", [(2, 4), (3, 5), (7, 1025), (7, 4001)])
def test_moments_and_rhat_within_the_derived_bounds(Cn, N):
    """fmcmc_rank_rhat_dev's means and variances against np.longdouble moments of the bit-exact scores, within
    rhat_cases.moment_bounds (derived from the documented order of the sums, not from what the kernel returns); then
    rhat_finish against rhat_host within rhat_cases.rhat_bound, the score difference between fmh_qnorm and ndtri included."""
    from fmcmc_amd import rhat_host
    from fmcmc_amd.summary import rhat_finish
    x, row0, got = ranks_case(Cn, N)
    nh, m = N // 2, 2 * Cn
    out = raw("rhat", x, row0, N, tuple(range(NCOLS)))
    fin = rhat_finish(out, Cn, nh)
    host = rhat_host(np.ascontiguousarray(x[:, :, row0:row0 + N].transpose(0, 2, 1)))
    mom = out[:, :4 * m].reshape(NCOLS, 2, m, 2)
    for j in range(NCOLS):
        assert out[j, 4 * m] == 0.0 and _bits(out[j, 4 * m + 1]) == _bits(host.median[j]), j
        for fold, name in enumerate(("bulk", "tail")):
            z = got[(0, fold)][0][j].astype(np.longdouble)
            e_mean, e_var = rc.moment_bounds(z)
            mean, var = z.mean(axis=1), z.var(axis=1, ddof=1)
            dm = np.abs(mom[j, fold, :, 0] - mean).astype(np.float64)
            dv = np.abs(mom[j, fold, :, 1] - var).astype(np.float64)
            print("col %d %s: |mean err| %.3g (bound %.3g)  |var err| %.3g (bound %.3g)"
                  % (j, name, dm.max(), e_mean.max(), dv.max(), e_var.max()))
            assert (dm <= e_mean).all() and (dv <= e_var).all(), (j, name)
            want, have = getattr(host, name)[j], getattr(fin, name)[j]
            if var.sum() == 0:                       # the constant column (and a fold that makes one)
                assert np.isnan(have) and np.isnan(want), (j, name)
                continue
            s_mean, s_var = rc.score_shift_bounds(z)
            tol = rc.rhat_bound(mean, var, e_mean + s_mean, e_var + s_var, nh)
            print("col %d %s: device %.17g host %.17g  |diff| %.3g (bound %.3g)" % (j, name, have, want, abs(have - want), tol))
            assert abs(have - want) <= tol, (j, name)
        assert np.isnan(fin.rhat[j]) if np.isnan(host.rhat[j]) else fin.rhat[j] == max(fin.bulk[j], fin.tail[j])


def _device_rhat(data):
    import fmcmc_amd as f
    Cn, N, p = data.shape
    ml = f.McmcList([f.Mcmc(data[c], start=1, end=N, thin=1) for c in range(Cn)])
    return f.rhat(ml)


def test_the_constructed_cases_hold_on_the_device():
    x = rc.identical_chains()
    nh = x.shape[1] // 2
    d = _device_rhat(x)
    want = float(np.sqrt(np.longdouble(nh - 1) / np.longdouble(nh)))
    assert d.bulk[0] == want and d.tail[0] == want and d.rhat[0] == want and (d.nchains, d.niter) == (4, 100)
    d = _device_rhat(rc.shifted_chains())
    assert d.bulk[0] > 1.5 and d.tail[0] < 1.05 and d.rhat[0] == d.bulk[0]
    d = _device_rhat(rc.scaled_chains())
    assert d.bulk[0] < 1.05 and d.tail[0] > 1.2 and d.rhat[0] == d.tail[0]
    x = np.random.default_rng(22).standard_normal((2, 31, 2))
    x[:, :, 1] = 3.25
    d = _device_rhat(x)
    assert np.isnan(d.rhat[1]) and d.median[1] == 3.25 and np.isfinite(d.rhat[0]) and "NA" in str(d)
    y = x.copy()
    y[:, 15, :] = 1e6                                # the middle row of an odd window takes part in nothing
    e = _device_rhat(y)
    assert np.array_equal(_bits(d.bulk), _bits(e.bulk)) and np.array_equal(_bits(d.median), _bits(e.median))


# ------------------------------------------------------------------------------------------------ equalities, bit for bit
EQ = (3, 2 * T + 15)                # three tiles and a part


def test_two_launches_agree():
    x, row0 = make_inputs(*EQ, seed=7)
    a = raw("rhat", x, row0, EQ[1], (0, 3, 5))
    b = raw("rhat", x, row0, EQ[1], (0, 3, 5))
    assert np.array_equal(_bits(a), _bits(b))
    za, _ = raw("scores", x, row0, EQ[1], (0, 3, 5), (1, 0))
    zb, _ = raw("scores", x, row0, EQ[1], (0, 3, 5), (1, 0))
    assert np.array_equal(_bits(za), _bits(zb))


def test_the_window_elsewhere_in_another_history():
    Cn, N = EQ
    x, row0 = make_inputs(Cn, N, seed=8)
    S2 = N + 40
    S2 += 1 - S2 % 2
    y = np.full((Cn, NCOLS + 2, S2), np.nan)
    y[:, 1:1 + NCOLS, 17:17 + N] = x[:, :, row0:row0 + N]
    y[:, :, :17] = 1e9
    y[:, :, 17 + N:] = -1e9
    a = raw("rhat", x, row0, N, (0, 1, 4))
    b = raw("rhat", y, 17, N, (1, 2, 5))
    assert x.shape[2] != S2 and S2 % 2 == 1 and np.array_equal(_bits(a), _bits(b))


def test_a_column_alone_and_among_three_in_another_order():
    x, row0 = make_inputs(*EQ, seed=9)
    three = raw("rhat", x, row0, EQ[1], (3, 0, 1))
    for j, col in enumerate((3, 0, 1)):
        alone = raw("rhat", x, row0, EQ[1], (col,))
        assert np.array_equal(_bits(alone[0]), _bits(three[j])), col
    z3, i3 = raw("scores", x, row0, EQ[1], (3, 0, 1), (1, 0))
    z1, i1 = raw("scores", x, row0, EQ[1], (0,), (1, 0))
    assert np.array_equal(_bits(z1[0]), _bits(z3[1])) and np.array_equal(_bits(i1[0]), _bits(i3[1]))


def test_a_side_stream_behind_a_busy_stream():
    """the rows reach the device ON the side stream, behind a kernel that keeps it busy: a call that left its caller's stream
    would read the NaN prefill"""
    import torch
    x, row0 = make_inputs(*EQ, seed=10)
    want = raw("rhat", x, row0, EQ[1], (0, 3, 5))
    side = torch.cuda.Stream()

    def stage():
        xd = torch.full(x.shape, float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(4_000_000)             # a few milliseconds
        return xd

    got = raw("rhat", x, row0, EQ[1], (0, 3, 5), stream=side, stage=stage)
    assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------ non-finite values
def test_non_finite_values_are_counted_and_refused():
    import diag_dev as dd
    import fmcmc_amd as f
    N = 1025
    x = dd.make_series(N, 77, non_finite=True)       # one NaN and one infinity in chain 1, column 2
    _, info = raw("scores", x, dd.ROW0, N, dd.COLS, (0, 1))
    assert info[:, 0].tolist() == [2.0, 0.0, 0.0]    # COLS = (2, 0, 3)
    out = raw("rhat", x, dd.ROW0, N, dd.COLS)
    assert out[:, 8 * dd.CHAINS].tolist() == [2.0, 0.0, 0.0]
    w = x[:, :, dd.ROW0:dd.ROW0 + N]
    ml = f.McmcList([f.Mcmc(w[c].T.copy(), start=1, end=N, thin=1) for c in range(dd.CHAINS)])
    with pytest.raises(ValueError, match=r"2 non-finite value\(s\) among the rows to rank \(columns \[2\]\)"):
        f.rhat(ml)
    with pytest.raises(ValueError, match=r"columns \[2\]"):
        f.rank_scores(ml, cols=[0, 2])
    assert np.isfinite(f.rhat(ml, cols=[0, 1, 3]).rhat).all()


# ------------------------------------------------------------------------------------------------ end to end
def _linreg():
    import fmcmc_amd as f
    from conftest import synth_linreg
    X, y = synth_linreg(200, 3, 31)
    rng = np.random.default_rng(32)
    init = np.array([3.0, 2.0, -1.0, 0.5, 4.0])[None, :] + 1.5 * rng.standard_normal((8, 5))
    init[:, -1] = np.abs(init[:, -1]) + 1.0
    return f, f.gaussian_linreg(X, y), init


def _host_bound(data, rhat):
    """|device - host| of rhat on data [C][N][p]: rhat_cases.rhat_bound of the host's own scores, per column the larger of bulk
    and tail (the maximum of two numbers moves by no more than they do)"""
    from fmcmc_amd.convergence import rank_z, split_chains
    sp = split_chains(data)
    nh = sp.shape[1]
    tol = np.zeros(data.shape[2])
    for j in range(data.shape[2]):
        v = sp[:, :, j]
        for w in (v, np.abs(v - pooled_median(v))):
            z = rank_z(w)[0].astype(np.longdouble)
            e_mean, e_var = rc.moment_bounds(z)
            s_mean, s_var = rc.score_shift_bounds(z)
            tol[j] = max(tol[j], rc.rhat_bound(z.mean(axis=1), z.var(axis=1, ddof=1), e_mean + s_mean, e_var + s_var, nh))
    return tol


def test_rhat_of_a_run_equals_the_host():
    f, fun, init = _linreg()
    ans = f.MCMC(init, fun, 2000, seed=33, nchains=8, kernel=f.kernel_normal(scale=0.1), _return_device=True)
    d = f.rhat(ans)
    assert d is not None and (d.nchains, d.niter) == (8, 2000) and d.bulk.shape == (5,)
    data = ans.to_host().as_array()
    host = f.rhat_host(data)
    tol = _host_bound(data, host.rhat)
    print("device", d.rhat, "host", host.rhat, "bound", tol)
    assert (np.abs(d.rhat - host.rhat) <= tol).all() and np.array_equal(_bits(d.median), _bits(host.median))
    assert np.array_equal(_bits(ans.rhat().rhat), _bits(d.rhat))
    z = ans.rank_scores(cols=[1])
    assert tuple(z.shape) == (1, 16, 1000) and bool(z.isfinite().all()) and float(z.abs().max()) < 4.5
    half = f.rhat(ans, autoburnin=True)
    assert (half.niter, half.start, half.end) == (1000, 1001, 2000)


class _HostRecorder:
    """a checker that never stops: rhat_host on the copied history after every bulk"""
    freq = 500

    def __init__(self):
        self.values, self.bounds, self.msg = [], [], ""

    def flush(self):
        pass

    def check_device(self, chains, cols, group=None):
        import fmcmc_amd as f
        from fmcmc_amd.convergence import _window
        row0, N = _window(chains.iters)
        data = np.ascontiguousarray(chains.samples.cpu().numpy()[:, np.asarray(cols), row0:row0 + N].transpose(0, 2, 1))
        host = f.rhat_host(data)
        self.values.append(float(host.rhat.max()))
        self.bounds.append(float(_host_bound(data, host.rhat).max()))
        return False


def test_the_checker_stops_where_the_host_says():
    f, fun, init = _linreg()
    rec = _HostRecorder()
    kw = dict(seed=34, nchains=8)                    # (a kernel carries its state from call to call: a fresh one per run)
    f.MCMC(init, fun, 2000, conv_checker=rec, kernel=f.kernel_normal(scale=0.1), **kw)
    v = rec.values
    assert len(v) == 4
    stop = next((b for b in range(1, 4) if v[b] < min(v[:b])), None)
    assert stop is not None, v                       # dispersed starts: the statistic falls
    t = 0.5 * (v[stop] + min(v[:stop]))
    assert min(v[:stop]) - t > 10 * max(rec.bounds) and t - v[stop] > 10 * max(rec.bounds), (v, rec.bounds)
    chk = f.convergence_rhat(freq=500, threshold=t)
    ans = f.MCMC(init, fun, 2000, conv_checker=chk, kernel=f.kernel_normal(scale=0.1), **kw)
    print("host", v, "device", [h[1] for h in chk.history], "threshold", t)
    assert len(chk.history) == stop + 1 and ans.niter == 500 * (stop + 1)
    assert [h[0] for h in chk.history] == [500 * (b + 1) for b in range(stop + 1)]
    for b, h in enumerate(chk.history):
        assert abs(h[1] - v[b]) <= rec.bounds[b], (b, h[1], v[b])
    assert chk.last == chk.history[-1][1] and chk.msg == "Rank-normalised split R-hat: %.4f." % chk.last
