"""GPU tests of the device-side summary (csrc/summary.hip) at its shape edges: AR orders up to 64, the groups of eight lags,
the 19456-row LDS tile and its halo, the shortest series and the load strides, 0 to 16 quantiles, 256 columns, the key order
of the radix select, and what must not depend on where a series sits in the launch.

Yardsticks beyond those of tests/test_gpu_summary.py (whose helpers are used here):
 * inputs whose selected AR order is the largest one (`seasonal`: x_t = phi x_{t-lag} + e_t with lag = M or M - 2), so that
   spec0 depends on every autocovariance r_0 .. r_M; tests/test_summary_host.py proves order and AIC gap from the reference;
 * the autocovariances themselves, read from the work buffer, against longdouble within a bound that holds for any kernel
   that centres on a float64 mean and sums fma products in some order (`check_acov`; nothing of the device enters the bound);
 * the tolerance of spec0 / ESS / time-series SE follows the rule of test_gpu_summary.py (16 x the worst float64-vs-longdouble
   distance of host restatements) with one more float64 member whose sums run as a device's do (`strided_sum`);
 * bit-for-bit equalities that need no tolerance: placement in the launch, window against upload, reductions;
 * order statistics against a sort of order-preserving integer keys where np.sort is not defined (-0.0 beside +0.0).
Measured distances (MI355X): DESIGN.md section 5.10.
"""
import numpy as np
import pytest

from test_gpu_summary import LD, U, _bits, ar1, check_exact, check_moments, check_series, host_series, upload

pytestmark = pytest.mark.gpu
LDS_ROWS = 19456        # csrc/summary.hip: rows of a series staged in LDS at once
DEFAULT = (0.025, 0.25, 0.5, 0.75, 0.975)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------ inputs
def order_max(N):
    """The largest AR order stats::ar tries: min(N - 1, floor(10 log10 N))."""
    return int(min(N - 1, np.floor(10 * np.log10(N))))


def first_n_of_order(M):
    """The smallest N with floor(10 log10 N) = M."""
    N = int(np.ceil(10.0 ** (M / 10.0)))
    while order_max(N) < M:
        N += 1
    while order_max(N - 1) >= M:
        N -= 1
    return N


def seasonal(N, lag, rng, phi=0.6, mu=0.0):
    """x_t = phi x_{t-lag} + e_t, started from its stationary law; one vector step per block of `lag` rows."""
    nb = -(-N // lag)
    x = rng.standard_normal((nb, lag))
    x[0] /= np.sqrt(1.0 - phi * phi)
    for b in range(1, nb):
        x[b] += phi * x[b - 1]
    return x.ravel()[:N] + mu


def length_case(N, nchains=2):
    """The two columns of the series-length tests, [nchains][N][2], and the lag each series is built with, which the
    order that the longdouble reference selects must reach (None below 100 rows: AR(1) inputs, whatever small order wins)."""
    M = order_max(N)
    rng = np.random.default_rng(77000000 + N)
    if N < 100:
        arr = np.stack([np.stack([ar1(0.9, N, rng, mu=3.0), ar1(0.3, N, rng, mu=-2.0)], axis=1) for _ in range(nchains)])
        return arr, None
    arr = np.stack([np.stack([seasonal(N, M, rng, mu=3.0), seasonal(N, M - 2, rng, mu=-2.0)], axis=1) for _ in range(nchains)])
    if N > LDS_ROWS:            # the largest products of the series cross the boundary between the first two tiles
        arr[:, LDS_ROWS - 1, :] += 25.0
        for row in sorted({min(LDS_ROWS + 7, N - 1), min(LDS_ROWS + 41, N - 1)}):
            arr[:, row, :] -= 25.0
    return arr, [M, M - 2] * nchains


def big_case(N):
    """One chain, one column, lag = M (M = 63 or 64): [1][N][1]."""
    M = order_max(N)
    return seasonal(N, M, np.random.default_rng(77000000 + N), mu=3.0)[None, :, None], [M]


SHORT = (3, 4, 5, 6, 10, 11, 12)
STRIDES = (63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193)
GROUP_EDGES = (16, 24, 32, 40, 48, 56)
TILE_EDGES = (LDS_ROWS - 1, LDS_ROWS, LDS_ROWS + 1, LDS_ROWS + 41, LDS_ROWS + 42, LDS_ROWS + 43, LDS_ROWS + 44, 2 * LDS_ROWS,
              2 * LDS_ROWS + 1)
BIG = (2511886, 2511887, 3162277)       # M = 63, 64 and the largest supported length (M = 64)


def width_case(k, N=600, nchains=2, seed=258):
    """[nchains][N][k] AR(1) columns with phi spread over [0, 0.95] and means spread over [-4, 4].  (Among 512 series one in two
    or three seeds has a series whose two best AIC values lie within 1e-3; the default seed and 65 have none, which
    tests/test_summary_host.py asserts.)"""
    rng = np.random.default_rng(seed)
    phi = np.tile(np.linspace(0.0, 0.95, k), (nchains, 1))
    e = rng.standard_normal((N, nchains, k))
    x = np.empty((N, nchains, k))
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for i in range(1, N):
        x[i] = phi * x[i - 1] + e[i]
    return np.ascontiguousarray(x.transpose(1, 0, 2)) + np.linspace(-4.0, 4.0, k)


# ------------------------------------------------------------------------------------------------ host references
def strided_sum(v):
    """A float64 sum shaped like a device's: 512 interleaved sequential chains (element i goes to chain i mod 512), joined by
    a pairwise tree."""
    v = np.asarray(v)
    full = v.size // 512 * 512
    w = np.zeros(512, dtype=v.dtype)
    if full:
        w += np.add.reduce(v[:full].reshape(-1, 512), axis=0)      # down the rows, one after the other, as np.cumsum would
    w[:v.size - full] += v[full:]
    while w.size > 1:
        w = w[0::2] + w[1::2]
    return w[0]


def restate(y, dtype=LD, ssum=None, acov=False):
    """host_series of test_gpu_summary.py (the same statements in the same order) with the summation left open; with
    `acov` it also returns what check_acov needs: the centred series xc, r_l = sum(xc_i xc_{i+l}) / n and sum |xc_i xc_{i+l}|."""
    y = np.asarray(y).astype(dtype)
    n = y.size
    ssum = ssum or (lambda v: v.sum())
    mean = ssum(y) / dtype(n)
    x = y - mean
    var = ssum(x * x) / dtype(n - 1)
    tc = np.arange(n).astype(dtype)
    tc = tc - ssum(tc) / dtype(n)
    slope = ssum(tc * x) / ssum(tc * tc)
    res = x - slope * tc
    res = res - ssum(res) / dtype(n)
    out = dict(mean=mean, var=var, spec0=dtype(0), order=0, gap=np.inf)
    if np.sqrt(ssum(res * res) / dtype(n - 1)) < 1.5e-8:
        return out
    del tc, res
    M = order_max(n)
    r = np.empty(M + 1, dtype=dtype)
    absr = np.empty(M + 1, dtype=dtype)
    x64 = x.astype(np.float64)
    for l in range(M + 1):
        r[l] = ssum(x[:n - l] * x[l:])
        if acov:                                  # (the size of a bound: float64 is plenty)
            absr[l] = np.abs(x64[:n - l] * x64[l:]).sum()
    r = r / dtype(n)
    coefs = np.zeros((M + 1, M + 1), dtype=dtype)
    v = np.empty(M + 1, dtype=dtype)
    v[0] = r[0]
    for m in range(1, M + 1):
        acc = r[m] - ssum(coefs[m - 1, 1:m] * r[m - 1:0:-1])
        phi = acc / v[m - 1]
        coefs[m, m] = phi
        coefs[m, 1:m] = coefs[m - 1, 1:m] - phi * coefs[m - 1, m - 1:0:-1]
        v[m] = v[m - 1] * (1 - phi * phi)
    aic = dtype(n) * np.log(v) + 2 * np.arange(M + 1) + 2
    o = int(np.argmin(aic))
    srt = np.sort(aic)
    var_pred = v[o] * dtype(n) / dtype(n - (o + 1))
    out.update(spec0=var_pred / (1 - ssum(coefs[o, 1:o + 1])) ** 2, order=o, gap=float(srt[1] - srt[0]))
    if acov:
        out.update(xc=x, r=r, absr=absr)
    return out


def edge_tolerance(columns, label, acov=True):
    """spec0_tolerance of test_gpu_summary.py with a third float64 member, the restatement summed by `strided_sum`: 16 x the
    worst relative distance of the float64 family from the longdouble restatement over `columns`, and the longdouble
    references (with the autocovariances).  Prints the distance of each member."""
    from fmcmc_amd.convergence import spectrum0_ar
    worst, refs, flips = np.zeros(3), [], 0
    for y in columns:
        ref = restate(y, LD, acov=acov)
        refs.append(ref)
        if ref["spec0"] == 0:
            continue
        s_a, o_a = spectrum0_ar(y)
        b = host_series(y, np.float64, flip=True)
        c = restate(y, np.float64, ssum=strided_sum)
        flips += (o_a != ref["order"]) + (b["order"] != ref["order"]) + (c["order"] != ref["order"])
        for i, s in enumerate((s_a, b["spec0"], c["spec0"])):
            worst[i] = max(worst[i], float(abs(LD(s) - ref["spec0"]) / ref["spec0"]))
    tol = 16 * float(worst.max())
    print("\n[%s] %d series: float64-vs-longdouble relative distance of spec0: package %.3g, reversed %.3g, strided %.3g -> "
          "tolerance %.3g; smallest AIC gap %.3g; float64 / longdouble host orders differ %d times"
          % (label, len(refs), worst[0], worst[1], worst[2], tol, min(r["gap"] for r in refs), flips))
    return tol, refs


def check_reference(refs, lags, label):
    """What the inputs must guarantee, from the reference alone: the selected order is at least the lag the series is built
    with (M or M - 2: spec0 then needs the autocovariances of the last group of lags; with lag = M - 2 an AR(M - 1) or AR(M)
    fit wins the AIC by chance in about a quarter of the series, as a chi-square of one or two degrees exceeds 2 or 4), an AIC
    gap that no float64 evaluation closes, and that check_series leaves out no series."""
    for i, ref in enumerate(refs):
        assert ref["spec0"] != 0 and np.isfinite(float(ref["spec0"])), (label, i)
        assert ref["gap"] >= 1e-3, (label, i, ref["gap"])
        if lags is not None:
            assert lags[i] <= ref["order"], (label, i, ref["order"], lags[i])


def check_acov(slots, host, cols, refs):
    """slots [C p][72]: the per-series head of the work buffer.  Every r_l, l <= M, against longdouble within
        (N + 2) u sum|xc_i xc_{i+l}| / N  +  d (|sum_{i<N-l} xc_i| + |sum_{i>=l} xc_i|) / N  +  d^2,   d = N u mean|x|:
    the centred products summed in any order with fma (two roundings of the centring, one of each product or fma, fewer than
    N of the sum, one of the division), plus what a mean that is off by at most d -- the worst error of a float64 mean --
    moves the sum.  m, xc and the sums come from the longdouble reference.  Lags above M are exactly 0; the mean within d."""
    from fmcmc_amd.summary import WORK_MAX_ORDER, WORK_MEAN, WORK_NON_FINITE
    C_, _, N = host.shape
    M = order_max(N)
    n, worst = 0, 0.0
    for c in range(C_):
        for col in cols:
            ref, s = refs[n], slots[n]
            n += 1
            d = N * U * np.abs(host[c, col].astype(LD)).mean()
            assert abs(LD(s[WORK_MEAN]) - ref["mean"]) <= d, (c, col)
            assert s[WORK_NON_FINITE] == 0.0
            assert not _bits(s[M + 1:WORK_MAX_ORDER + 1]).any(), (c, col, s[M + 1:WORK_MAX_ORDER + 1])
            cs = np.concatenate([[LD(0)], np.cumsum(ref["xc"])])
            for l in range(M + 1):
                bound = (N + 2) * U * ref["absr"][l] / N + d * (abs(cs[N - l]) + abs(cs[N] - cs[l])) / N + d * d
                err = abs(LD(s[l]) - ref["r"][l])
                worst = max(worst, float(err / bound))
                assert err <= bound, (c, col, l, float(s[l]), float(ref["r"][l]), float(err), float(bound))
    print("autocovariances r_0..r_%d of %d series: worst |device - longdouble| / bound = %.3g" % (M, n, worst))


def key_sort(a):
    """Sorts doubles by the order-preserving integer key of their bits (sign-and-magnitude -> offset binary).  Unlike np.sort,
    which treats the two zeros as equal and leaves their order open, this puts -0.0 below +0.0."""
    u = _bits(a).ravel()
    neg = (u >> np.uint64(63)).astype(bool)
    key = np.sort(np.where(neg, ~u, u | np.uint64(1 << 63)))
    back = np.where((key >> np.uint64(63)).astype(bool), key & np.uint64((1 << 63) - 1), ~key)
    return back.view(np.float64)


# ------------------------------------------------------------------------------------------------ device side
def device_chains(cks, nrows=None):
    """[C][k][capacity] host array -> DeviceChains whose first `nrows` rows are the kept ones."""
    import torch
    from fmcmc_amd import DeviceChains
    cks = np.ascontiguousarray(cks, dtype=np.float64)
    n = cks.shape[2] if nrows is None else nrows
    return DeviceChains(torch.as_tensor(cks).cuda(), None, None, np.arange(1, n + 1), 1, None, 0, cks.shape[0], nrows=n)


def series_slots(dc, cols=None):
    from fmcmc_amd.summary import _columns, _series_work, enqueue_window
    _, _, work, _ = enqueue_window(dc, 0, dc.nrows, cols)
    return _series_work(work, int(dc._samples.shape[0]) * _columns(dc, cols).size).cpu().numpy()


def run_length_case(arr, lags, label, dc=None):
    """Sections 2 and 3 of the module docstring for one input [C][N][k]."""
    dc = upload(arr) if dc is None else dc
    host = dc.samples.cpu().numpy()
    C_, k, N = host.shape
    assert np.array_equal(_bits(host), _bits(arr.transpose(0, 2, 1)))
    tol, refs = edge_tolerance([host[c, j] for c in range(C_) for j in range(k)], label)
    check_reference(refs, lags, label)
    check_acov(series_slots(dc), host, range(k), refs)
    sm, _ = check_exact(dc, DEFAULT)
    check_moments(sm, host, range(k))
    check_series(sm.per_chain, host, list(range(k)), tol, refs)
    assert np.all(np.isfinite(sm.statistics)) and np.all(np.isfinite(sm.quantiles)) and np.all(sm.ess > 0)


# ------------------------------------------------------------------------------------------------ series lengths
@pytest.mark.parametrize("N", SHORT)
def test_short_series_and_the_order_cap(N):
    """M = N - 1 caps the order up to N = 11 (floor(10 log10 N) >= N - 1; at N = 12 it is N - 2); three rows are the minimum."""
    assert order_max(N) == min(N - 1, {3: 4, 4: 6, 5: 6, 6: 7, 10: 10, 11: 10, 12: 10}[N])
    run_length_case(*length_case(N, nchains=3), "N = %d" % N)


def test_two_rows_are_too_short():
    arr, _ = length_case(3)
    with pytest.raises(ValueError, match="too short"):
        upload(arr[:, :2]).summary()
    with pytest.raises(ValueError, match="too short"):
        upload(arr[:, :2]).effective_size()


@pytest.mark.parametrize("N", STRIDES)
def test_lengths_around_the_load_strides(N):
    """Around the 64 lanes, the 512 threads, the 2048-row tile of the histogram kernel and the 8192 rows a batch of the mean
    loop loads; odd N ends the mean loop with half a pair."""
    run_length_case(*length_case(N), "N = %d" % N)


@pytest.mark.parametrize("M", GROUP_EDGES)
def test_orders_at_the_edges_of_the_lag_groups(M):
    """M = 8 g is the first order that needs lag group g; M - 1 is the last one that must not leave a trace of it."""
    N = first_n_of_order(M)
    assert order_max(N) == M and order_max(N - 1) == M - 1 and M % 8 == 0
    if M == 48:
        assert N == 63096
    for n in (N - 1, N):
        run_length_case(*length_case(n), "M = %d, N = %d" % (order_max(n), n))


@pytest.mark.parametrize("N", TILE_EDGES)
def test_lengths_around_the_lds_tile(N):
    """One tile up to 19456 rows; then a second tile of one row, a halo that the end of the series cuts short, a halo that is
    exactly full (N = 19456 + M), one and two rows over, and a third tile of one row.  Spikes on both sides of the first
    boundary make the products that cross it the largest of the series."""
    M = order_max(N)
    assert M == (42 if N < 2 * LDS_ROWS else 45)
    run_length_case(*length_case(N), "N = %d" % N)


@pytest.mark.parametrize("N", BIG)
def test_ar_orders_63_and_64(N):
    """M = 64 runs the 65th accumulator, its own wave sum, out[64] and the Levinson step that broadcasts from lane 63."""
    M = order_max(N)
    assert M == {2511886: 63, 2511887: 64, 3162277: 64}[N]
    arr, lags = big_case(N)
    last = N == BIG[-1]
    dc = device_chains(np.concatenate([arr.transpose(0, 2, 1), np.zeros((1, 1, 1))], axis=2), nrows=N) if last else None
    run_length_case(arr, lags, "M = %d, N = %d" % (M, N), dc)
    if last:                                    # one more row asks for order 65
        from fmcmc_amd.summary import window_stats
        dc.nrows = N + 1
        with pytest.raises(NotImplementedError, match="AR order up to 65"):
            window_stats(dc, 0, N + 1, None, DEFAULT)


# ------------------------------------------------------------------------------------------------ bit for bit
def _chain_fields(pc, c, a):
    return [int(_bits(f[c, a])[0]) for f in (pc.mean, pc.spec0, pc.sd, pc.ess, pc.tsse)] + [int(pc.order[c, a])]


@pytest.mark.parametrize("N", (1025, LDS_ROWS + 1))
def test_a_series_gives_the_same_bits_wherever_it_sits(N):
    """Chain 0 of 1, 2 of 5, 300 of 301 (the pooling kernel strides the chains by 256); column 0 of 1, 3 of 7 under several
    `cols`, also one that names it twice."""
    rng = np.random.default_rng(N)
    M = order_max(N)
    s = seasonal(N, M, rng, mu=3.0)
    base = device_chains(s[None, None, :]).summary(quantiles=())
    want = _chain_fields(base.per_chain, 0, 0)
    assert base.per_chain.order[0, 0] == M
    for nchains, at in ((5, 2), (301, 300)):
        cks = rng.standard_normal((nchains, 1, N))
        cks[at, 0] = s
        assert _chain_fields(device_chains(cks).summary(quantiles=()).per_chain, at, 0) == want, (nchains, at)
    cks = rng.standard_normal((1, 7, N)) * np.arange(1, 8)[None, :, None]
    cks[0, 3] = s
    dc = device_chains(cks)
    for cols, where in (([3], [0]), ([5, 3, 0], [1]), ([3, 3], [0, 1]), (None, [3])):
        pc = dc.summary(quantiles=(0.5,), cols=cols).per_chain
        for a in where:
            assert _chain_fields(pc, 0, a) == want, (cols, a)
    # one chain, one column: the pooled statistics are the chain's
    assert _bits(base.statistics[0, 0]) == _bits(base.per_chain.mean[0, 0]) and _bits(base.ess[0]) == _bits(base.per_chain.ess[0, 0])


@pytest.mark.parametrize("N", (3000, 3001))
def test_a_window_of_a_history_equals_its_rows_uploaded_alone(N):
    """A history with more rows allocated than kept, an odd row stride: the series of a window start at any 8-byte boundary."""
    from fmcmc_amd.summary import window_stats
    rng = np.random.default_rng(N)
    nrows, cap = 7098, 7101
    cks = np.full((2, 2, cap), np.nan)
    for c in range(2):
        cks[c, 0, :nrows] = seasonal(nrows, 20, rng, mu=3.0)
        cks[c, 1, :nrows] = ar1(0.7, nrows, rng, mu=-2.0)
    hist = device_chains(cks, nrows=nrows)
    assert hist.capacity - hist.nrows == 3
    probs = (0.0, 0.025, 0.5, 0.975, 1.0)
    for row0 in (0, 1, 7, 4096):
        alone = device_chains(cks[:, :, row0:row0 + N])
        for cols in (None, [1]):
            a, b = window_stats(hist, row0, N, cols, probs), window_stats(alone, 0, N, cols, probs)
            for x, y in zip(a, b):
                assert np.array_equal(_bits(x), _bits(y)), (row0, cols)
    with pytest.raises(ValueError, match="outside"):
        window_stats(hist, nrows - N + 1, N, None, probs)


def test_reductions_do_not_depend_on_the_quantiles():
    arr, _ = length_case(2049, nchains=3)
    dc = upload(arr)
    ref = dc.summary()
    assert np.array_equal(_bits(dc.effective_size()), _bits(ref.ess))
    assert np.array_equal(_bits(dc.effective_size(cols=[1])), _bits(ref.ess[[1]]))
    for q in ((), (0.5,), tuple(np.linspace(0, 1, 16))):
        sm = dc.summary(quantiles=q)
        assert sm.quantiles.shape == (2, len(q))
        assert np.array_equal(_bits(sm.statistics), _bits(ref.statistics)) and np.array_equal(_bits(sm.ess), _bits(ref.ess))
        for f in ("mean", "sd", "spec0", "ess", "tsse"):
            assert np.array_equal(_bits(getattr(sm.per_chain, f)), _bits(getattr(ref.per_chain, f))), (q, f)
        assert np.array_equal(sm.per_chain.order, ref.per_chain.order)
    assert str(dc.summary(quantiles=())).count("Quantiles") == 0


@pytest.mark.parametrize("N", (20, 21, 40, 101))
def test_geweke_windows_are_the_short_series_they_name(N):
    """geweke()'s first window is a tenth of the chain (3 rows of 20): z is, bit for bit, the formula on the statistics of the
    two windows uploaded alone -- and those short series are held to the reference by the tests above."""
    from fmcmc_amd.convergence import _window_rows
    from fmcmc_amd.summary import window_stats
    arr, _ = length_case(N, nchains=3)
    dc = upload(arr)
    iters = np.arange(1, N + 1)
    wins = [_window_rows(iters, 1.0, np.ceil(1.0 + 0.1 * (N - 1.0))), _window_rows(iters, np.floor(N - 0.5 * (N - 1.0)), float(N))]
    assert wins[0][1] - wins[0][0] == {20: 3, 21: 3, 40: 5, 101: 11}[N]
    cs = [window_stats(upload(arr[:, lo:hi]), 0, hi - lo, None)[2] for lo, hi in wins]
    want = (cs[0][:, :, 0] - cs[1][:, :, 0]) / np.sqrt(cs[0][:, :, 2] / (wins[0][1] - wins[0][0]) + cs[1][:, :, 2] / (wins[1][1] - wins[1][0]))
    assert np.array_equal(_bits(dc.geweke()), _bits(want))


# ------------------------------------------------------------------------------------------------ selection
SEL_C, SEL_N = 3, 2049          # 6147 pooled values; a chain is one histogram tile and one row
LINSPACE16 = tuple(np.linspace(0.0, 1.0, 16))
PACKED16 = tuple(np.linspace(0.5 - 1e-4, 0.5 + 1e-4, 16))


def _pooled_to_chains(values, rng, other=None):
    """6147 values, shuffled -> [3][2049][1 or 2]; `other`: an ordinary second column next to them."""
    v = np.asarray(values, dtype=np.float64).copy()
    assert v.size == SEL_C * SEL_N
    rng.shuffle(v)
    cols = [v.reshape(SEL_C, SEL_N)] + ([] if other is None else [other])
    return np.stack(cols, axis=2)


def _ordinary(rng):
    return np.stack([ar1(0.5, SEL_N, rng, mu=1.0) for _ in range(SEL_C)])


def check_exact_keys(dc, probs):
    """check_exact with key_sort in the place of np.sort (one column)."""
    from fmcmc_amd.summary import window_stats
    host = dc.samples.cpu().numpy()
    C_, k, N = host.shape
    assert k == 1
    _, os_, _ = window_stats(dc, 0, N, None, probs)
    sm = dc.summary(quantiles=probs)
    n = C_ * N
    srt = key_sort(host[:, 0, :])
    for q, prob in enumerate(probs):
        index = 1.0 + np.float64(n - 1) * np.float64(prob)
        lo, hi = int(np.floor(index)), int(np.ceil(index))
        xlo, xhi = srt[lo - 1], srt[hi - 1]
        assert _bits(os_[0, q, 0]) == _bits(xlo), (prob, os_[0, q, 0], xlo)
        assert _bits(os_[0, q, 1]) == _bits(xhi), (prob, os_[0, q, 1], xhi)
        h = index - lo
        want = (1.0 - h) * xlo + h * xhi if (index > lo and xhi != xlo) else xlo
        assert _bits(sm.quantiles[0, q]) == _bits(want), prob
    return sm


@pytest.mark.parametrize("probs", [LINSPACE16, PACKED16, (0.5, 0.5, 0.25, 0.5, 0.25, 1.0, 1.0, 0.0), (0.0,), (1.0,)],
                         ids=["16-spread", "16-packed", "repeated", "min", "max"])
def test_sixteen_quantiles_and_their_corners(probs):
    """16 probs are 32 targets per column: the full width of the per-target arrays of select_scan_kernel and of the LDS
    histograms.  Packed around the median the targets share their prefix until the last passes."""
    rng = np.random.default_rng(16)
    arr = np.stack([np.stack([ar1(0.8, SEL_N, rng, mu=3.0), ar1(0.2, SEL_N, rng, mu=-2.0)], axis=1) for _ in range(SEL_C)])
    dc = upload(arr)
    sm, host = check_exact(dc, probs)
    check_moments(sm, host, [0, 1])
    check_exact(dc, probs, cols=[1])
    assert np.all(np.isfinite(sm.statistics)) and np.all(np.isfinite(sm.quantiles))


def test_seventeen_quantiles_are_refused():
    arr, _ = length_case(64)
    with pytest.raises(ValueError, match="at most 16"):
        upload(arr).summary(quantiles=np.linspace(0, 1, 17))


def _last_byte(rng):
    return 1.0 + rng.integers(0, 256, SEL_C * SEL_N) * 2.0 ** -52


def _top_bytes(rng):
    e = np.arange(-127, 128)                    # 2^(8 e): 2^-1016 .. 2^1016, one value per top-byte pair and sign
    v = np.concatenate([np.ldexp(1.0, 8 * e), -np.ldexp(1.0, 8 * e)])
    return v[rng.integers(0, v.size, SEL_C * SEL_N)]


def _extremes(rng):
    fi = np.finfo(np.float64)
    pool = np.array([fi.max, -fi.max, fi.tiny, -fi.tiny, 5e-324, -5e-324, 2.0 ** -1060, -2.0 ** -1060, fi.tiny / 2, -fi.tiny / 2,
                     np.nextafter(fi.tiny, 0.0), -np.nextafter(fi.tiny, 0.0), 1.0, -1.0])
    return pool[rng.integers(0, pool.size, SEL_C * SEL_N)]


def _all_negative(rng):
    return -np.exp(3.0 * rng.standard_normal(SEL_C * SEL_N))


V0 = np.array([0x3FF80000000000FF], dtype=np.uint64).view(np.float64)[0]      # the next double carries into the second byte:
V1 = np.nextafter(V0, 2.0)                                                    # the two runs of ties lie in different bins
N_BELOW, N_V0, N_V1 = 100, 2359, 2458                                         # of passes 6 and 7


def _ties(rng):
    """100 values below, 2359 x V0, 2458 x V1, 1230 above: with n = 6147, prob 0.4 has index 2459.4 -> x_(2459) is the last
    V0 and x_(2460) the first V1; prob 0.8 has index 4917.8 -> x_(4917) is the last V1 and x_(4918) the first value above."""
    n = SEL_C * SEL_N
    above = n - N_BELOW - N_V0 - N_V1
    return np.concatenate([V0 - 1e-3 - rng.random(N_BELOW), np.full(N_V0, V0), np.full(N_V1, V1), V1 + 1e-3 + rng.random(above)])


TIE_PROBS = (0.4, 0.8, 0.2, 0.6, 0.0, 1.0, (N_BELOW - 0.5) / 6146.0)


@pytest.mark.parametrize("make, probs, moments", [
    (_last_byte, LINSPACE16, "mean"), (_top_bytes, LINSPACE16, None), (_extremes, LINSPACE16, None),
    (_all_negative, LINSPACE16, "all"), (_ties, TIE_PROBS, "all")],
    ids=["last-byte", "top-bytes", "subnormal-to-DBL_MAX", "all-negative", "ties-across-a-bin-edge"])
def test_key_order_of_the_radix_select(make, probs, moments):
    """Pass 7 alone decides (values that differ in the last byte only); pass 0 alone decides (both sign halves of the top
    byte); subnormals and +-DBL_MAX (the second moments of these two overflow: not checked); negative keys run backwards; ranks that fall on
    the two ends of long runs of ties in neighbouring bins.  The ordinary column beside them is not disturbed."""
    rng = np.random.default_rng(5)
    other = _ordinary(rng)
    if make is _ties:
        n = SEL_C * SEL_N
        assert [int(np.floor(1.0 + (n - 1) * q)) for q in probs[:2]] == [N_BELOW + N_V0, N_BELOW + N_V0 + N_V1]
        assert (int(_bits(V0)[0]) & 0xFF, int(_bits(V1)[0]) & 0xFFFF) == (0xFF, 0x0100)
    dc = upload(_pooled_to_chains(make(rng), rng, other))
    sm, host = check_exact(dc, probs)
    alone = upload(other[:, :, None]).summary(quantiles=probs)
    assert np.array_equal(_bits(sm.statistics[1]), _bits(alone.statistics[0]))
    assert np.array_equal(_bits(sm.quantiles[1]), _bits(alone.quantiles[0]))
    assert np.all(np.isfinite(sm.statistics[1])) and np.all(np.isfinite(sm.quantiles))
    if moments == "all":
        check_moments(sm, host, [0, 1])
    if moments == "mean":
        # values 2^-52 apart around 1.0: a float64 mean lies on their grid, up to d = N u mean|x| >> sd from the true one, and
        # the variance of any algorithm that centres on it carries d^2 (the last term of check_acov's bound) >> var: only
        # the means can be held to the reference
        x = host[:, 0, :].astype(LD)
        assert np.all(np.abs(sm.per_chain.mean[:, 0] - x.mean(1)) <= SEL_N * U * np.abs(x).mean(1))
        assert abs(sm.statistics[0, 0] - x.mean()) <= x.size * U * np.abs(x).mean()
        assert (SEL_N * U * np.abs(x).mean()) ** 2 > x.var()
    if moments:
        assert np.all(np.isfinite(sm.statistics)) and np.all(np.isfinite(sm.ess))


def test_negative_zero_sorts_below_positive_zero():
    """np.sort leaves the order of -0.0 and +0.0 open (they compare equal), so the reference here is a sort of the
    order-preserving integer keys, which puts -0.0 below +0.0: the device's radix select works on the same keys.  R's sort()
    and quantile(type = 7) treat the two zeros as equal, so either sign is a correct order statistic there; the choice is
    documented in INTEGRATION.md section 2.2.  One prob puts x_(lo) on the last -0.0 and x_(hi) on the first +0.0."""
    rng = np.random.default_rng(0)
    n = SEL_C * SEL_N
    neg = np.concatenate([-rng.random(600), np.full(300, -5e-324), np.full(300, -1e-300)])
    pos = np.concatenate([rng.random(n - 1200 - 1800 - 1800 - 600), np.full(300, 5e-324), np.full(300, 1e-300)])
    values = np.concatenate([neg, np.full(1800, -0.0), np.full(1800, 0.0), pos])
    lo = neg.size + 1800                        # 1-based rank of the last -0.0
    probs = LINSPACE16[:15] + ((lo - 0.5) / (n - 1),)
    dc = upload(_pooled_to_chains(values, rng))
    srt = key_sort(dc.samples.cpu().numpy())
    assert np.array_equal(srt, np.sort(values)) and np.all(np.signbit(srt[:lo])) and not np.any(np.signbit(srt[lo:]))
    sm = check_exact_keys(dc, probs)
    assert _bits(sm.quantiles[0, 15]) == _bits(-0.0)
    host = dc.samples.cpu().numpy()
    check_moments(sm, host, [0])
    assert np.all(np.isfinite(sm.statistics)) and np.all(np.isfinite(sm.ess))


# ------------------------------------------------------------------------------------------------ width
def test_256_columns():
    """k = 256 is the engine's ceiling: 2048 / p histogram blocks per column shrink to 8, and the pooling and selection grids
    are 256 wide."""
    arr = width_case(256)
    dc = upload(arr)
    host = dc.samples.cpu().numpy()
    tol, refs = edge_tolerance([host[c, j] for c in range(2) for j in range(256)], "2 x 600 x 256", acov=False)
    check_reference(refs, None, "width")
    for probs in (DEFAULT, LINSPACE16):
        sm, _ = check_exact(dc, probs)
        check_moments(sm, host, range(256))
        check_series(sm.per_chain, host, list(range(256)), tol, refs)


def test_a_permuted_subset_of_65_columns():
    arr = width_case(65, seed=65)
    cols = [int(c) for c in np.random.default_rng(33).permutation(65)[:33]]
    dc = upload(arr)
    host = dc.samples.cpu().numpy()
    tol, refs = edge_tolerance([host[c, j] for c in range(2) for j in cols], "2 x 600 x 33 of 65", acov=True)
    check_reference(refs, None, "width, subset")
    check_acov(series_slots(dc, cols), host, cols, refs)
    sm, _ = check_exact(dc, LINSPACE16, cols=cols)
    check_moments(sm, host, cols)
    check_series(sm.per_chain, host, cols, tol, refs)
    full = dc.summary(quantiles=LINSPACE16)
    assert np.array_equal(_bits(sm.statistics), _bits(full.statistics[cols])) and np.array_equal(_bits(sm.quantiles), _bits(full.quantiles[cols]))
