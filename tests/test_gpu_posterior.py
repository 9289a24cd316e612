"""GPU tests of hpd_interval(), autocorr_diag() and crosscorr() (fmcmc_amd/summary.py -> csrc/raftery.hip: chain_hpd_kernel,
csrc/summary.hip: summary_lag_kernel, csrc/gelman.hip through enqueue_gelman).

 * HPD is a selection, a sort and one float64 subtraction per width: lower, upper and the index are compared bit for bit with
   host_hpd_interval (np.sort) on the host copy of the rows; a zero may carry either sign (`same_u` of test_gpu_raftery.py:
   np.sort leaves the order of -0.0 and +0.0 open).  A tail holds 8192 rows: where a listed (N, prob) asks for more -- N = 10000
   at prob 0.05 has 9500 -- the documented NotImplementedError is what is asserted.
 * Every autocovariance against longdouble within the a-priori bound of check_acov (tests/test_gpu_summary_edges.py; restated
   as acov_bounds in tests/test_posterior_host.py): nothing of the device enters it.  The worst err / bound is printed.
 * acf and its mean over the chains are, bit for bit, the float64 division and the chain-order sum of the returned c_h.
 * crosscorr() is, bit for bit, crosscorr_finish of the partial of enqueue_gelman, and agrees with longdouble within 16 x the
   distance of float64 np.corrcoef from longdouble on the same rows (printed).
 * Against the float64 host functions on to_host(): HPD bit for bit; the autocorrelation within twice acf_bound (each side is
   within acf_bound of longdouble)."""
import numpy as np
import pytest

from test_gpu_raftery import mixed, same_u
from test_gpu_summary import _bits, ar1, upload
from test_gpu_summary_edges import device_chains, order_max, series_slots
from test_posterior_host import LD, acf_bound, acov_bounds, corr_tolerance, ld_autocov

pytestmark = pytest.mark.gpu
HPD_MAX_TAIL = 8192
DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------ HPD
def check_hpd(dc, prob, cols=None):
    """hpd_interval(prob) of `dc` against np.sort on the host copy, or the documented refusal where a tail is too long."""
    from fmcmc_amd.summary import host_hpd_interval, hpd_gap
    host = dc.samples.cpu().numpy()                                    # [C][k][N]
    C_, k, N = host.shape
    cols_ = list(range(k)) if cols is None else list(cols)
    gap = hpd_gap(N, prob)
    if N - gap > HPD_MAX_TAIL:
        with pytest.raises(NotImplementedError, match="8192"):
            dc.hpd_interval(prob, cols=cols)
        return None
    h = dc.hpd_interval(prob, cols=cols)
    lo, hi, idx = host_hpd_interval(host[:, cols_], prob)
    assert h.lower.shape == (C_, len(cols_)) and h.table.shape == (C_, len(cols_), 2)
    assert h.gap == gap and h.nrows == N and h.probability == gap / N
    assert same_u(h.lower, lo) and same_u(h.upper, hi), (N, prob)
    assert np.array_equal(h.index, idx), (N, prob, h.index, idx)
    return h


def check_hpd_gap(dc, gap):
    """fmcmc_hpd_dev with an explicit gap against np.sort."""
    from fmcmc_amd.summary import enqueue_hpd, host_hpd_interval
    host = dc.samples.cpu().numpy()
    out, work, _ = enqueue_hpd(dc, gap, None)
    oh, wh = out.cpu().numpy(), work.cpu().numpy()
    lo, hi, idx = host_hpd_interval(host, gap=gap)
    assert same_u(oh[:, :, 0], lo) and same_u(oh[:, :, 1], hi) and np.array_equal(oh[:, :, 2], idx) and not oh[:, :, 3].any()
    srt = np.sort(host, axis=-1)
    N = host.shape[-1]
    assert same_u(wh[:, :, 0], srt[:, :, N - gap - 1]) and same_u(wh[:, :, 1], srt[:, :, gap])


@pytest.mark.parametrize("N", (3, 4, 5, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 10000))
def test_hpd_lengths_and_probabilities(N):
    """T = N - gap runs from 1 (prob 0.999999: round(N prob) = N, clamped to N - 1) to 0.95 N; below prob 0.5 the two tails
    overlap.  Around the 64 lanes, the 512 threads, the 4096 rows of a walk batch and the powers of two of the sort."""
    from fmcmc_amd.summary import hpd_gap
    dc = upload(mixed(N, 31 * N, chains=3))
    assert hpd_gap(N, 0.999999) == N - 1
    for prob in (0.05, 0.5, 0.95, 0.999999):
        check_hpd(dc, prob)
    if N == 10000:
        assert hpd_gap(N, 0.05) == 500 and hpd_gap(N, 0.5) == 5000


def test_hpd_at_the_tail_limit():
    """N = 8200 with gap 9, 8 and 7: T = 8191, 8192 (the whole of the LDS tails) and 8193, which is refused."""
    from fmcmc_amd.summary import enqueue_hpd
    dc = upload(mixed(8200, 8200, chains=2))
    check_hpd_gap(dc, 9)
    check_hpd_gap(dc, 8)
    with pytest.raises(NotImplementedError, match="8193.*8192"):
        enqueue_hpd(dc, 7, None)
    with pytest.raises(ValueError, match="gap = 0"):
        enqueue_hpd(dc, 0, None)
    with pytest.raises(ValueError, match="gap = 8200"):
        enqueue_hpd(dc, 8200, None)


def test_hpd_of_the_longest_series_at_95_percent():
    rng = np.random.default_rng(163840)
    dc = device_chains(np.exp(rng.standard_normal((1, 1, 163840))))
    h = check_hpd(dc, 0.95)
    assert h.gap == 155648 and h.nrows - h.gap == HPD_MAX_TAIL
    with pytest.raises(NotImplementedError, match="8192"):
        device_chains(rng.standard_normal((1, 1, 163860))).hpd_interval(0.95)       # gap 155667: T = 8193


def test_hpd_lattice_and_constant_series():
    """Integers 0 .. 7: hundreds of copies of each threshold value fill the tails, and many widths tie; a constant series."""
    rng = np.random.default_rng(8)
    arr = rng.integers(0, 8, (3, 3000, 3)).astype(np.float64)
    arr[:, :, 2] = 2.5
    dc = upload(arr)
    for prob in (0.05, 0.3, 0.5, 0.8, 0.95):
        h = check_hpd(dc, prob)
        assert np.all(h.lower[:, 2] == 2.5) and np.all(h.upper[:, 2] == 2.5) and not h.index[:, 2].any()
    few = upload(rng.integers(0, 2, (2, 65, 2)).astype(np.float64))
    for prob in (0.1, 0.5, 0.9):
        check_hpd(few, prob)


def test_hpd_extreme_values():
    """+-DBL_MAX: where every width overflows to inf, the first interval is the answer; beside ordinary values the infinite
    widths lose.  Subnormals: the widths are exact multiples of 2^-1074.  -0.0 beside +0.0."""
    rng = np.random.default_rng(100)
    n = 100
    arr = np.empty((2, n, 3))
    for c in range(2):
        arr[c, :, 0] = rng.permutation(np.repeat([-DBL_MAX, DBL_MAX], n // 2))
        z = rng.standard_normal(n)
        z[:3], z[3:6] = DBL_MAX, -DBL_MAX
        arr[c, :, 1] = rng.permutation(z)
        z = np.round(rng.standard_normal(n))
        z[z == 0] = np.where(rng.random((z == 0).sum()) < 0.5, -0.0, 0.0)
        arr[c, :, 2] = z
    dc = upload(arr)
    h = check_hpd(dc, 0.5)
    assert not h.index[:, 0].any() and np.all(h.lower[:, 0] == -DBL_MAX) and np.all(h.upper[:, 0] == DBL_MAX)
    assert np.all(np.isfinite(h.upper[:, 1] - h.lower[:, 1]))
    for prob in (0.05, 0.95):
        check_hpd(dc, prob)
    sub = upload(rng.integers(-1000, 1001, (2, 513, 2)) * 5e-324)
    for prob in (0.05, 0.5, 0.95):
        h = check_hpd(sub, prob)
        assert np.all(np.abs(h.table) < 2e-320)


def test_hpd_history_with_an_odd_row_stride():
    """More rows allocated than kept, an odd row stride: the series of odd (chain, column) start at an odd multiple of 8 bytes."""
    rng = np.random.default_rng(7101)
    nrows, cap = 5005, 7101
    cks = np.full((3, 2, cap), np.nan)
    for c in range(3):
        cks[c, 0, :nrows] = ar1(0.6, nrows, rng, mu=3.0)
        cks[c, 1, :nrows] = np.round(ar1(0.3, nrows, rng, mu=-2.0), 1) + 0.0
    hist = device_chains(cks, nrows=nrows)
    assert hist.capacity % 2 == 1
    alone = device_chains(cks[:, :, :nrows])
    for prob in (0.3, 0.95):
        a, b = check_hpd(hist, prob), check_hpd(alone, prob)
        assert np.array_equal(_bits(a.table), _bits(b.table)) and np.array_equal(a.index, b.index)
    ad, bd = hist.autocorr_diag((0, 1, 7, 5004)), alone.autocorr_diag((0, 1, 7, 5004))
    assert np.array_equal(_bits(ad.acov), _bits(bd.acov)) and np.array_equal(_bits(ad.c0), _bits(bd.c0))
    assert np.array_equal(_bits(hist.crosscorr()), _bits(alone.crosscorr()))


def test_hpd_of_a_series_does_not_depend_on_where_it_sits():
    rng = np.random.default_rng(1025)
    N = 1025
    s = np.round(ar1(0.8, N, rng, mu=3.0), 2) + 0.0

    def fields(dc, c, a, cols=None):
        return [[_bits(h.lower[c, a]).tolist(), _bits(h.upper[c, a]).tolist(), int(h.index[c, a])]
                for h in (dc.hpd_interval(prob, cols=cols) for prob in (0.2, 0.95))]

    want = fields(device_chains(s[None, None, :]), 0, 0)
    for nchains, at in ((5, 2), (40, 39)):
        cks = rng.standard_normal((nchains, 1, N)) * 10.0
        cks[at, 0] = s
        assert fields(device_chains(cks), at, 0) == want, (nchains, at)
    cks = rng.standard_normal((1, 7, N)) * np.arange(1, 8)[None, :, None]
    cks[0, 3] = s
    dc = device_chains(cks)
    for cols, where in (([3], [0]), ([5, 3, 0], [1]), ([3, 3], [0, 1]), (None, [3])):
        for a in where:
            assert fields(dc, 0, a, cols) == want, (cols, a)
    check_hpd(dc, 0.95, cols=[5, 3, 0])


def test_non_finite_rows_are_refused_and_the_column_is_named():
    arr = mixed(500, 5, chains=3)
    for row, bad in ((3, np.nan), (499, np.inf), (250, -np.inf)):
        a = arr.copy()
        a[2, row, 1] = bad
        dc = upload(a)
        with pytest.raises(ValueError, match=r"non-finite.*\[1\]"):
            dc.hpd_interval()
        with pytest.raises(ValueError, match=r"non-finite.*\[1\]"):
            dc.autocorr_diag()
        assert dc.hpd_interval(cols=[0, 2]).table.shape == (3, 2, 2)
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        upload(arr).hpd_interval(1.0)


# ------------------------------------------------------------------------------------------------ autocovariances
def check_autocov(dc, lags, cols=None):
    """mean, c_0 and every c_h of fmcmc_autocov_dev against longdouble within acov_bounds.  Returns out [C][p][3 + nlags]."""
    from fmcmc_amd.summary import enqueue_autocov
    host = dc.samples.cpu().numpy()
    C_, k, N = host.shape
    cols_ = list(range(k)) if cols is None else list(cols)
    out, work, _ = enqueue_autocov(dc, lags, cols)
    oh = out.cpu().numpy()
    assert oh.shape == (C_, len(cols_), 3 + len(lags)) and not oh[:, :, 2].any() and not work.cpu().numpy().any()
    worst = 0.0
    for c in range(C_):
        for a, col in enumerate(cols_):
            ref = ld_autocov(host[c, col], lags)
            e0, eh, d = acov_bounds(ref)
            assert abs(LD(oh[c, a, 0]) - ref["mean"]) <= d, (c, col)
            err0 = abs(LD(oh[c, a, 1]) - ref["c0"])
            err = np.abs(oh[c, a, 3:].astype(LD) - ref["c"])
            worst = max(worst, float(err0 / e0), float((err / eh).max()))
            assert err0 <= e0, (c, col, float(err0), float(e0))
            assert np.all(err <= eh), (c, col, lags, err / eh)
    print("N = %d, lags %s, %d series: worst |device - longdouble| / bound = %.3g" % (N, list(lags), C_ * len(cols_), worst))
    return oh


def lag_case(N, seed):
    """[2][N][2]: AR(1) with phi = 0.9, and a series around 1e8."""
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([ar1(0.9, N, rng), 1e8 + ar1(0.5, N, rng)], axis=1) for _ in range(2)])


@pytest.mark.parametrize("N", (3, 5, 64, 65, 4095, 4096, 4097, 19456, 19457, 40001))
def test_autocovariances_against_longdouble(N):
    lags = sorted({0, 1, 2, 4095, 4096, 4097, N - 2, N - 1} & set(range(N)))
    check_autocov(upload(lag_case(N, 5 * N)), lags)


def test_acf_and_its_mean_are_the_division_and_the_chain_order_sum():
    from fmcmc_amd.summary import enqueue_autocov
    rng = np.random.default_rng(300)
    arr = np.stack([np.stack([ar1(0.2 * j + 0.1 * c, 300, rng, mu=j) for j in range(3)], axis=1) for c in range(5)])
    dc = upload(arr, thin=3)
    ad = dc.autocorr_diag()
    assert ad.lags.tolist() == [0, 3, 15, 30, 150] and ad.rows.tolist() == [0, 1, 5, 10, 50]
    assert ad.rownames[2] == "Lag 15" and str(ad).split("\n")[3].split()[:2] == ["Lag", "15"]
    oh = enqueue_autocov(dc, ad.rows, None)[0].cpu().numpy()
    assert ad.acf.shape == (5, 5, 3) and ad.mean.shape == (5, 3)
    assert np.array_equal(_bits(ad.acov), _bits(oh[:, :, 3:].transpose(0, 2, 1))) and np.array_equal(_bits(ad.c0), _bits(oh[:, :, 1]))
    assert np.array_equal(_bits(ad.chain_mean), _bits(oh[:, :, 0]))
    assert np.array_equal(_bits(ad.acf), _bits(ad.acov / ad.c0[:, None, :])) and np.all(ad.acf[:, 0, :] == 1.0)
    total = ad.acf[0]
    for c in range(1, 5):
        total = total + ad.acf[c]
    assert np.array_equal(_bits(ad.mean), _bits(total / 5))
    assert np.all(np.abs(ad.mean[1] - (0.2 * np.arange(3) + 0.2)) < 0.2)          # (AR(1): acf_1 = phi, here 0.2 j + 0.1 c)
    labels = dc.autocorr_diag((0, 3, 30), relative=False)
    assert np.array_equal(_bits(labels.acov), _bits(ad.acov[:, [0, 1, 3]])) and labels.lags.tolist() == [0, 3, 30]
    with pytest.raises(ValueError, match="^Lags do not conform to thinning interval$"):
        dc.autocorr_diag((0, 1), relative=False)
    const = arr.copy()
    const[1, :, 2] = 7.0
    nan = upload(const).autocorr_diag((0, 1))
    assert np.all(np.isnan(nan.acf[1, :, 2])) and np.all(np.isnan(nan.mean[:, 2])) and np.all(np.isfinite(nan.mean[:, :2]))


def test_a_lag_has_the_same_bits_alone_among_32_and_elsewhere():
    """The sum of a lag depends on (N, h) alone: asked alone, as the last of 32 lags (the fourth walk), first of 9 (two walks),
    in another chain and column of a larger launch, and under a `cols` subset."""
    from fmcmc_amd.summary import enqueue_autocov
    rng = np.random.default_rng(4097)
    N = 4097
    s = ar1(0.9, N, rng, mu=2.0)
    one = device_chains(s[None, None, :])
    probe = (0, 1, 36, 1000, N - 1)
    alone = {h: enqueue_autocov(one, [h], None)[0].cpu().numpy()[0, 0] for h in probe}
    cks = rng.standard_normal((6, 4, N))
    cks[4, 2] = s
    big = device_chains(cks)
    for h in probe:
        others = [v for v in range(2, 2 + 40) if v not in probe]
        for lags in ([h] + others[:8], others[:31] + [h], others[:16] + [h] + others[16:20]):
            at = lags.index(h)
            for dc, c, a, cols in ((one, 0, 0, None), (big, 4, 2, None), (big, 4, 1, [3, 2])):
                got = enqueue_autocov(dc, lags, cols)[0].cpu().numpy()[c, a]
                assert np.array_equal(_bits(got[:3]), _bits(alone[h][:3])), (h, lags)
                assert _bits(got[3 + at]) == _bits(alone[h][3]), (h, lags, cols)
        if h == 0:
            assert _bits(alone[h][3]) == _bits(alone[h][1])                           # c_0 is the sum of lag 0


def test_lags_up_to_the_ar_order_agree_with_the_summary_kernel():
    """summary_series_kernel keeps r_0 .. r_M in its work buffer: both kernels are within the bound of longdouble, so within
    twice the bound of each other; the means are the same sum."""
    N = 4097
    M = order_max(N)
    assert M == 36
    dc = upload(lag_case(N, 36))
    lags = list(range(32))
    oh = check_autocov(dc, lags)
    slots = series_slots(dc).reshape(2, 2, 72)
    host = dc.samples.cpu().numpy()
    assert np.array_equal(_bits(oh[:, :, 0]), _bits(slots[:, :, 65]))
    for c in range(2):
        for j in range(2):
            _, eh, _ = acov_bounds(ld_autocov(host[c, j], lags))
            assert np.all(np.abs(oh[c, j, 3:].astype(LD) - slots[c, j, :32].astype(LD)) <= 2 * eh), (c, j)
    check_autocov(dc, [M, 5, 0, 33], cols=[1])


def test_lag_arguments():
    from fmcmc_amd.summary import enqueue_autocov
    dc = upload(lag_case(40, 40))
    for lags, piece in (([0, 40], r"lags\[1\] = 40"), ([3, 1, 3], "repeats"), (list(range(33)), "nlags = 33"), ([-1], r"lags\[0\] = -1")):
        with pytest.raises(ValueError, match=piece):
            enqueue_autocov(dc, lags, None)
    with pytest.raises(ValueError, match="repeats"):
        dc.autocorr_diag((1, 1))
    ad = dc.autocorr_diag()
    assert ad.lags.tolist() == [0, 1, 5, 10] and ad.acf.shape == (2, 4, 2)          # lag 50 is not below 40 rows
    assert dc.autocorr_diag(tuple(range(32))).acf.shape == (2, 32, 2)
    check_autocov(dc, list(range(8, 40)))


# ------------------------------------------------------------------------------------------------ cross-correlation
@pytest.mark.parametrize("C_,p,N", [(4, 3, 1000), (2, 65, 200), (1, 3, 500)])
def test_crosscorr_is_the_finish_of_the_gelman_partial_and_agrees_with_longdouble(C_, p, N):
    from fmcmc_amd.summary import crosscorr_finish, enqueue_gelman
    from test_posterior_host import correlated
    dc = upload(correlated(C_, N, p, 1000 * C_ + p))
    host = dc.samples.cpu().numpy().transpose(0, 2, 1)                               # [C][N][p]
    got = dc.crosscorr()
    assert got.shape == (p, p) and np.array_equal(_bits(got.diagonal()), _bits(np.ones(p))) and np.array_equal(got, got.T)
    partial = enqueue_gelman(dc, 0, N, None)[0].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(crosscorr_finish(partial, p, N)))
    tol, ref = corr_tolerance(host, "%d x %d x %d" % (C_, N, p))
    err = float(np.abs(got.astype(LD) - ref).max())
    print("|crosscorr() - longdouble| = %.3g" % err)
    assert err <= tol
    cols = [2, 0]
    sub = dc.crosscorr(cols=cols)
    assert np.array_equal(_bits(sub), _bits(crosscorr_finish(enqueue_gelman(dc, 0, N, cols)[0].cpu().numpy(), 2, N)))
    assert float(np.abs(sub.astype(LD) - ref[np.ix_(cols, cols)]).max()) <= tol


# ------------------------------------------------------------------------------------------------ public path
@pytest.fixture(scope="module")
def readme_run(readme_data):
    from fmcmc_amd import MCMC, gaussian_linreg, kernel_normal
    X, y = readme_data
    init = np.array([0.0, 0.0, np.std(y, ddof=1)])[None, :] + 0.1 * np.random.default_rng(4).standard_normal((4, 3))
    init[:, 2] = np.abs(init[:, 2])
    return MCMC(init, gaussian_linreg(X, y), 1000, nchains=4, burnin=100, thin=2, seed=11, kernel=kernel_normal(scale=0.15),
                _return_device=True)


def test_public_path_after_a_run(readme_run):
    import fmcmc_amd as F
    from fmcmc_amd.summary import host_autocorr, host_hpd_interval
    ans = readme_run
    ml = ans.to_host()
    series = np.ascontiguousarray(ml.as_array().transpose(0, 2, 1))                  # [C][k][N]
    C_, k, N = series.shape
    assert (C_, k, N) == (4, 3, 450)
    h = ans.hpd_interval()
    lo, hi, idx = host_hpd_interval(series, 0.95)
    assert h.table.shape == (4, 3, 2) and same_u(h.lower, lo) and same_u(h.upper, hi) and np.array_equal(h.index, idx)
    assert h.gap == 428 and h.probability == 428 / 450 and 'attr(,"Probability")' in str(h) and "[[4]]" in str(h)
    ad = ans.autocorr_diag()
    assert ad.acf.shape == (4, 5, 3) and ad.mean.shape == (5, 3) and ad.lags.tolist() == [0, 2, 10, 20, 100]
    want = host_autocorr(series, ad.rows)                                            # [C][k][nlags]
    for c in range(C_):
        for j in range(k):
            bound = acf_bound(ld_autocov(series[c, j], ad.rows))
            assert np.all(np.abs(ad.acf[c, :, j].astype(LD) - want[c, j].astype(LD)) <= 2 * bound), (c, j)
    cc = ans.crosscorr()
    tol, ref = corr_tolerance(series.transpose(0, 2, 1), "readme run")
    assert cc.shape == (3, 3) and float(np.abs(cc.astype(LD) - ref).max()) <= tol
    # an McmcList / Mcmc is uploaded first and gives the same bits
    assert np.array_equal(_bits(F.hpd_interval(ml).table), _bits(h.table))
    assert np.array_equal(_bits(F.autocorr_diag(ml).acf), _bits(ad.acf)) and np.array_equal(_bits(F.crosscorr(ml)), _bits(cc))
    one = F.hpd_interval(ml[1], 0.8, cols=[2])
    assert np.array_equal(_bits(one.table[0, 0]), _bits(ans.hpd_interval(0.8).table[1, 2])) and len(one.varnames) == 1
    assert F.crosscorr(ml[1]).shape == (3, 3)


def test_only_reads_and_refuses_sharded_chains(readme_run, monkeypatch):
    import torch
    import torch.distributed as dist
    kept = (readme_run._samples, readme_run._logpost, readme_run._draws)
    before = [t.clone() for t in kept]
    readme_run.hpd_interval()
    readme_run.autocorr_diag()
    readme_run.crosscorr()
    torch.cuda.synchronize()
    for b, a in zip(before, kept):
        assert torch.equal(b.view(torch.int64), a.view(torch.int64))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    for call in (readme_run.hpd_interval, readme_run.autocorr_diag, readme_run.crosscorr):
        with pytest.raises(NotImplementedError, match="sharded"):
            call()
