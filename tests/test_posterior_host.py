"""Host tests of hpd_interval(), autocorr_diag() and crosscorr() (fmcmc_amd/summary.py: hpd_gap, host_hpd_interval, HpdInterval,
autocorr_lags, host_autocov, host_autocorr, AutocorrDiag, crosscorr_finish).  No GPU.

 * HPD is comparisons and one subtraction per width: host_hpd_interval is held bit for bit to a scalar loop of coda's
   HPDinterval written here (sorted(), Python's round, which is half-to-even as R's, and the first strict minimum).
 * Autocovariances against a longdouble loop within the a-priori bound of check_acov (tests/test_gpu_summary_edges.py), which
   holds for any float64 evaluation that centres on a float64 mean and sums the products in some order; the autocorrelation
   within what that bound leaves of a ratio (`acf_bound`).
 * crosscorr_finish on a partial formed in longdouble against the longdouble correlation of the pooled rows, within 16 x the
   distance of float64 np.corrcoef from that longdouble value on the same data (the rule of test_gpu_summary_edges.py:181:
   measured from the reference's own float64 evaluation, printed).
The helpers below are shared with tests/test_gpu_posterior.py."""
import numpy as np
import pytest

from fmcmc_amd.summary import (AutocorrDiag, HpdInterval, autocorr_lags, crosscorr_finish, host_autocorr, host_autocov,
                               host_hpd_interval, hpd_gap)

LD = np.longdouble
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ar1(phi, n, rng, mu=0.0):
    e = rng.standard_normal(n)
    x = np.empty(n)
    x[0] = e[0] / np.sqrt(1 - phi * phi)
    for i in range(1, n):
        x[i] = phi * x[i - 1] + e[i]
    return x + mu


# ------------------------------------------------------------------------------------------------ references
def scalar_hpd(x, prob=None, gap=None):
    """coda::HPDinterval of one series as a scalar loop: (lower, upper, index, gap)."""
    vals = sorted(float(v) for v in x)
    n = len(vals)
    if gap is None:
        gap = max(1, min(n - 1, round(n * prob)))
    best, at = None, 0
    for i in range(n - gap):
        w = np.float64(vals[i + gap]) - np.float64(vals[i])
        if best is None or w < best:
            best, at = w, i
    return vals[at], vals[at + gap], at, gap


def ld_autocov(x, lags):
    """One series in longdouble: the mean, the centred series, c_0, c_h per lag and sum |xc_i xc_{i+h}| per lag (and for 0)."""
    x = np.asarray(x).astype(LD)
    n = x.size
    mean = x.sum() / LD(n)
    xc = x - mean
    lags = [int(h) for h in lags]
    c = np.array([(xc[:n - h] * xc[h:]).sum() / LD(n) for h in lags], dtype=LD)
    absr = np.array([np.abs(xc[:n - h] * xc[h:]).sum() for h in lags], dtype=LD)
    return dict(mean=mean, xc=xc, c0=(xc * xc).sum() / LD(n), abs0=(xc * xc).sum(), c=c, absr=absr, lags=lags, x=x)


def acov_bounds(ref):
    """The bound of check_acov for c_0 and for every lag of `ref`, and d = N u mean|x|, the worst error of a float64 mean:
        (N + 2) u sum|xc_i xc_{i+h}| / N  +  d (|sum_{i<N-h} xc_i| + |sum_{i>=h} xc_i|) / N  +  d^2."""
    n = ref["x"].size
    d = n * U * np.abs(ref["x"]).mean()
    cs = np.concatenate([[LD(0)], np.cumsum(ref["xc"])])
    one = lambda h, a: (n + 2) * U * a / n + d * (abs(cs[n - h]) + abs(cs[n] - cs[h])) / n + d * d
    return one(0, ref["abs0"]), np.array([one(h, a) for h, a in zip(ref["lags"], ref["absr"])], dtype=LD), d


def acf_bound(ref):
    """What acov_bounds leaves of c_h / c_0: with |c_h - r_h| <= e_h and |c_0 - r_0| <= e_0 < r_0,
    |c_h / c_0 - r_h / r_0| <= (e_h + |r_h / r_0| e_0) / (r_0 - e_0), plus one rounding of the division."""
    e0, eh, _ = acov_bounds(ref)
    rho = np.abs(ref["c"] / ref["c0"])
    return (eh + rho * e0) / (ref["c0"] - e0) + U * (rho + (eh + rho * e0) / (ref["c0"] - e0))


def ld_partial(chains, center=None):
    """chains [m][N][p] -> the head of the partial of fmcmc_gelman_partial_dev (m, sum xbar, sum xbar xbar^T, sum S_c; the
    remaining 4 p slots are left 0), every sum formed in longdouble and rounded once."""
    x = np.asarray(chains).astype(LD)
    m, n, p = x.shape
    if center is not None:
        x = x - np.asarray(center).astype(LD)[None, None, :]
    xbar = x.sum(1) / LD(n)                                               # [m][p]
    dev = x - xbar[:, None, :]
    S = np.einsum("cni,cnj->cij", dev, dev) / LD(n - 1)
    P = np.zeros(1 + 5 * p + 2 * p * p)
    P[0] = m
    P[1:1 + p] = xbar.sum(0)
    P[1 + p:1 + p + p * p] = np.einsum("ci,cj->ij", xbar, xbar).ravel()
    P[1 + p + p * p:1 + p + 2 * p * p] = S.sum(0).ravel()
    return P


def ld_corr(chains):
    """The correlation matrix of the m N pooled rows in longdouble."""
    x = np.asarray(chains).astype(LD)
    x = x.reshape(-1, x.shape[-1])
    dev = x - x.sum(0) / LD(x.shape[0])
    cov = dev.T @ dev
    sd = np.sqrt(cov.diagonal())
    return cov / np.outer(sd, sd)


def corr_tolerance(chains, label):
    """16 x the distance of float64 np.corrcoef from the longdouble correlation of the same pooled rows, and that reference."""
    ref = ld_corr(chains)
    x = np.asarray(chains, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    own = np.atleast_2d(np.corrcoef(x, rowvar=False))
    dist = float(np.abs(own.astype(LD) - ref).max())
    print("[%s] float64 np.corrcoef vs longdouble: %.3g -> tolerance %.3g" % (label, dist, 16 * dist))
    return 16 * dist, ref


def correlated(m, n, p, seed):
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((p, p)) + 2.0 * np.eye(p)
    return rng.standard_normal((m, n, p)) @ mix + rng.standard_normal(p) + 0.3 * rng.standard_normal((m, 1, p))


# ------------------------------------------------------------------------------------------------ HPD
def check_hpd(series, prob):
    lo, hi, idx = host_hpd_interval(series, prob)
    flat = np.asarray(series, dtype=np.float64).reshape(-1, np.shape(series)[-1])
    for s, a, b, i in zip(flat, np.ravel(lo), np.ravel(hi), np.ravel(idx)):
        wl, wu, wi, gap = scalar_hpd(s, prob)
        assert gap == hpd_gap(s.size, prob)
        assert (a, b, i) == (wl, wu, wi), (prob, a, b, i, wl, wu, wi)
        assert _bits(a) == _bits(wl) or a == 0.0
        assert _bits(b) == _bits(wu) or b == 0.0


def test_gap_rounds_half_to_even_and_is_clamped():
    assert hpd_gap(10, 0.25) == 2 and hpd_gap(6, 0.25) == 2              # 2.5 -> 2, 1.5 -> 2 (R's round)
    assert hpd_gap(10, 0.35) == 4 and hpd_gap(14, 0.25) == 4              # 3.5 -> 4
    assert hpd_gap(10, 0.01) == 1 and hpd_gap(10, 0.04) == 1              # round gives 0: clamped to 1
    assert hpd_gap(10, 0.99) == 9 and hpd_gap(10, 0.96) == 9              # round gives 10: clamped to N - 1
    assert hpd_gap(3, 0.5) == 2 and hpd_gap(10000, 0.95) == 9500
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            hpd_gap(10, bad)


@pytest.mark.parametrize("n,prob", [(10, 0.25), (6, 0.25), (10, 0.01), (10, 0.99), (3, 0.5), (257, 0.95), (1000, 0.5), (1000, 0.05)])
def test_host_hpd_against_a_scalar_loop(n, prob):
    rng = np.random.default_rng(1000 * n + int(100 * prob))
    check_hpd(np.stack([rng.standard_normal((3, n)), np.exp(rng.standard_normal((3, n)))]), prob)


def test_host_hpd_ties_take_the_first_minimum():
    rng = np.random.default_rng(7)
    lattice = rng.integers(0, 8, (4, 400)).astype(np.float64)
    for prob in (0.1, 0.5, 0.9):
        check_hpd(lattice, prob)
    lo, hi, idx = host_hpd_interval(np.arange(20.0), 0.5)                # every width is 10: the first interval
    assert (lo, hi, idx) == (0.0, 10.0, 0)
    lo, hi, idx = host_hpd_interval(np.array([0.0, 5.0, 6.0, 7.0, 12.0, 13.0, 14.0, 30.0]), 0.25)   # gap 2: widths 6 2 6 6 2 16
    assert (lo, hi, idx) == (5.0, 7.0, 1)


def test_host_hpd_of_a_constant_series():
    lo, hi, idx = host_hpd_interval(np.full((2, 50), 3.25), 0.95)
    assert np.all(lo == 3.25) and np.all(hi == 3.25) and not idx.any()
    check_hpd(np.full((2, 50), 3.25), 0.95)


def test_hpd_object_and_its_printed_layout():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 2, 200))
    lo, hi, idx = host_hpd_interval(x, 0.9)
    h = HpdInterval(lo, hi, idx, hpd_gap(200, 0.9), 200, ["alpha", "beta"])
    assert h.table.shape == (2, 2, 2) and h.probability == 0.9 and h.gap == 180
    assert np.array_equal(h.table[1][:, 0], lo[1]) and np.array_equal(h.table[1][:, 1], hi[1])
    lines = str(h).split("\n")
    assert lines[0] == "[[1]]" and lines[1].split() == ["lower", "upper"] and lines[2].split()[0] == "alpha"
    assert lines[4] == 'attr(,"Probability")' and lines[5] == "[1] 0.9" and lines[7] == "[[2]]"
    assert float(lines[3].split()[1]) == pytest.approx(lo[0, 1], abs=1e-3)


# ------------------------------------------------------------------------------------------------ autocorrelation
@pytest.mark.parametrize("n", (3, 5, 64, 1000, 4097))
@pytest.mark.parametrize("family", ("ar1", "offset"))
def test_host_autocorr_against_longdouble(n, family):
    rng = np.random.default_rng(n)
    x = ar1(0.9, n, rng) if family == "ar1" else 1e8 + ar1(0.5, n, rng)
    lags = sorted({0, 1, 2, 50, n - 2, n - 1} & set(range(n)))
    ref = ld_autocov(x, lags)
    mean, c0, c = host_autocov(x, lags)
    e0, eh, d = acov_bounds(ref)
    assert abs(LD(mean) - ref["mean"]) <= d and abs(LD(c0) - ref["c0"]) <= e0
    assert np.all(np.abs(c.astype(LD) - ref["c"]) <= eh)
    acf = host_autocorr(x, lags)
    err, bound = np.abs(acf.astype(LD) - ref["c"] / ref["c0"]), acf_bound(ref)
    print("n = %d, %s: worst |acf - longdouble| / bound = %.3g" % (n, family, float((err / bound).max())))
    assert np.all(err <= bound) and acf[0] == 1.0


def test_host_autocorr_shapes_and_the_constant_series():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((2, 3, 100))
    acf = host_autocorr(x, [0, 1, 7])
    assert acf.shape == (2, 3, 3) and np.all(acf[..., 0] == 1.0)
    assert np.array_equal(_bits(acf[1, 2]), _bits(host_autocorr(x[1, 2], [0, 1, 7])))
    assert np.all(np.isnan(host_autocorr(np.full(10, 2.0), [0, 1])))


def test_lags_follow_coda():
    labels, rows = autocorr_lags((0, 1, 5, 10, 50), 40, 1)
    assert labels.tolist() == [0, 1, 5, 10] and rows.tolist() == [0, 1, 5, 10]       # lag 50 is not below 40 rows
    labels, rows = autocorr_lags((0, 1, 5, 10, 50), 40, 3)
    assert labels.tolist() == [0, 3, 15, 30] and rows.tolist() == [0, 1, 5, 10]      # 150 is not below 120 iterations
    labels, rows = autocorr_lags((0, 3, 117), 40, 3, relative=False)
    assert labels.tolist() == [0, 3, 117] and rows.tolist() == [0, 1, 39]
    assert autocorr_lags((0, 3, 120), 40, 3, relative=False)[0].tolist() == [0, 3]
    with pytest.raises(ValueError, match="^Lags do not conform to thinning interval$"):
        autocorr_lags((0, 1, 5), 40, 3, relative=False)
    with pytest.raises(ValueError, match="no lag below"):
        autocorr_lags((50, 60), 40, 1)


def test_autocorr_object_divides_and_averages_in_chain_order():
    rng = np.random.default_rng(5)
    acov, c0 = rng.standard_normal((3, 4, 2)), 1.0 + rng.random((3, 2))
    a = AutocorrDiag(acov, c0, [0, 2, 10, 20], [0, 1, 5, 10], ["u", "v"])
    assert np.array_equal(_bits(a.acf), _bits(acov / c0[:, None, :]))
    assert np.array_equal(_bits(a.mean), _bits(((a.acf[0] + a.acf[1]) + a.acf[2]) / 3))
    assert a.rownames == ["Lag 0", "Lag 2", "Lag 10", "Lag 20"]
    lines = str(a).split("\n")
    assert lines[0].split() == ["u", "v"] and lines[3].split()[:2] == ["Lag", "10"] and len(lines) == 5
    assert float(lines[2].split()[2]) == pytest.approx(a.mean[1, 0], abs=1e-3)


# ------------------------------------------------------------------------------------------------ cross-correlation
@pytest.mark.parametrize("m", (1, 2, 5))
@pytest.mark.parametrize("p", (1, 3))
def test_crosscorr_finish_against_longdouble(m, p):
    chains = correlated(m, 500, p, 100 * m + p)
    tol, ref = corr_tolerance(chains, "m = %d, p = %d" % (m, p))
    for center in (None, chains[0, 0]):
        got = crosscorr_finish(ld_partial(chains, center), p, 500)
        err = float(np.abs(got.astype(LD) - ref).max())
        print("m = %d, p = %d, centred %s: |crosscorr_finish - longdouble| = %.3g" % (m, p, center is not None, err))
        assert got.shape == (p, p) and np.array_equal(_bits(got.diagonal()), _bits(np.ones(p)))
        assert np.array_equal(got, got.T)
        assert err <= tol


def test_crosscorr_finish_zero_variance_and_arguments():
    chains = correlated(2, 300, 3, 9)
    chains[:, :, 1] = 4.5
    got = crosscorr_finish(ld_partial(chains), 3, 300)
    assert np.all(np.isnan(got[1, :])) and np.all(np.isnan(got[:, 1]))
    assert got[0, 0] == 1.0 and got[2, 2] == 1.0 and np.isfinite(got[0, 2]) and got[0, 2] == got[2, 0]
    with pytest.raises(ValueError, match="partial"):
        crosscorr_finish(np.zeros(5), 3, 300)


# ------------------------------------------------------------------------------------------------ ABI, exports
def test_exports():
    import fmcmc_amd
    from fmcmc_amd import _abi as abi
    from test_abi import declared_functions
    L = abi.lib()
    for name in ("fmcmc_hpd_work_len", "fmcmc_hpd_dev", "fmcmc_autocov_out_len", "fmcmc_autocov_dev"):
        assert name in abi.EXPORTS and name in declared_functions() and hasattr(L, name), name
    for name in ("hpd_interval", "HpdInterval", "autocorr_diag", "AutocorrDiag", "crosscorr"):
        assert name in fmcmc_amd.__all__ and hasattr(fmcmc_amd, name), name
    for name in ("hpd_interval", "autocorr_diag", "crosscorr"):
        assert hasattr(fmcmc_amd.DeviceChains, name)
    assert abi.ABI_VERSION == 6 and L.fmcmc_abi_version() == 6
    assert L.fmcmc_hpd_work_len(4, 3) == 24 and L.fmcmc_hpd_work_len(0, 3) == 0
    assert L.fmcmc_autocov_out_len(4, 3, 5) == 4 * 3 * 8 and L.fmcmc_autocov_out_len(4, 3, 33) == 0


def test_argument_errors_come_before_any_device_call():
    import ctypes as C
    from fmcmc_amd import _abi as abi
    L = abi.lib()

    def hpd(N, gap, S=200000):
        return L.fmcmc_hpd_dev(1, 2, 3, S, 0, N, 1, 3, gap, 1, 1, None), abi.last_error()

    def acov(N, lags, S=1000):
        lags = np.asarray(lags, dtype=np.int64)
        return L.fmcmc_autocov_dev(1, 2, 3, S, 0, N, 1, 3, lags.ctypes.data_as(C.POINTER(C.c_int64)), lags.size, 1, 1, None), \
            abi.last_error()

    for gap in (0, 100, -1):
        rc, text = hpd(100, gap)
        assert rc == abi.ERR_ARG and "gap = %d" % gap in text, text
    rc, text = hpd(2, 1)
    assert rc == abi.ERR_ARG and "too short" in text
    rc, text = hpd(8200, 7)
    assert rc == abi.ERR_UNSUPPORTED and "8193" in text and "8192" in text, text
    rc, text = hpd(163841, 155648)
    assert rc == abi.ERR_UNSUPPORTED and "8192" in text
    for lags, piece in (([0, 100], "lags[1] = 100"), ([-1], "lags[0] = -1"), ([0, 5, 5], "repeats"), (list(range(33)), "nlags = 33"),
                        ([], "nlags = 0")):
        rc, text = acov(100, lags)
        assert rc == abi.ERR_ARG and piece in text, text
    assert L.fmcmc_autocov_dev(1, 2, 3, 1000, 0, 100, 1, 3, None, 1, 1, 1, None) == abi.ERR_ARG
