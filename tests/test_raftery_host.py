"""Host tests of the Raftery-Lewis diagnostic (fmcmc_amd/convergence.py: raftery_diag, raftery_counts, raftery_threshold;
fmcmc_amd/summary.py: raftery_bound, raftery_finish, host_chain_quantiles).  No GPU.

Everything here is exact: the counts are integers, and the finish is compared bit for bit with a scalar loop written in this
file from coda's raftery.diag (g2 accumulated cell by cell in coda's loop order, the burn-in and precision formulas term for
term)."""
import numpy as np
import pytest

from fmcmc_amd import raftery_diag
from fmcmc_amd.convergence import raftery_counts, raftery_threshold
from fmcmc_amd.summary import host_chain_quantiles, raftery_bound, raftery_finish, type7_quantiles, type7_ranks

LOOSE = ((0.25, 0.05, 0.9), (0.5, 0.1, 0.8))      # (q, r, s) with nmin = 203 and 42: small shapes


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    """NaN where the other is NaN, the same bits elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got[~np.isnan(got)]), _bits(want[~np.isnan(want)]))


def ar1(rho, n, rng, mu=0.0):
    e = rng.standard_normal(n)
    y = np.empty(n)
    y[0] = e[0] / np.sqrt(1 - rho * rho)
    for t in range(1, n):
        y[t] = rho * y[t - 1] + e[t]
    return y + mu


def scalar_finish(tri, last_pair, m, thin, q, r, s, eps, js):
    """coda::raftery.diag from the counts of one series, as a scalar loop: returns (M, N, I, kthin) or NaNs."""
    phi, nmin = raftery_bound(q, r, s)
    log = lambda v: np.log(np.array([v], dtype=np.float64))[0]
    nan4 = (np.nan, np.nan, np.nan, np.nan)
    with np.errstate(all="ignore"):
        for a, j in enumerate(js):
            if m[a] < 3:
                return nan4
            T = np.asarray(tri[a], dtype=np.float64).reshape(2, 2, 2)
            g2 = 0.0
            for i1 in range(2):
                for i2 in range(2):
                    for i3 in range(2):
                        if T[i1, i2, i3] != 0:
                            fitted = ((T[i1, i2, 0] + T[i1, i2, 1]) * (T[0, i2, i3] + T[1, i2, i3])) / (
                                (T[0, i2, 0] + T[0, i2, 1]) + (T[1, i2, 0] + T[1, i2, 1]))
                            g2 = g2 + T[i1, i2, i3] * log(T[i1, i2, i3] / fitted) * 2.0
            bic = g2 - log(np.float64(m[a] - 2)) * 2.0
            if bic < 0:
                break
        else:
            return None                                            # undecided
        F = T[:, :, 0] + T[:, :, 1]
        F[last_pair[a][0], last_pair[a][1]] += 1.0
        alpha = F[0, 1] / (F[0, 0] + F[0, 1])
        beta = F[1, 0] / (F[1, 0] + F[1, 1])
        kthin = np.float64(j * thin)
        largest = alpha if (alpha >= beta or np.isnan(alpha)) else beta          # R's max(): NA when either is
        tempburn = log((eps * (alpha + beta)) / largest) / log(abs(1.0 - alpha - beta))
        M = np.ceil(tempburn) * kthin
        ab = alpha + beta
        tempprec = ((2.0 - alpha - beta) * alpha * beta * (phi * phi)) / ((ab * ab * ab) * (r * r))
        N = M + np.ceil(tempprec) * kthin
        if not (np.isfinite(M) and np.isfinite(N)):
            return nan4[:3] + (kthin,)
        return M, N, N / nmin, kthin


def test_lower_bound():
    assert raftery_bound(0.025, 0.005, 0.95)[1] == 3746
    assert raftery_bound(0.25, 0.05, 0.9)[1] == 203
    assert raftery_bound(0.5, 0.1, 0.8)[1] == 42


@pytest.mark.parametrize("qrs", ((0.025, 0.005, 0.95),) + LOOSE)
def test_one_row_short_is_the_error_outcome(qrs):
    rng = np.random.default_rng(7)
    nmin = raftery_bound(*qrs)[1]
    x = rng.standard_normal((nmin, 2))
    short = raftery_diag(x[:nmin - 1], np.arange(1, nmin), *qrs)
    assert short.shape == (2, 4) and np.all(short[:, 2] == nmin) and np.all(np.isnan(short[:, [0, 1, 3]]))
    enough = raftery_diag(x, np.arange(1, nmin + 1), *qrs)
    assert np.all(np.isfinite(enough)) and np.all(enough[:, 2] == nmin)


def test_counts_derived_by_hand():
    """x_t = 0 when t % 40 == 0, else 1; n = 4000, q = 0.025.  Sorted: 100 zeros, then ones; index = 1 + 3999 * 0.025 = 100.975,
    so x_(100) = 0, x_(101) = 1, h = 0.975, u = 0.975 (to rounding) and Z marks the zeros at t = 0, 40, .., 3960.
    Triples (i = 0 .. 3997): (1,0,0) once per zero: 100; (0,0,1) for i + 2 = 40 .. 3960: 99; (0,1,0) for i + 1 = 40 .. 3960: 99;
    no two ones within a triple; (0,0,0) the remaining 3998 - 298 = 3700.  Last pair (Z_3998, Z_3999) = (0, 0).
    Pairs (i = 0 .. 3998): (1,0) 100, (0,1) 99, (1,1) 0, (0,0) 3999 - 199 = 3800."""
    n = 4000
    t = np.arange(n)
    x = np.where(t % 40 == 0, 0.0, 1.0)[:, None]
    u = raftery_threshold(x, 0.025)
    assert abs(u[0] - 0.975) < 1e-12          # (h = index - 100 carries the rounding of index = 100.975: an ulp is 1.4e-14)
    Z = x <= u
    assert Z.sum() == 100 and np.all(Z[::40, 0])
    tri, last = raftery_counts(Z, 1, 1)
    T = np.zeros((2, 2, 2), dtype=np.int64)
    T[1, 0, 0], T[0, 0, 1], T[0, 1, 0], T[0, 0, 0] = 100, 99, 99, 3700
    assert np.array_equal(tri[0, 0], T.ravel()) and list(last[0, 0]) == [0, 0]
    F = T.sum(axis=2)
    F[0, 0] += 1
    assert F.tolist() == [[3800, 99], [100, 0]]
    # from the hand-made tables: alpha = F01 / (F00 + F01), beta = F10 / (F10 + F11)
    fin = raftery_finish(T.reshape(1, 8), np.array([[0, 0]]), [n], 1)
    assert fin.j == 1 and fin.alpha == 99.0 / 3899.0 and fin.beta == 1.0
    # the whole diagnostic of this series is what a scalar loop makes of the counts of its thinnings
    got = raftery_diag(x, t + 1)
    js = list(range(1, 17))
    tri, last = raftery_counts(Z, 1, 16)
    want = scalar_finish(tri[0], last[0], [-(-n // j) for j in js], 1, 0.025, 0.005, 0.95, 0.001, js)
    assert want is not None
    assert same(got[0, [0, 1, 3]], want[:3]) and np.all(np.isfinite(want))
    assert got[0, 2] == 3746


def test_vectorised_finish_equals_a_scalar_loop_bit_for_bit():
    rng = np.random.default_rng(2024)
    nser, nj = 400, 6
    tri = rng.integers(0, 60, size=(nser, nj, 8))
    tri[rng.random((nser, nj, 8)) < 0.25] = 0                       # empty cells
    tri[:40, :, 4:] = 0                                             # a never 1: an empty row of F unless the last pair fills it
    tri[40:60, :, :] = 0
    tri[40:60, :, 0] = rng.integers(1, 500, size=(20, nj))          # one cell only: the constant indicator
    tri[60:90] *= 1000                                              # large counts
    last = rng.integers(0, 2, size=(nser, nj, 2))
    last[40:60] = 0
    js = [1, 2, 3, 4, 5, 6]
    ndecided = nnan = 0
    for m, thin in (([500, 250, 167, 125, 100, 84], 1), ([9, 5, 3, 3, 2, 2], 3)):
        for qrs in ((0.025, 0.005, 0.95),) + LOOSE:
            fin = raftery_finish(tri, last, m, thin, *qrs, converge_eps=0.001, j=js)
            for i in range(nser):
                want = scalar_finish(tri[i], last[i], m, thin, *qrs, 0.001, js)
                if want is None:
                    assert fin.undecided[i] and not fin.failed[i] and np.isnan(fin.M[i])
                    continue
                assert not fin.undecided[i]
                got = (fin.M[i], fin.N[i], fin.I[i], fin.kthin[i])
                assert same(got, want), (i, got, want)
                ndecided += np.isfinite(want[0])
                nnan += np.isnan(want[0])
    assert ndecided > 500 and nnan > 100


@pytest.mark.parametrize("seed", (1, 2, 3, 4))
def test_iid_normal_needs_about_nmin_rows(seed):
    """For an independent series alpha + beta -> 1, so kthin = 1, M is a row or two and N -> nmin: I within 0.9 .. 1.1."""
    x = np.random.default_rng(seed).standard_normal((10000, 1))
    from fmcmc_amd.summary import raftery_search
    Z = x <= raftery_threshold(x, 0.025)
    fin = raftery_search(lambda j0, nj: raftery_counts(Z, j0, nj), 10000, 1)
    assert fin.kthin[0] == 1 and 0.9 <= fin.I[0] <= 1.1
    row = raftery_diag(x, np.arange(1, 10001))[0]
    assert np.array_equal(_bits(row), _bits([fin.M[0], fin.N[0], 3746.0, fin.I[0]]))


def test_dependence_grows_with_autocorrelation():
    rng = np.random.default_rng(5)
    d = np.stack([ar1(0.0, 10000, rng), ar1(0.9, 10000, rng), ar1(0.99, 10000, rng)], axis=1)
    I = raftery_diag(d, np.arange(1, 10001))[:, 3]
    assert I[0] < 1.2 and 2.5 < I[1] < 8 and I[2] > 12


def test_constant_series_gives_nan_with_nmin_set():
    x = np.stack([np.full(5000, 3.25), np.zeros(5000), np.random.default_rng(1).standard_normal(5000)], axis=1)
    got = raftery_diag(x, np.arange(1, 5001))
    assert np.all(np.isnan(got[:2][:, [0, 1, 3]])) and np.all(got[:, 2] == 3746) and np.all(np.isfinite(got[2]))


def test_alternating_series_has_no_burn_in_to_report():
    """Z = 1, 0, 1, 0, ...: the second-order fit is exact at j = 1 (G2 = 0, BIC < 0) and alpha = beta = 1, so log|1 - alpha - beta|
    is 0 and coda's burn-in is -Inf: no number (NaN), Nmin set.  (A search that runs out of rows, m < 3, before any BIC < 0 is
    covered from the counts: the second set of lengths of the bit-for-bit test above.)"""
    x = np.tile([0.0, 1.0], 21)[:, None]
    got = raftery_diag(x, np.arange(1, 43), 0.5, 0.1, 0.8)
    assert got[0, 2] == 42 and np.all(np.isnan(got[0, [0, 1, 3]]))


def test_thin_3_scales_m_and_n_by_3():
    rng = np.random.default_rng(9)
    d = np.stack([ar1(0.0, 6000, rng), ar1(0.8, 6000, rng)], axis=1)
    one = raftery_diag(d, np.arange(1, 6001))
    three = raftery_diag(d, np.arange(5, 5 + 3 * 6000, 3))
    assert np.array_equal(three[:, :2], 3 * one[:, :2]) and np.array_equal(three[:, 2], one[:, 2])
    assert np.array_equal(_bits(three[:, 3]), _bits((3 * one[:, 1]) / 3746))


def test_non_finite_rows_are_refused():
    x = np.random.default_rng(3).standard_normal((4000, 3))
    x[17, 1] = np.nan
    with pytest.raises(ValueError, match=r"non-finite.*\[1\]"):
        raftery_diag(x, np.arange(1, 4001))


@pytest.mark.parametrize("n", (1, 2, 5, 100, 101))
def test_host_chain_quantiles_equal_a_sort(n):
    rng = np.random.default_rng(n)
    x = np.round(rng.standard_normal((3, 2, n)), 1)                 # many ties
    x[0, 0, : n // 2] = x[0, 0, 0]
    probs = [0.0, 0.025, 0.25, 1 / 3, 0.5, 0.75, 0.99, 1.0]
    got = host_chain_quantiles(x, probs)
    assert got.shape == (3, 2, len(probs))
    for c in range(3):
        for j in range(2):
            srt = np.sort(x[c, j])
            _, lo, hi = type7_ranks(n, probs)
            os_ = np.stack([srt[np.clip(lo - 1, 0, n - 1)], srt[np.clip(hi - 1, 0, n - 1)]], axis=-1)
            assert np.array_equal(_bits(got[c, j]), _bits(type7_quantiles(os_, n, probs)))
            assert got[c, j, 0] == srt[0] and got[c, j, -1] == srt[-1]
            if n > 1:
                assert np.allclose(got[c, j], np.quantile(x[c, j], probs), rtol=1e-12, atol=1e-12)


def test_print_follows_coda():
    from fmcmc_amd.summary import RafteryDiag, raftery_table, raftery_search
    x = np.random.default_rng(2).standard_normal((10000, 2))
    Z = x <= raftery_threshold(x, 0.025)
    fin = raftery_search(lambda j0, nj: raftery_counts(Z, j0, nj), 10000, 1)
    rd = RafteryDiag(raftery_table(fin, (2,))[None], fin.kthin[None], fin.nmin, 10000, 0.025, 0.005, 0.95, 0.001, ["a", "b"])
    text = str(rd)
    for piece in ("Quantile (q) = 0.025", "Accuracy (r) = +/- 0.005", "Probability (s) = 0.95", "Burn-in", "(M)", "Total", "(N)",
                  "Lower bound", "(Nmin)", "Dependence", "factor (I)", "3746", "%d" % fin.N[0], "%.3g" % fin.I[1]):
        assert piece in text, piece
    short = RafteryDiag(raftery_table(type("B", (), {"nmin": 3746})(), (1, 2)), np.full((1, 2), np.nan), 3746, 100, 0.025, 0.005,
                        0.95, 0.001)
    assert "You need a sample size of at least 3746" in str(short)


def test_c_entries_check_their_arguments_before_any_device_call():
    """No GPU here: every refusal below is returned, with its text, before the library touches the device."""
    import ctypes as C
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    assert L.fmcmc_chain_order_work_len(7, 3, 4) == 21 and L.fmcmc_chain_order_work_len(0, 3, 4) == 0
    assert L.fmcmc_raftery_work_len(7, 3, 64) == 21 and L.fmcmc_raftery_work_len(7, 3, 65) == 42
    assert L.fmcmc_raftery_out_len(7, 3, 16) == 21 * (4 + 160) and L.fmcmc_raftery_out_len(7, 3, 33) == 0
    fake = 4096                                                     # a non-null address nothing reads
    ranks = (C.c_int64 * 33)(*range(33))

    def raftery(N=100, S=100, row0=0, q=0.25, j0=1, nj=16, p=2, samples=fake):
        return L.fmcmc_raftery_dev(samples, 3, 4, S, row0, N, fake, p, q, j0, nj, fake, fake, None)

    def order(N=100, S=100, nranks=4, samples=fake, ranks_=ranks):
        return L.fmcmc_chain_order_dev(samples, 3, 4, S, 0, N, fake, 2, ranks_, nranks, fake, fake, None)

    for call, code, text in ((lambda: raftery(samples=None), abi.ERR_ARG, "null argument"),
                             (lambda: raftery(N=2), abi.ERR_ARG, "too short"),
                             (lambda: raftery(row0=1), abi.ERR_ARG, "outside the 100 rows"),
                             (lambda: raftery(q=-0.1), abi.ERR_ARG, "q = -0.1"),
                             (lambda: raftery(q=float("nan")), abi.ERR_ARG, "q = nan"),
                             (lambda: raftery(j0=0), abi.ERR_ARG, "j0 = 0"),
                             (lambda: raftery(nj=0), abi.ERR_ARG, "nj = 0"),
                             (lambda: raftery(nj=33), abi.ERR_ARG, "nj = 33"),
                             (lambda: raftery(p=0), abi.ERR_ARG, "p = 0"),
                             (lambda: raftery(N=3162278, S=3162278), abi.ERR_UNSUPPORTED, "3162278"),
                             (lambda: order(samples=None), abi.ERR_ARG, "null argument"),
                             (lambda: order(ranks_=None), abi.ERR_ARG, "null argument"),
                             (lambda: order(nranks=0), abi.ERR_ARG, "nranks = 0"),
                             (lambda: order(nranks=33), abi.ERR_ARG, "nranks = 33"),
                             (lambda: order(N=3, S=3), abi.ERR_ARG, "ranks[3] = 3"),
                             (lambda: order(N=3162278, S=3162278), abi.ERR_UNSUPPORTED, "3162278")):
        assert call() == code and text in abi.last_error(), (text, abi.last_error())
