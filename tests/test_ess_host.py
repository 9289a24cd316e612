"""The host side of the rank-normalised effective sample size: geyer_tau on hand-made S(t) whose
answers are worked out below, ess_host against a second restatement (tests/ess_cases.py: FFT autocovariances, a plain loop),
closed forms, the tail quantiles on heavy ties, and convergence_rhat's unchanged form without min_ess.  No GPU."""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest

import ess_cases as ec


# ------------------------------------------------------------------------------------------------ geyer_tau by hand
def from_rho(rho, n):
    """(S, m, n, means) with W = V = 1, so that rho_t of the definition is the given rho[t] (t >= 1): two chains, m = 2;
    W = S0 / 2 n / (n - 1) = 1 gives S0 = 2 (n - 1) / n; V = S0 / 2 + var(means) = 1 gives var(means) = 1 / n, the means
    +-a with 2 a^2 = 1 / n; rho_t = 1 - (1 - S_t / 2) / 1 = S_t / 2."""
    S = 2.0 * np.asarray(rho, dtype=np.float64)
    S[0] = 2.0 * (n - 1) / n
    a = np.sqrt(1.0 / (2.0 * n))
    return S, 2, n, [a, -a]


def tau_of(rho, n):
    from fmcmc_amd import geyer_tau
    return geyer_tau(*from_rho(rho, n))


def test_a_cut_at_the_first_pair():
    """P_0 = 1 + 0.5, P_1 = -0.3 - 0.4 < 0: K = 1; rho_2 = -0.3 adds nothing: tau = -1 + 2 (1.5) = 2, ESS = 202 / 2"""
    g = tau_of([1, 0.5, -0.3, -0.4, 0.9, 0.9], 101)
    assert g.K == 1 and g.tau == pytest.approx(2.0, rel=1e-12) and g.ess == pytest.approx(101.0, rel=1e-12)


def test_the_end_term_present_and_absent():
    """P_1 = 0.2 - 0.4 < 0: K = 1; rho_2 = 0.2 > 0 is added: tau = 2 + 0.2.  With rho_2 = -0.2 it is not: tau = 2."""
    g = tau_of([1, 0.5, 0.2, -0.4], 101)
    assert g.K == 1 and g.tau == pytest.approx(2.2, rel=1e-12)
    g = tau_of([1, 0.5, -0.2, -0.4], 101)
    assert g.K == 1 and g.tau == pytest.approx(2.0, rel=1e-12)


def test_pairs_that_rise_again():
    """P = 1.4, 0.2, 0.5, then -0.4: K = 3; the monotone step turns 0.5 into 0.2: tau = -1 + 2 (1.4 + 0.2 + 0.2) = 2.6 (3.2
    without it); rho_6 = -0.5 adds nothing"""
    g = tau_of([1, 0.4, 0.1, 0.1, 0.3, 0.2, -0.5, 0.1], 101)
    assert g.K == 3 and g.tau == pytest.approx(2.6, rel=1e-12)


def test_a_cut_by_the_lag_cap():
    """rho = 0.5 at every lag.  n = 9: lags 0 .. 6; j = 3 has 2 j + 1 = 7 > 6: K = 3, P = 1.5, 1, 1: -1 + 2 (3.5) = 6, and
    lag 2 K = 6 is within the cap with rho_6 > 0: tau = 6.5.  n = 10: lags 0 .. 7; j = 4 has 9 > 7: K = 4, P = 1.5, 1, 1, 1:
    -1 + 2 (4.5) = 8, lag 8 is beyond the cap: tau = 8."""
    g = tau_of([1] + [0.5] * 6, 9)
    assert g.K == 3 and g.tau == pytest.approx(6.5, rel=1e-12) and g.ess == pytest.approx(18 / 6.5, rel=1e-12)
    g = tau_of([1] + [0.5] * 7, 10)
    assert g.K == 4 and g.tau == pytest.approx(8.0, rel=1e-12)


def test_the_floor_is_taken():
    """P_0 = 1 - 0.9 = 0.1, P_1 < 0: tau = -1 + 0.2 < 0 is raised to 1 / log10(202): ESS = 202 log10(202)"""
    g = tau_of([1, -0.9, -0.5, -0.5], 101)
    assert g.K == 1 and g.tau == 1.0 / np.log10(202.0) and g.ess == pytest.approx(202.0 * np.log10(202.0), rel=1e-12)


def test_a_constant_series_gives_nan_and_a_nan_pair_cuts():
    from fmcmc_amd import geyer_tau
    g = geyer_tau(np.zeros(8), 4, 10, [1.5] * 4)
    assert np.isnan(g.tau) and np.isnan(g.ess) and g.K == 1
    S, m, n, mu = from_rho([1, 0.5, 0.5, 0.5, 0.5, 0.5], 101)
    S[4] = np.nan                                    # P_2 is NaN: K = 2, tau = -1 + 2 (1.5 + 1)
    g = geyer_tau(S, m, n, mu)
    assert g.K == 2 and g.tau == pytest.approx(4.0, rel=1e-12)


def test_an_undecided_pair_test_asks_for_more_lags():
    from fmcmc_amd.summary import LagsNeeded
    with pytest.raises(LagsNeeded):
        tau_of([1] + [0.5] * 5, 101)


# ------------------------------------------------------------------------------------------------ a second restatement
@pytest.mark.parametrize("Cn, N", [(1, 8), (2, 9), (3, 101), (4, 2000)])
def test_ess_host_against_the_fft_restatement(Cn, N):
    from fmcmc_amd import ess_host
    x, row0 = ec.make_inputs(Cn, N, 300 + N)
    data = ec.window(x, row0, N)
    h = ess_host(data)
    have = np.stack([h.bulk, h.tail_q05, h.tail_q95, h.mean], axis=1)
    want = ec.fft_ess_all(data)
    print(have, want)
    assert np.isnan(have[2]).all() and np.isnan(h.mcse_mean[2])          # the constant column
    ok = ~np.isnan(want)
    assert np.array_equal(ok, ~np.isnan(have)) and ok[[0, 3]][:, [0, 3]].all()
    assert np.allclose(have[ok], want[ok], rtol=1e-9, atol=0.0)
    assert np.array_equal(np.isnan(h.tail), np.isnan(h.tail_q05) | np.isnan(h.tail_q95))
    both = ~np.isnan(h.tail)
    assert np.array_equal(h.tail[both], np.minimum(h.tail_q05, h.tail_q95)[both])
    assert np.allclose(h.mcse_mean[ok[:, 3]], (h.pooled_sd / np.sqrt(h.mean))[ok[:, 3]], rtol=1e-15)


# ------------------------------------------------------------------------------------------------ closed forms
# The yardstick is the closed form; the margin is five standard deviations of the estimator, which were estimated from 300
# seeds each at this shape (4 chains of 2000 rows, M = 8000) with the longdouble restatement:
#   ess_mean, AR(1) phi = 0:    mean 7889, sd 267 (3.3 % of 8000)    -> margin 17 %
#   ess_mean, AR(1) phi = 0.5:  mean 2654, sd 166 (6.2 % of 2667)    -> margin 31 %
#   ess_mean, AR(1) phi = 0.9:  mean  425, sd  58 (13.7 % of 421)    -> margin 69 %
#   ess_bulk, iid normal:       mean 7893, sd 248 (3.1 % of 8000)    -> margin 16 %
@pytest.mark.parametrize("phi, margin", [(0.0, 0.17), (0.5, 0.31), (0.9, 0.69)])
def test_ess_mean_of_ar1_against_the_closed_form(phi, margin):
    from fmcmc_amd import ess_host
    x = ec.ar1(np.random.default_rng(41), phi, 4, 2000)
    h = ess_host(x[:, :, None])
    want = 8000.0 * (1.0 - phi) / (1.0 + phi)
    print(phi, h.mean[0], want)
    assert abs(h.mean[0] - want) <= margin * want


def test_ess_bulk_of_iid_draws_against_the_closed_form():
    from fmcmc_amd import ess_host
    x = np.random.default_rng(42).standard_normal((4, 2000, 1))
    h = ess_host(x)
    print(h.bulk[0])
    assert abs(h.bulk[0] - 8000.0) <= 0.16 * 8000.0


# ------------------------------------------------------------------------------------------------ tail, heavy ties
@pytest.mark.parametrize("Cn, N", [(2, 9), (3, 101), (4, 2000)])
def test_tail_quantiles_and_counts_on_heavy_ties(Cn, N):
    from fmcmc_amd import ess_host
    from fmcmc_amd.convergence import split_chains
    from fmcmc_amd.summary import type7_order_ranks, type7_quantiles
    x, row0 = ec.make_inputs(Cn, N, 500 + N)
    data = ec.window(x, row0, N)[:, :, 1:2]
    h = ess_host(data)
    pooled = split_chains(data)[:, :, 0].ravel()
    q = type7_quantiles(np.sort(pooled)[type7_order_ranks(pooled.size, [0.05, 0.95])], pooled.size, [0.05, 0.95])
    assert h.q05.view(np.uint64)[0] == q.view(np.uint64)[0] and h.q95.view(np.uint64)[0] == q.view(np.uint64)[1]
    assert h.counts[0].tolist() == [int(np.sum(pooled <= q[0])), int(np.sum(pooled <= q[1]))]
    assert set(np.unique(pooled)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and h.counts[0, 1] > 0.9 * pooled.size


# ------------------------------------------------------------------------------------------------ convergence_rhat
class _Dev:
    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def _stub_rhat(monkeypatch, Cn, p):
    """check_device with the device call replaced: `out` of fmcmc_rank_rhat_dev with split-chain means 0, 0.1, 0.2, ... and unit
    variances for both kinds"""
    summary = importlib.import_module("fmcmc_amd.summary")     # (fmcmc_amd.summary is the function)
    m = 2 * Cn
    out = np.zeros((p, 4 * m + 2))
    for kind in range(2):
        out[:, 2 * m * kind:2 * m * (kind + 1):2] = 0.1 * np.arange(m)
        out[:, 2 * m * kind + 1:2 * m * (kind + 1):2] = 1.0
    monkeypatch.setattr(summary, "enqueue_rank_rhat", lambda dc, row0, N, cols: (_Dev(out), None, np.asarray(cols)))
    chains = SimpleNamespace(iters=np.arange(1, 41), nrows=40, _samples=SimpleNamespace(shape=(Cn, p, 40)))
    return chains, summary.rhat_finish(out, Cn, 10)


def test_without_min_ess_the_checker_is_what_it_was(monkeypatch):
    import fmcmc_amd as f
    summary = importlib.import_module("fmcmc_amd.summary")     # (fmcmc_amd.summary is the function)
    chains, fin = _stub_rhat(monkeypatch, 2, 3)

    def never(*a, **k):
        raise AssertionError("no ESS call without min_ess")

    monkeypatch.setattr(summary, "enqueue_rank_ess", never)
    chk = f.convergence_rhat(freq=20, threshold=10.0)
    assert chk.min_ess is None and chk.check_device(chains, np.arange(3)) is True
    val = float(fin.rhat.max())
    assert chk.msg == "Rank-normalised split R-hat: %.4f." % val and chk.last == val
    assert len(chk.history) == 1 and len(chk.history[0]) == 3
    assert chk.history[0][0] == 40 and chk.history[0][1] == val and np.array_equal(chk.history[0][2], fin.rhat)


@pytest.mark.parametrize("bulk, want, least", [([500.0, 450.0, 900.0], True, 420.0), ([500.0, 350.0, 900.0], False, 350.0),
                                               ([500.0, np.nan, 900.0], False, np.nan)])
def test_with_min_ess_both_must_hold(monkeypatch, bulk, want, least):
    import fmcmc_amd as f
    summary = importlib.import_module("fmcmc_amd.summary")     # (fmcmc_amd.summary is the function)
    chains, fin = _stub_rhat(monkeypatch, 2, 3)
    tail = np.array([420.0, 800.0, 700.0])
    monkeypatch.setattr(summary, "enqueue_rank_ess", lambda dc, row0, N, cols: (_Dev(None), None, np.asarray(cols)))
    monkeypatch.setattr(summary, "ess_finish", lambda out, Cn, N: SimpleNamespace(bulk=np.array(bulk), tail=tail))
    chk = f.convergence_rhat(freq=20, threshold=10.0, min_ess=400)
    assert chk.check_device(chains, np.arange(3)) is want
    assert chk.msg == "Rank-normalised split R-hat: %.4f. Smallest ESS: %.1f." % (float(fin.rhat.max()), least)
    assert len(chk.history[0]) == 4 and np.array_equal(chk.history[0][3], np.minimum(bulk, tail), equal_nan=True)
    low = f.convergence_rhat(freq=20, threshold=0.5, min_ess=1)      # R-hat above its threshold: the ESS does not rescue it
    assert low.check_device(chains, np.arange(3)) is False
