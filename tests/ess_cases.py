"""What tests/test_ess_host.py and tests/test_gpu_rank_ess.py share: a second restatement of the rank-normalised effective sample
size on zero-padded FFT autocovariances, the inputs, and the error bounds of the device's autocovariance
sums, derived from how csrc/diag_ess.hpp sums them and never from what it returns.  A plain module next to
tests/rhat_cases.py."""
import numpy as np

import rhat_cases as rc

U = rc.U
KINDS = ("bulk", "q05", "q95", "mean")


# ------------------------------------------------------------------------------------------------ the definition, a second time
def fft_ess(y):
    """y [m][n] -> (ess, tau, K): the definition with float64 zero-padded FFT autocovariances and a plain loop for the pairs"""
    y = np.asarray(y, dtype=np.float64)
    m, n = y.shape
    size = 1
    while size < 2 * n:
        size *= 2
    u = y - y.mean(axis=1, keepdims=True)
    f = np.fft.rfft(u, size, axis=1)
    c = np.fft.irfft(f * np.conj(f), size, axis=1)[:, :n] / n          # c_s(t), biased
    S = c.sum(axis=0)
    W = S[0] / m * n / (n - 1)
    V = S[0] / m + (y.mean(axis=1).var(ddof=1) if m > 1 else 0.0)
    if V == 0:
        return float("nan"), float("nan"), 1
    rho = lambda t: 1.0 if t == 0 else 1.0 - (W - S[t] / m) / V
    pairs = [rho(0) + rho(1)]
    j = 1
    while True:
        if 2 * j + 1 > n - 3:
            break
        P = rho(2 * j) + rho(2 * j + 1)
        if not P >= 0:
            break
        pairs.append(P)
        j += 1
    K = j
    for i in range(1, K):
        pairs[i] = min(pairs[i], pairs[i - 1])
    tau = -1.0 + 2.0 * sum(pairs)
    if 2 * K <= n - 3 and rho(2 * K) > 0:
        tau += rho(2 * K)
    tau = max(tau, 1.0 / np.log10(m * n))
    return m * n / tau, tau, K


def fft_ess_all(data):
    """data [C][N][p] -> [p][4]: bulk, q05, q95, mean through fft_ess"""
    from fmcmc_amd.convergence import rank_z, split_chains
    from fmcmc_amd.summary import type7_order_ranks, type7_quantiles
    sp = split_chains(data)
    M = sp.shape[0] * sp.shape[1]
    out = np.empty((sp.shape[2], 4))
    for j in range(sp.shape[2]):
        x = sp[:, :, j] + 0.0
        q = type7_quantiles(np.sort(x.ravel())[type7_order_ranks(M, [0.05, 0.95])], M, [0.05, 0.95])
        for kind, y in enumerate((rank_z(x)[0], (x <= q[0]) * 1.0, (x <= q[1]) * 1.0, x)):
            out[j, kind] = fft_ess(y)[0]
    return out


# ------------------------------------------------------------------------------------------------ inputs
def ar1(rng, phi, Cn, N):
    """stationary AR(1) rows [C][N] with unit innovations"""
    e = rng.standard_normal((Cn, N))
    x = np.empty((Cn, N))
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - phi * phi)
    for i in range(1, N):
        x[:, i] = phi * x[:, i - 1] + e[:, i]
    return x


NCOLS = 4


def make_inputs(Cn, N, seed, row0=3):
    """x [C][4][S], S odd with guard rows (1e9 / -1e9) on both sides of the window [row0, row0 + N), the columns:
    0  AR(1), phi = 0.6: the cut is a pair that turns negative
    1  values drawn from five integers: heavy ties, q05 and q95 sit on runs of equal values
    2  all equal
    3  iid normal around 100: centring matters"""
    rng = np.random.default_rng(seed)
    S = row0 + N + 2
    S += 1 - S % 2
    x = np.empty((Cn, NCOLS, S))
    x[:, 0] = ar1(rng, 0.6, Cn, S)
    x[:, 1] = rng.integers(-2, 3, size=(Cn, S)).astype(np.float64)
    x[:, 2] = 3.25
    x[:, 3] = 100.0 + rng.standard_normal((Cn, S))
    x[:, :, :row0] = 1e9
    x[:, :, row0 + N:] = -1e9
    return np.ascontiguousarray(x), row0


def window(x, row0, N):
    """data [C][N][k] of the window, the layout ess_host takes"""
    return np.ascontiguousarray(x[:, :, row0:row0 + N].transpose(0, 2, 1))


def ramp(Cn, N, seed):
    """[C][N]: a straight line plus small noise: rho stays positive at every lag, the cap sets the cut"""
    rng = np.random.default_rng(seed)
    return np.arange(N)[None, :] * 1.0 + 0.01 * rng.standard_normal((Cn, N))


def alternating(Cn, N, seed):
    """[C][N]: +1, -1, +1, ... plus noise of standard deviation 0.5: rho_t is near (-1)^t 0.8 (1 - t / n), so P_0 = 1 + rho_1 and
    P_1 = rho_2 + rho_3 are both small; the noise decides the sign of P_1, and the seed is one at which it is negative"""
    rng = np.random.default_rng(seed)
    return np.where(np.arange(N)[None, :] % 2 == 0, 1.0, -1.0) + 0.5 * rng.standard_normal((Cn, N))


def series_of(x):
    """x [m][n], the pooled split values of a column -> (the four series in the order of KINDS, as the host forms them; q [2])"""
    from fmcmc_amd.convergence import rank_z
    from fmcmc_amd.summary import type7_order_ranks, type7_quantiles
    x = np.asarray(x, dtype=np.float64) + 0.0
    q = type7_quantiles(np.sort(x.ravel())[type7_order_ranks(x.size, [0.05, 0.95])], x.size, [0.05, 0.95])
    return (rank_z(x)[0], (x <= q[0]) * 1.0, (x <= q[1]) * 1.0, x), q


def host_case(y, kind, L=None):
    """The host's answer for one series y [m][n] and what the device may differ by: a namespace of g (geyer_tau's), c, E [m][L]
    and S, ES [L] (autocov_ref, sum_bound; L: the lags the host needed unless given), mu, e_mean [m], and, where the ESS is a number,
    bound (on the ESS) and gap (see ess_bound).  kind 0: the device's scores are fmh_qnorm's, the host's ndtri's."""
    from types import SimpleNamespace
    from fmcmc_amd.convergence import ess_series_host
    g, S_host = ess_series_host(y)
    shift = bulk_shift(y) if kind == 0 else 0.0
    c, E = autocov_ref(y, S_host.size if L is None else L, shift)
    S, ES = sum_bound(c, E)
    e_mean = rc.moment_bounds(y)[0] + (rc.score_shift_bounds(y)[0] if kind == 0 else 0.0)
    mu = np.asarray(y, dtype=np.longdouble).mean(axis=1).astype(np.float64)
    r = SimpleNamespace(g=g, c=c, E=E, S=S, ES=ES, mu=mu, e_mean=e_mean, bound=None, gap=None)
    if not np.isnan(g.ess):
        m, n = np.shape(y)
        r.bound, r.gap = ess_bound(S.astype(np.float64), ES.astype(np.float64), mu, e_mean, m, n, g.K)
    return r


# ------------------------------------------------------------------------------------------------ bounds
def autocov_ref(y, L, shift=0.0):
    """y [m][n], the series as the device holds it (or, with `shift`, within shift [m] of it, value by value) -> (c [m][L], E [m][L]):
    the exact biased autocovariances c_s(t) in np.longdouble, t < L, and how far the device's may be from them.
      centring  the device's mean of a split chain is within e = moment_bounds(y) of the exact one and the difference
                y - mean is rounded once: the centred value is (u_i + h_i)(1 + d_i), |h_i| <= h = e + shift, |d_i| <= U;
      products  sum (u_i + h_i)(u_{i+t} + h_{i+t}) is within h B + (n - t) h^2 of sum u_i u_{i+t}, B = sum (|u_i| + |u_{i+t}|);
      sum       n - t products, each rounded once (or not at all, when the matrix core fuses it), added in an order we do not
                state, then the 3 joins of the four wavefronts and the division by n: every term carries at most
                2 (centring) + 1 + (n - t - 1) + 3 + 1 <= n + 6 roundings, whatever the order: gamma(n + 8) covers it;
    so E = (gamma(n + 8) A' + h B + (n - t) h^2) / n with A' = sum (|u_i| + h)(|u_{i+t}| + h), plus n 2^-64 A / n for the
    reference's own roundings."""
    y = np.asarray(y, dtype=np.longdouble)
    m, n = y.shape
    e_mean = rc.moment_bounds(y)[0].astype(np.longdouble)
    h = (e_mean + shift)[:, None]
    u = y - (y.sum(axis=1) / n)[:, None]
    a = np.abs(u)
    c = np.empty((m, L), dtype=np.longdouble)
    E = np.empty((m, L), dtype=np.longdouble)
    g, ref = rc.gamma(n + 8), n * 2.0 ** -64
    for t in range(L):
        c[:, t] = (u[:, :n - t] * u[:, t:]).sum(axis=1) / n
        A = (a[:, :n - t] * a[:, t:]).sum(axis=1)
        B = a[:, :n - t].sum(axis=1) + a[:, t:].sum(axis=1)
        A2 = A + h[:, 0] * B + (n - t) * h[:, 0] ** 2
        E[:, t] = ((g + ref) * A2 + h[:, 0] * B + (n - t) * h[:, 0] ** 2) / n
    return c, E


def sum_bound(c, E):
    """c, E [m][L] -> (S [L], ES [L]): S(t) = sum_s c_s(t) and the device's distance from it: the chains' own bounds and the
    m - 1 additions in the order s = 0, 1, ..."""
    m = c.shape[0]
    return c.sum(axis=0), E.sum(axis=0) + rc.gamma(m) * (np.abs(c) + E).sum(axis=0)


def bulk_shift(z):
    """z [m][n] -> [m]: how far a centred score of the device may be from the host's, fmh_qnorm against ndtri: the value by
    QNORM_REL |z|, the mean by the mean of that"""
    a = rc.QNORM_REL * np.abs(np.asarray(z, dtype=np.float64))
    return a.max(axis=1) + a.mean(axis=1)


def ess_bound(S, ES, means, e_mean, m, n, K):
    """How far the device's ESS may be from geyer_tau(S), given |S'(t) - S(t)| <= ES(t), means within e_mean, and the same cut
    K: (bound on ESS, the smallest |P_j| - dP_j over j <= K (j = K only where a pair decided the cut), which must be positive
    for K to be safe).
      W = S0 / m n / (n - 1): dW = ES0 / m n / (n - 1);  V = S0 / m + var(means): dV = ES0 / m + (4 e sum|d_s| + 4 m e^2) / (m - 1)
      rho_t = 1 - (W - S_t / m) / V:  drho_t <= (dW + ES_t / m) / (V - dV) + |W - S_t / m| dV / (V (V - dV))
      P_j: dP_j = drho_2j + drho_2j+1; the running minimum moves by at most max_{i <= j} dP_i; the end term max(rho_2K, 0) by
      drho_2K; the floor is a maximum and moves by no more.  tau: dtau = 2 sum_j max_{i<=j} dP_i + drho_2K + 4 (K + 2) U tau for
      the roundings of the finish.  ESS = m n / tau: dESS = m n dtau / (tau (tau - dtau))."""
    S = np.asarray(S, dtype=np.float64)
    ES = np.asarray(ES, dtype=np.float64)
    mu = np.asarray(means, dtype=np.float64)
    e = float(np.max(e_mean))
    d = mu - mu.mean()
    W = S[0] / m * n / (n - 1)
    V = S[0] / m + (d * d).sum() / (m - 1)
    dW = ES[0] / m * n / (n - 1)
    dV = ES[0] / m + (4.0 * e * np.abs(d).sum() + 4.0 * m * e * e) / (m - 1)
    assert V > 2.0 * dV, "the bound needs V well above its own error"
    top = min(2 * K + 2, S.size)
    rho = 1.0 - (W - S[:top] / m) / V
    rho[0] = 1.0
    drho = (dW + ES[:top] / m) / (V - dV) + np.abs(W - S[:top] / m) * dV / (V * (V - dV))
    drho[0] = 0.0
    have = top // 2
    P = rho[0:2 * have:2] + rho[1:2 * have:2]
    dP = drho[0:2 * have:2] + drho[1:2 * have:2]
    upto = min(K + 1, have) if (K < have and not P[K] >= 0) else K
    gap = float(np.min(np.abs(P[:upto]) - dP[:upto]))
    run = np.minimum.accumulate(P[:K])
    tau = -1.0 + 2.0 * run.sum()
    dtau = 2.0 * np.maximum.accumulate(dP[:K]).sum()
    if 2 * K <= n - 3:
        tau += max(rho[2 * K], 0.0)
        dtau += drho[2 * K]
    tau = max(tau, 1.0 / np.log10(m * n))
    dtau += 4.0 * (K + 2) * U * tau
    assert tau > 2.0 * dtau
    return m * n * dtau / (tau * (tau - dtau)), gap


def pooled_sd_bound(r, y):
    """(the exact pooled sd of y [m][n] with divisor m n - 1, how far the device's may be from it): the device forms the pooled
    variance as (n S(0) + n sum_s d_s^2) / (m n - 1) from the values' S(0) (within r.ES[0]) and the split chains' means (within
    e: sum d_s^2 moves by at most 4 e sum|d_s| + 4 m e^2); a square root moves by at most the change of its argument over twice
    the smaller root; 8 U sd covers the roundings of these few operations."""
    y = np.asarray(y, dtype=np.longdouble)
    m, n = y.shape
    var = y.var(ddof=1)
    d = y.mean(axis=1) - y.mean()
    e = float(np.max(r.e_mean))
    dvar = float((n * r.ES[0] + n * (4.0 * e * np.abs(d).sum() + 4.0 * m * e * e)) / (m * n - 1))
    assert var > 2.0 * dvar
    return float(np.sqrt(var)), dvar / (2.0 * float(np.sqrt(var - dvar))) + 8.0 * U * float(np.sqrt(var))
