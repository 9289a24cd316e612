"""GPU tests of the device-side summary (fmcmc_amd/summary.py -> csrc/summary.hip).

Yardsticks, all on the host copy of the same rows:
 * the table fmcmc's README prints for its first run (tests/golden/readme_summary.json);
 * np.sort for the order statistics: bit for bit, no tolerance;
 * numpy in longdouble for the moments, within the a-priori bound n 2^-53 mean(|terms|) that holds for any summation order;
 * the host restatement of coda::spectrum0.ar in longdouble for spec0 / order / ESS / time-series SE.  The tolerance is
   computed in the test: the worst relative distance, over the same series, between the float64 host restatement (two
   summation orders) and the longdouble one, times 16 (both are float64 evaluations of one formula that differ in summation
   order only; the factor covers that a worst case seen over a few hundred series underestimates the common bound).
   Measured on an MI355X for the inputs below (printed by the tests with -s): see DESIGN.md section 5.10.
"""
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
R = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "readme_summary.json")))
LD = np.longdouble
U = 2.0 ** -53


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fmcmc_amd import engine
    return engine


def sig(x, d):
    return float("%.*g" % (d, x))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ host references
def host_series(y, dtype=LD, flip=False):
    """fmcmc_amd.convergence.spectrum0_ar restated in `dtype` (flip: every sum runs from the last row to the first).
    Returns mean, var, spec0, order and the gap between the best and the second-best AIC."""
    y = np.asarray(y).astype(dtype)
    n = y.size
    ssum = (lambda v: v[::-1].sum()) if flip else (lambda v: v.sum())
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
    M = int(min(n - 1, np.floor(10 * np.log10(n))))
    r = np.array([ssum(x[:n - l] * x[l:]) for l in range(M + 1)], dtype=dtype) / dtype(n)
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
    return out


def spec0_tolerance(columns, label):
    """16 x the worst relative distance between the float64 host restatement (the package's spectrum0_ar, and the restatement
    above summed in the opposite direction) and the longdouble one, over `columns`.  Also returns the longdouble references."""
    from fmcmc_amd.convergence import spectrum0_ar
    worst, refs, flips = 0.0, [], 0
    for y in columns:
        ref = host_series(y, LD)
        refs.append(ref)
        if ref["spec0"] == 0:
            continue
        s_a, o_a = spectrum0_ar(y)
        b = host_series(y, np.float64, flip=True)
        flips += (o_a != ref["order"]) + (b["order"] != ref["order"])
        for s in (s_a, b["spec0"]):
            worst = max(worst, float(abs(LD(s) - ref["spec0"]) / ref["spec0"]))
    gaps = [r["gap"] for r in refs]
    print("\n[%s] %d series: worst float64-vs-longdouble relative distance of spec0 %.3g -> tolerance %.3g; smallest AIC gap "
          "%.3g; float64 / longdouble host orders differ %d times" % (label, len(refs), worst, 16 * worst, min(gaps), flips))
    return 16 * worst, refs


def check_series(per_chain, host, cols, tol, refs=None):
    """per_chain: McmcSummary.per_chain; host [C][k][N]; every (chain, column) against the longdouble restatement."""
    C_, _, N = host.shape
    left_out, worst, n = 0, 0.0, 0
    for c in range(C_):
        for a, col in enumerate(cols):
            ref = refs[n] if refs is not None else host_series(host[c, col], LD)
            n += 1
            if ref["spec0"] == 0:
                assert per_chain.spec0[c, a] == 0.0 and per_chain.ess[c, a] == 0.0 and per_chain.order[c, a] == 0
                continue
            if ref["gap"] < 1e-6:          # the order is an argmin: two AIC values tie
                left_out += 1
                continue
            assert per_chain.order[c, a] == ref["order"], (c, col)
            ess = LD(N) * ref["var"] / ref["spec0"]
            tsse = np.sqrt(ref["spec0"] / LD(N))
            for got, want in ((per_chain.spec0[c, a], ref["spec0"]), (per_chain.ess[c, a], ess), (per_chain.tsse[c, a], tsse)):
                d = float(abs(LD(got) - want) / abs(want))
                worst = max(worst, d)
                assert d <= tol, (c, col, float(got), float(want), d, tol)
    assert left_out <= 0.01 * n, (left_out, n)
    print("device vs longdouble: worst relative distance %.3g over %d series (tolerance %.3g, %d left out)"
          % (worst, n, tol, left_out))


def check_moments(sm, host, cols):
    """means / variances, per chain and pooled, against longdouble numpy within n 2^-53 mean(|terms|)."""
    C_, _, N = host.shape
    for a, col in enumerate(cols):
        x = host[:, col, :].astype(LD)
        m_c = x.sum(1) / N
        v_c = ((x - m_c[:, None]) ** 2).sum(1) / (N - 1)
        assert np.all(np.abs(sm.per_chain.mean[:, a] - m_c) <= N * U * np.abs(x).mean(1))
        assert np.all(np.abs(sm.per_chain.sd[:, a].astype(LD) ** 2 - v_c) <= N * U * v_c + 4 * U * v_c)   # (+ the sqrt and its square)
        n = C_ * N
        m = x.sum() / n
        v = ((x - m) ** 2).sum() / (n - 1)
        assert abs(sm.statistics[a, 0] - m) <= n * U * np.abs(x).mean()
        assert abs(LD(sm.statistics[a, 1]) ** 2 - v) <= n * U * v + 4 * U * v
        assert abs(LD(sm.statistics[a, 2]) ** 2 * n - v) <= n * U * v + 8 * U * v


def check_exact(dc, probs, cols=None):
    """The two order statistics of every prob equal np.sort of the pooled host copy bit for bit, and the quantile is the
    type-7 formula applied to them, bit for bit."""
    from fmcmc_amd.summary import window_stats
    host = dc.samples.cpu().numpy()
    C_, k, N = host.shape
    cols_ = list(range(k)) if cols is None else list(cols)
    _, os_, _ = window_stats(dc, 0, N, cols, probs)
    sm = dc.summary(quantiles=probs, cols=cols)
    n = C_ * N
    for a, col in enumerate(cols_):
        srt = np.sort(host[:, col, :].ravel())
        for q, prob in enumerate(probs):
            index = 1.0 + np.float64(n - 1) * np.float64(prob)
            lo, hi = int(np.floor(index)), int(np.ceil(index))
            xlo, xhi = srt[lo - 1], srt[hi - 1]
            assert _bits(os_[a, q, 0]) == _bits(xlo), (col, prob, os_[a, q, 0], xlo)
            assert _bits(os_[a, q, 1]) == _bits(xhi), (col, prob, os_[a, q, 1], xhi)
            h = index - lo
            want = (1.0 - h) * xlo + h * xhi if (index > lo and xhi != xlo) else xlo
            assert _bits(sm.quantiles[a, q]) == _bits(want), (col, prob)
    return sm, host


# ------------------------------------------------------------------------------------------------ inputs
@pytest.fixture(scope="module")
def g1(E, O, readme_data):
    """README.md:156-166: the first run, fed R's own Mersenne-Twister stream (tests/test_gpu_api.py), kept on the device."""
    import torch
    from fmcmc_amd import _abi as abi, DeviceChains
    X, y = readme_data
    gm = E.DeviceModel(abi.FAM_GAUSSIAN_LINREG, X, y, intercept=True, guard=True)
    g = O.RRng(1215)
    logu = np.log(g.runif(5000))
    z = np.zeros((5000, 3))
    for i in range(1, 5000):
        z[i] = g.rnorm(3)
    gk = E.KernelSpec(abi.KERNEL_NORMAL, 3, np.zeros(3), np.ones(3), np.full(3, -E.DBL_MAX), np.full(3, E.DBL_MAX),
                      np.zeros(3, np.uint8), warmup=0)
    st = E.ChainState(np.array([[0, 0, O.r_sd(y)]], dtype=np.float64), 3)
    r = E.sweep(gm, gk, st, 5000, fed_logu=torch.as_tensor(logu[None, :]).cuda().contiguous(),
                fed_z=torch.as_tensor(z[None, :, :]).cuda().contiguous())
    torch.cuda.synchronize()
    return DeviceChains(r.samples, None, None, r.iters, 1, ["par1", "par2", "par3"], 0, 1)


def _philox48(readme_data, kernel, **kw):
    from fmcmc_amd import MCMC, gaussian_linreg
    X, y = readme_data
    init = np.array([0.0, 0.0, np.std(y, ddof=1)])[None, :] + 0.1 * np.random.default_rng(48).standard_normal((48, 3))
    init[:, 2] = np.abs(init[:, 2])
    return MCMC(init, gaussian_linreg(X, y), 3000, nchains=48, burnin=500, thin=2, seed=11, kernel=kernel, _return_device=True,
                **kw)


@pytest.fixture(scope="module")
def normal48(E, readme_data):
    from fmcmc_amd import kernel_normal
    return _philox48(readme_data, kernel_normal(scale=0.15))


@pytest.fixture(scope="module")
def ram48(E, readme_data):
    from fmcmc_amd import kernel_ram
    return _philox48(readme_data, kernel_ram(), keep_logpost=False, keep_draws=False)


@pytest.fixture(scope="module")
def headline(E):
    """The headline call's output: 1024 chains x 5 parameters x 10^4 kept rows (bench.py, config c2)."""
    from conftest import synth_linreg
    from fmcmc_amd import MCMC, gaussian_linreg, kernel_normal
    X, y = synth_linreg(10000, 3, 20260102, beta=np.array([3.0, 2.0, -1.0, 0.5]))
    init = np.array([0.0, 0.0, 0.0, 0.0, np.std(y, ddof=1)])[None, :] + 0.1 * np.random.default_rng(7).standard_normal((1024, 5))
    init[:, 4] = np.abs(init[:, 4])
    return MCMC(init, gaussian_linreg(X, y), 10000, nchains=1024, seed=1215, kernel=kernel_normal(scale=0.02),
                _return_device=True, keep_logpost=False, keep_draws=False)


def ar1(phi, n, rng, mu=0.0):
    e = rng.standard_normal(n)
    x = np.empty(n)
    x[0] = e[0] / np.sqrt(1 - phi * phi) if phi < 1 else e[0]
    for i in range(1, n):
        x[i] = phi * x[i - 1] + e[i]
    return x + mu


def upload(arr, thin=1, start=1):
    """arr [C][N][p] -> DeviceChains through the public path (an McmcList, uploaded by the package)."""
    from fmcmc_amd import Mcmc, McmcList
    from fmcmc_amd.summary import _as_device_chains
    return _as_device_chains(McmcList(Mcmc(a, start=start, thin=thin) for a in arr))


# ------------------------------------------------------------------------------------------------ tests
def test_readme_table_from_the_device(g1):
    """README.md:183-201: every printed number of summary(ans), from the device, at its printed significant digits."""
    sm = g1.summary()
    assert (sm.start, sm.end, sm.thin, sm.nchain, sm.niter) == (R["start"], R["end"], R["thin"], R["nchain"], R["niter"])
    assert sm.varnames == R["varnames"]
    st = sm.statistics
    assert [sig(v, 4) for v in st[:, 0]] == R["mean"]
    assert [sig(v, 4) for v in st[:, 1]] == [sig(v, 4) for v in R["sd"]]
    assert [sig(v, 4) for v in st[:, 2]] == R["naive_se"]
    assert [sig(v, 4) for v in st[:, 3]] == [sig(v, 4) for v in R["ts_se"]]
    assert [[sig(v, 4) for v in row] for row in sm.quantiles] == R["quantiles"]
    assert list(sm.per_chain.order[0]) == [28, 35, 36]
    text = str(sm)
    print(text)
    assert "par1 3.113 0.17593 0.002488       0.024341" in text and "par3 3.978 4.070 4.101 4.102 4.226" in text
    assert np.array_equal(_bits(g1.effective_size()), _bits(sm.ess))


def test_order_statistics_are_exact_one_chain(g1):
    check_exact(g1, (0.025, 0.25, 0.5, 0.75, 0.975))
    check_exact(g1, (0.0, 1.0, 0.5, 1.0 / 3.0))


def test_order_statistics_and_moments_48_chains(normal48):
    assert tuple(normal48.samples.shape) == (48, 3, 1250)
    sm, host = check_exact(normal48, (0.025, 0.25, 0.5, 0.75, 0.975))
    assert (sm.start, sm.end, sm.thin, sm.nchain, sm.niter) == (502, 3000, 2, 48, 1250)
    check_moments(sm, host, [0, 1, 2])
    check_exact(normal48, (0.0, 0.001, 0.999, 1.0), cols=[2, 0])
    sub = normal48.summary(cols=[2, 0])
    assert sub.varnames == [sm.varnames[2], sm.varnames[0]]
    assert np.array_equal(_bits(sub.statistics), _bits(sm.statistics[[2, 0]]))
    assert np.array_equal(_bits(sub.quantiles), _bits(sm.quantiles[[2, 0]]))


def test_history_with_a_row_stride_beyond_its_rows(E, readme_data):
    """MCMC_with_conv_checker allocates the rows of all bulks and stops early: ld_rows > S, and with an odd number of unused
    rows the windows of the chains are 8-byte aligned only."""
    from fmcmc_amd import MCMC, gaussian_linreg, kernel_normal, convergence_gelman
    X, y = readme_data
    init = np.array([0.0, 0.0, np.std(y, ddof=1)])[None, :] + 0.1 * np.random.default_rng(8).standard_normal((8, 3))
    init[:, 2] = np.abs(init[:, 2])
    dc = MCMC(init, gaussian_linreg(X, y), 3999, nchains=8, seed=3, kernel=kernel_normal(scale=0.15),
              conv_checker=convergence_gelman(freq=1000, threshold=1e6), _return_device=True)
    assert dc.capacity == 3999 and dc.nrows == 1000 and dc.capacity > dc.nrows
    sm, host = check_exact(dc, (0.025, 0.5, 0.975, 1.0))
    check_moments(sm, host, [0, 1, 2])
    tol, refs = spec0_tolerance([host[c, j] for c in range(8) for j in range(3)], "history")
    check_series(sm.per_chain, host, [0, 1, 2], tol, refs)


def test_headline_shape_exact_moments_and_time(headline):
    """1024 x 5 x 10^4 once: exact order statistics, moments, and the one timing claim of the feature: summary() (kernels +
    the small copy back) takes less wall time than copying the same rows to the host."""
    import torch
    assert tuple(headline.samples.shape) == (1024, 5, 10000)
    sm, host = check_exact(headline, (0.025, 0.25, 0.5, 0.75, 0.975))
    check_moments(sm, host, range(5))
    del host
    t_sum, t_copy = [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        headline.summary()                  # ends with the copy of its results: synchronised
        t_sum.append(time.perf_counter() - t0)
    headline.to_host()
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        headline.to_host()
        t_copy.append(time.perf_counter() - t0)
    print("\nheadline shape: summary() best of five %.3f ms, to_host() best of five %.3f ms" % (1e3 * min(t_sum), 1e3 * min(t_copy)))
    assert min(t_sum) < min(t_copy)


def test_spec0_order_ess_tsse_per_chain(g1, normal48, ram48):
    rng = np.random.default_rng(20260)
    phis = np.linspace(0.0, 0.99, 32)
    synth = np.stack([ar1(phi, 5000, rng, mu=3.0)[:, None] for phi in phis])        # [32][5000][1]
    inputs = [("README first run", g1, None), ("32 synthetic AR(1)", upload(synth), None),
              ("48 chains kernel_normal(scale = .15)", normal48, None), ("48 chains kernel_ram", ram48, None)]
    for label, dc, _ in inputs:
        host = dc.samples.cpu().numpy()
        C_, k, _n = host.shape
        tol, refs = spec0_tolerance([host[c, j] for c in range(C_) for j in range(k)], label)
        sm = dc.summary()
        check_series(sm.per_chain, host, list(range(k)), tol, refs)
        # the pooled columns follow from the per-chain ones
        n = C_ * _n
        tsse = np.sqrt(np.mean([[r["spec0"] for r in refs[c * k:(c + 1) * k]] for c in range(C_)], axis=0) / n)
        assert np.all(np.abs(sm.statistics[:, 3] - tsse) <= tol * tsse)
        ess = np.sum([[_n * r["var"] / r["spec0"] for r in refs[c * k:(c + 1) * k]] for c in range(C_)], axis=0)
        assert np.all(np.abs(sm.ess - ess) <= tol * ess)


def test_series_longer_than_the_lds_tile():
    """45000 rows per chain do not fit the LDS: the second pass walks tiles with a halo (AR orders up to 46)."""
    rng = np.random.default_rng(45)
    arr = np.stack([np.stack([ar1(0.9, 45000, rng, mu=-2.0), ar1(0.5, 45000, rng, mu=10.0)], axis=1) for _ in range(2)])
    dc = upload(arr)
    sm, host = check_exact(dc, (0.025, 0.5, 0.975))
    check_moments(sm, host, [0, 1])
    tol, refs = spec0_tolerance([host[c, j] for c in range(2) for j in range(2)], "45000 rows")
    check_series(sm.per_chain, host, [0, 1], tol, refs)


def test_degenerate_series_and_non_finite_values():
    rng = np.random.default_rng(5)
    n = 2000
    arr = np.stack([np.stack([np.full(n, 2.5), 0.25 + 0.001 * np.arange(n), ar1(0.6, n, rng, mu=1.0)], axis=1)
                    for _ in range(4)])
    dc = upload(arr, thin=3, start=10)
    sm = dc.summary()
    pc = sm.per_chain
    assert np.all(pc.spec0[:, :2] == 0.0) and np.all(pc.ess[:, :2] == 0.0) and np.all(pc.order[:, :2] == 0)
    assert np.all(sm.ess[:2] == 0.0) and np.all(sm.statistics[:2, 3] == 0.0)
    assert np.all(sm.statistics[0, :3] == [2.5, 0.0, 0.0]) and np.all(sm.quantiles[0] == 2.5)
    host = dc.samples.cpu().numpy()
    tol, refs = spec0_tolerance([host[c, j] for c in range(4) for j in range(3)], "degenerate")
    check_series(pc, host, [0, 1, 2], tol, refs)             # the third column is not poisoned by its neighbours
    assert np.all(np.isfinite(sm.statistics)) and np.all(np.isfinite(sm.quantiles)) and sm.ess[2] > 0
    assert (sm.start, sm.end, sm.thin) == (10, 10 + 3 * (n - 1), 3)
    bad = arr.copy()
    bad[2, 777, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        upload(bad).summary()
    bad[2, 777, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        upload(bad).effective_size()


def test_geweke_of_every_chain(normal48):
    from fmcmc_amd.convergence import geweke_diag, _window_rows
    host = normal48.samples.cpu().numpy()
    C_, k, N = host.shape
    iters = normal48.iters
    z = normal48.geweke()
    assert z.shape == (C_, k)
    tol, _ = spec0_tolerance([host[c, j] for c in range(C_) for j in range(k)], "geweke (whole series)")
    # the windows' own series set the tolerance; the difference of two means carries their summation bounds
    start, end = float(iters[0]), float(iters[-1])
    wins = [_window_rows(iters, start, np.ceil(start + 0.1 * (end - start))), _window_rows(iters, np.floor(end - 0.5 * (end - start)), end)]
    tolw = max(spec0_tolerance([host[c, j, lo:hi] for c in range(C_) for j in range(k)], "geweke window %d" % i)[0]
               for i, (lo, hi) in enumerate(wins))
    tolw = max(tolw, tol)
    worst = 0.0
    for c in range(C_):
        want = geweke_diag(host[c].T, iters)
        for j in range(k):
            if not np.isfinite(want[j]):
                assert not np.isfinite(z[c, j])
                continue
            v = [np.array(host_series(host[c, j, lo:hi], LD)["spec0"] / (hi - lo), dtype=np.float64) for lo, hi in wins]
            mean_bound = sum((hi - lo) * U * np.abs(host[c, j, lo:hi]).mean() for lo, hi in wins)
            bound = abs(want[j]) * tolw + 2 * mean_bound / np.sqrt(v[0] + v[1])
            worst = max(worst, abs(z[c, j] - want[j]) / bound)
            assert abs(z[c, j] - want[j]) <= bound, (c, j, z[c, j], want[j], bound)
    print("geweke: worst |z - host| / bound = %.3g" % worst)


def test_summary_only_reads(normal48):
    before = [t.clone() for t in (normal48._samples, normal48._logpost, normal48._draws)]
    normal48.summary()
    normal48.effective_size()
    normal48.geweke()
    import torch
    torch.cuda.synchronize()
    for b, a in zip(before, (normal48._samples, normal48._logpost, normal48._draws)):
        assert torch.equal(b.view(torch.int64), a.view(torch.int64))


def test_calls_are_reproducible(normal48):
    a, b = normal48.summary(), normal48.summary()
    for f in ("statistics", "quantiles", "ess"):
        assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f)))
    assert np.array_equal(_bits(a.per_chain.spec0), _bits(b.per_chain.spec0))


def test_refuses_sharded_chains(normal48, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="sharded"):
        normal48.summary()
    with pytest.raises(NotImplementedError, match="sharded"):
        normal48.effective_size()
