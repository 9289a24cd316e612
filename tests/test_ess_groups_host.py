"""The host side of the grouped effective sample size (summary.py: geyer_tau_rows, ess_rows_finish, ess_groups_finish,
EssDiagBatch, the dispatch of ess()) without a GPU: the vectorised finish against ess_finish / geyer_tau row by row TO THE BIT on
`out` arrays built on the host from convergence.autocov_sums (rounded to float64), in the layout and with the rounds of lags of
fmcmc_rank_ess_dev, and the two length functions of the C-ABI, which need no device."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import ess_cases as ec


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind in "iu":
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def host_column(x):
    """x [C][N], one column of a window -> its row of `out` as the device lays it out: per series the split chains' means and
    variances, L (whole rounds of lags, as far as geyer_tau needed them), K, S(0 .. L) and NaN above; then the info."""
    from fmcmc_amd.convergence import ess_series_host
    from fmcmc_amd.summary import ess_lag_cap
    Cn, N = x.shape
    m, n = 2 * Cn, N // 2
    sp = np.stack([x[:, :n], x[:, N - n:]], axis=1).reshape(m, n)
    series, q = ec.series_of(sp)
    cap = ess_lag_cap(n)
    kl = 2 * m + 2 + cap
    row = np.full(4 * kl + 7, np.nan)
    for kind, y in enumerate(series):
        y = np.asarray(y, dtype=np.float64)
        g, S = ess_series_host(y)
        part = row[kind * kl:(kind + 1) * kl]
        part[0:2 * m:2] = y.astype(np.longdouble).mean(axis=1).astype(np.float64)
        part[1:2 * m:2] = y.var(axis=1, ddof=1)
        part[2 * m], part[2 * m + 1] = S.size, g.K
        part[2 * m + 2:2 * m + 2 + S.size] = S.astype(np.float64)
    v = sp + 0.0
    row[4 * kl:] = [0.0, q[0], q[1], v.mean(), v.std(ddof=1), v.min(), v.max()]
    return row


@functools.lru_cache(maxsize=None)
def host_rows():
    """(Cn, N, out [R][.], what each row is): every way the cut comes about, in one array"""
    Cn, N = 2, 1100                                  # n = 550, cap 548: the rounds end at 256, 512, 548
    rng = np.random.default_rng(5)
    cols = {
        "ar1": ec.ar1(rng, 0.6, Cn, N),              # a pair turns negative in the first round
        "ar1 slow": ec.ar1(rng, 0.97, Cn, N),
        "ramp": ec.ramp(Cn, N, 61),                  # rho stays positive: the cap
        "alternating": ec.alternating(Cn, N, 2),     # K = 1
        "ties": rng.integers(-2, 3, size=(Cn, N)).astype(np.float64),
        "constant": np.full((Cn, N), 3.25),
        "offset": 100.0 + rng.standard_normal((Cn, N)),
        # nine tenths of the values are the largest: q95 is the largest value and x <= q95 holds everywhere
        "constant indicator": np.where(rng.random((Cn, N)) < 0.9, 1.0, rng.random((Cn, N))),
    }
    out = np.stack([host_column(x) for x in cols.values()])
    out.setflags(write=False)
    return Cn, N, out, list(cols)


FIELDS = ("bulk", "tail_q05", "tail_q95", "tail", "mean", "mcse_mean", "tau_bulk", "q05", "q95", "non_finite", "pooled_mean",
          "pooled_sd", "lags", "computed", "device_lags")


def assert_rows_equal_ess_finish(out, Cn, N):
    from fmcmc_amd.summary import ess_finish, ess_rows_finish
    got = ess_rows_finish(out, Cn, N)
    for r in range(out.shape[0]):
        want = ess_finish(out[r], Cn, N)
        for f in FIELDS:
            assert _same(getattr(got, f)[r:r + 1], getattr(want, f)), (r, f, getattr(got, f)[r], getattr(want, f))
    return got


def test_the_cases_are_what_they_claim():
    Cn, N, out, names = host_rows()
    from fmcmc_amd.summary import ess_finish
    fin = ess_finish(out, Cn, N)
    n, cap = N // 2, N // 2 - 2
    at = {name: r for r, name in enumerate(names)}
    assert fin.lags[at["alternating"], 0] == 1 and fin.lags[at["alternating"], 3] == 1
    assert fin.lags[at["ramp"], 0] == cap // 2 and fin.computed[at["ramp"], 0] == cap and fin.computed[at["ramp"], 3] == cap
    assert 1 < fin.lags[at["ar1"], 3] < 128 and fin.computed[at["ar1"], 3] == 256
    assert fin.lags[at["ar1 slow"], 3] > fin.lags[at["ar1"], 3]
    assert np.isnan(fin.bulk[at["constant"]]) and np.isnan(fin.mcse_mean[at["constant"]]) and (fin.lags[at["constant"]] == 1).all()
    ci = at["constant indicator"]
    assert np.isnan(fin.tail_q95[ci]) and np.isnan(fin.tail[ci]) and np.isfinite(fin.bulk[ci]) and np.isfinite(fin.tail_q05[ci])
    assert np.isfinite(fin.bulk[[at[k] for k in ("ar1", "ar1 slow", "ramp", "alternating", "ties", "offset")]]).all()


def test_the_vectorised_finish_equals_ess_finish_to_the_bit():
    Cn, N, out, names = host_rows()
    got = assert_rows_equal_ess_finish(out, Cn, N)
    assert got.bulk.shape == (len(names),) and got.lags.shape == (len(names), 4)
    again = assert_rows_equal_ess_finish(out[::-1], Cn, N)          # a row's answer does not depend on its neighbours
    assert _same(again.bulk[::-1], got.bulk) and _same(again.lags[::-1], got.lags)
    assert_rows_equal_ess_finish(out[2:3], Cn, N)                   # one row


@pytest.mark.parametrize("K", [1, 2, 3, 7, 8, 9, 127, 128, 129, 130, 255, 256, 257, 1000, 2047])
def test_geyer_tau_rows_at_every_length_of_the_sum(K):
    """np.sum changes its order with the length (unrolled by 8, blocks of 128): rows cut at K by a negative pair, among rows
    with other cuts, against geyer_tau row by row; the running minimum is made to bite by noise on a decaying rho"""
    from fmcmc_amd.summary import geyer_tau, geyer_tau_rows
    m, n = 4, 4200
    cap = n - 2
    rng = np.random.default_rng(K)
    R = 6
    t = np.arange(cap)
    Ks = [K, K, max(1, K - 1), K + 1, 1, K]
    S = np.empty((R, cap))
    L = np.empty(R, dtype=np.int64)
    means = rng.standard_normal((R, m)) * 0.01
    for r in range(R):
        S[r] = m * (0.999 ** t) * (1.0 + 0.05 * rng.random(cap))
        S[r, 2 * Ks[r]:2 * Ks[r] + 2] = -3.0 * m                 # P at Ks[r] is negative
        L[r] = min(cap, max(256, 512 * ((2 * Ks[r] + 2 + 511) // 512)))
    tau, ess, Kg, W, V = geyer_tau_rows(S, L, m, n, means)
    for r in range(R):
        g = geyer_tau(S[r, :L[r]], m, n, means[r])
        assert g.K == Kg[r] == Ks[r]
        for have, want in ((tau[r], g.tau), (ess[r], g.ess), (W[r], g.W), (V[r], g.V)):
            assert _bits(have) == _bits(want), (r, have, want)


def test_a_row_that_stopped_short_raises_as_geyer_tau_does():
    from fmcmc_amd.summary import LagsNeeded, ess_finish, ess_rows_finish
    Cn, N, out, names = host_rows()
    m = 2 * Cn
    kl = 2 * m + 2 + N // 2 - 2
    ramp = names.index("ramp")
    short = out.copy()
    short[ramp, 3 * kl + 2 * m] = 256.0                # the values of the ramp: one round of the three it needs
    short[ramp, 3 * kl + 2 * m + 2 + 256:4 * kl] = np.nan
    with pytest.raises(LagsNeeded) as single:
        ess_finish(short, Cn, N)
    with pytest.raises(LagsNeeded) as rows:
        ess_rows_finish(short, Cn, N)
    assert str(rows.value) == str(single.value) and "undecided after 256 lags of at most 548" in str(rows.value)
    ar = names.index("ar1")
    both = short.copy()                                # two rows that raise: the first in order speaks, as in the loop
    both[ar, 2 * m] = 2.0 * out[ar, 2 * m + 1]         # the AR(1) scores: no lag from 2 K on, so no pair that fails
    with pytest.raises(LagsNeeded) as single:
        ess_finish(both, Cn, N)
    with pytest.raises(LagsNeeded) as rows:
        ess_rows_finish(both, Cn, N)
    assert str(rows.value) == str(single.value) and "undecided after %d lags" % both[ar, 2 * m] in str(rows.value)
    # the cap sets K and the lag 2 K = n - 3 behind it is missing: an odd cap, one lag short of it
    from fmcmc_amd.summary import geyer_tau, geyer_tau_rows
    n13 = 13
    S = np.tile(4.0 * 0.9 ** np.arange(11), (3, 1))
    means = np.zeros((3, 2))
    with pytest.raises(LagsNeeded) as single:
        geyer_tau(S[1, :10], 2, n13, means[1])
    with pytest.raises(LagsNeeded) as rows:
        geyer_tau_rows(S, [11, 10, 11], 2, n13, means)
    assert str(rows.value) == str(single.value) == "geyer_tau: lag 10 is needed, 10 lags were given"
    tau, _ess, K, _W, _V = geyer_tau_rows(S, [11, 11, 11], 2, n13, means)
    assert (K == 5).all() and _bits(tau[0]) == _bits(geyer_tau(S[0], 2, n13, means[0]).tau)
    bad = out.copy()
    bad[ar, 2 * m] = 1.0                               # L < 2: geyer_tau's ValueError
    with pytest.raises(ValueError, match="between 2 and n - 2 lags are needed") as rows:
        ess_rows_finish(bad, Cn, N)
    with pytest.raises(ValueError) as single:
        ess_finish(bad, Cn, N)
    assert str(rows.value) == str(single.value) and not isinstance(rows.value, LagsNeeded)


def test_masked_and_non_finite_rows():
    """a row still at its NaN prefill (a masked group) and a row with non-finite values take no part and disturb no other"""
    from fmcmc_amd.summary import ess_groups_finish
    Cn, N, out, names = host_rows()
    D, p = 4, 2
    o = out.reshape(D, p, -1).copy()
    o[1] = np.nan                                    # dataset 1 masked
    o[2, 1, -7] = 3.0                                # dataset 2, column 1: three non-finite values
    got = ess_groups_finish(o, Cn, N)
    full = ess_groups_finish(out.reshape(D, p, -1), Cn, N)
    for f in FIELDS:
        a, b = getattr(got, f), getattr(full, f)
        assert a.shape[:2] == (D, p)
        assert _same(a[0], b[0]) and _same(a[3], b[3]) and _same(a[2, 0], b[2, 0]), f
        if a.dtype.kind == "f":
            assert np.isnan(a[1]).all() or f in ("q05", "q95", "non_finite", "pooled_mean", "pooled_sd"), f
        else:
            assert (a[1] == 0).all() and (a[2, 1] == 0).all(), f
    assert np.isnan(got.non_finite[1]).all() and got.non_finite[2, 1] == 3.0 and np.isnan(got.bulk[2, 1])
    assert_rows_equal_ess_finish(o.reshape(D * p, -1), Cn, N)
    none = ess_groups_finish(np.full_like(o, np.nan), Cn, N)
    assert np.isnan(none.bulk).all() and (none.lags == 0).all()


def test_groups_finish_is_ess_finish_of_every_dataset():
    from fmcmc_amd.summary import ess_finish, ess_groups_finish
    Cn, N, out, names = host_rows()
    o = out.reshape(2, 4, -1)
    got = ess_groups_finish(o, Cn, N)
    for d in range(2):
        want = ess_finish(o[d], Cn, N)
        for f in FIELDS:
            assert _same(getattr(got, f)[d], getattr(want, f)), (d, f)


# ------------------------------------------------------------------------------------------------ EssDiagBatch, ess()
def test_ess_diag_batch_stacks_and_prints():
    import fmcmc_amd as f
    from fmcmc_amd.summary import ess_finish
    Cn, N, out, names = host_rows()
    o = out.reshape(2, 4, -1)
    diags = [f.EssDiag(ess_finish(o[d], Cn, N), Cn, N, ["a", "b", "c", "d"], 1, N) for d in range(2)]
    b = f.EssDiagBatch(diags)
    assert isinstance(b, list) and len(b) == 2 and b[1] is diags[1] and repr(b) == "<EssDiagBatch ndatasets=2 nvar=4>"
    for name in ("bulk", "tail", "tail_q05", "tail_q95", "mean", "mcse_mean", "tau_bulk", "q05", "q95"):
        assert getattr(b, name).shape == (2, 4) and _same(getattr(b, name), np.stack([getattr(d, name) for d in diags])), name
    assert b.lags.shape == (2, 4, 4) and b.lags.dtype == np.int64 and np.array_equal(b.lags[1], diags[1].lags)
    assert "Bulk" in str(b[0]) and repr(f.EssDiagBatch([])) == "<EssDiagBatch ndatasets=0 nvar=0>"


def test_ess_dispatches_a_batch_to_ess_batch(monkeypatch):
    import importlib
    import fmcmc_amd as f
    summary = importlib.import_module("fmcmc_amd.summary")          # (the package's `summary` is the function)
    ans = f.McmcBatch(SimpleNamespace(nrows=10), 3, 2)
    seen = []
    monkeypatch.setattr(summary, "ess_batch", lambda x, autoburnin=False, cols=None: seen.append((x, autoburnin, cols)) or "batch")
    assert f.ess(ans) == "batch" and f.ess(ans, True, [1]) == "batch" and ans.ess(cols=[0]) == "batch"
    assert seen == [(ans, False, None), (ans, True, [1]), (ans, False, [0])]
    monkeypatch.undo()
    with pytest.raises(TypeError, match="expects an McmcBatch"):
        f.ess_batch([1, 2])


# ------------------------------------------------------------------------------------------------ the C-ABI without a device
def test_the_length_functions():
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    top = L.fmcmc_rank_groups_max_values()
    for G, Cm, p, N in [(1, 1, 1, 8), (3, 1, 2, 9), (256, 4, 4, 2000), (2, 2, 3, 4096), (2, 1, 1, top), (5, 3, 4, 400)]:
        m, n = 2 * Cm, N // 2
        assert L.fmcmc_rank_ess_groups_out_len(G, Cm, p, N) == G * p * (4 * (2 * m + 2 + n - 2) + 7), (G, Cm, p, N)
        assert L.fmcmc_rank_ess_groups_work_len(G, Cm, p, N) == G * p * m * n, (G, Cm, p, N)
        assert L.fmcmc_rank_ess_groups_out_len(1, Cm, p, N) == L.fmcmc_rank_ess_out_len(Cm, p, N)
    for bad in [(0, 1, 1, 8), (1, 0, 1, 8), (1, 1, 0, 8), (1, 1, 1, 7), (1, 1, 1, top + 2), (1, 2, 1, top // 2 + 2),
                (2 ** 31, 1, 1, 8), (2 ** 30, 1, 2, 8), (-1, 1, 1, 8)]:
        assert L.fmcmc_rank_ess_groups_out_len(*bad) == 0 and L.fmcmc_rank_ess_groups_work_len(*bad) == 0, bad
    assert L.fmcmc_rank_ess_groups_out_len(2 ** 31 - 1, 1, 1, 8) == (2 ** 31 - 1) * 39
    for name in ("fmcmc_rank_ess_groups_work_len", "fmcmc_rank_ess_groups_out_len", "fmcmc_rank_ess_groups_dev"):
        assert name in abi.EXPORTS
