"""summary(ans) / McmcBatch.summary() / effective_size(ans) of an McmcBatch (summary.summary_batch: one grouped call,
fmcmc_summary_groups_dev, and one copy back) on the GPU: element d is what summary(ans[d]) returns, field for field and in its
printed text; a ragged result takes one call per distinct row count; the grouped call is quicker than the loop it replaces."""
import importlib
import time

import numpy as np
import pytest

from test_gpu_parity import _bits_equal

pytestmark = pytest.mark.gpu

PER_CHAIN = ("mean", "sd", "tsse", "ess", "spec0", "order")


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def assert_same_summary(a, b):
    """two McmcSummary objects: every field, to the bit, and the printed text"""
    assert _bits_equal(a.statistics, b.statistics) and _bits_equal(a.quantiles, b.quantiles) and _bits_equal(a.ess, b.ess)
    assert a.statistics.shape == b.statistics.shape and a.quantiles.shape == b.quantiles.shape
    for f in PER_CHAIN:
        x, y = getattr(a.per_chain, f), getattr(b.per_chain, f)
        assert x.shape == y.shape and x.dtype == y.dtype and _bits_equal(x, y), f
    assert (a.start, a.end, a.thin, a.nchain, a.niter) == (b.start, b.end, b.thin, b.nchain, b.niter)
    assert a.probs == b.probs and a.varnames == b.varnames
    assert str(a) == str(b)


def assert_batch_is_the_loop(F, ans, **kw):
    got = F.summary(ans, **kw)
    D = len(ans)
    assert isinstance(got, F.McmcSummaryBatch) and isinstance(got, list) and len(got) == D
    each = [F.summary(ans[d], **kw) for d in range(D)]
    for d in range(D):
        assert isinstance(got[d], F.McmcSummary)
        assert_same_summary(got[d], each[d])
    assert _bits_equal(got.statistics, np.stack([s.statistics for s in each]))
    assert _bits_equal(got.quantiles, np.stack([s.quantiles for s in each]))
    assert _bits_equal(got.ess, np.stack([s.ess for s in each]))
    p = each[0].statistics.shape[0]
    assert got.statistics.shape == (D, p, 4) and got.quantiles.shape == (D, p, len(each[0].probs)) and got.ess.shape == (D, p)
    for f in PER_CHAIN:
        assert _bits_equal(getattr(got.per_chain, f), np.concatenate([getattr(s.per_chain, f) for s in each])), f
        assert getattr(got.per_chain, f).shape == (D * ans.nchains, p)
    return got


@pytest.fixture(scope="module")
def tiny(T):
    """MCMC_batch on 5 datasets x 3 chains: linear regression, n = 50, two covariates (k = 4), 400 steps, kernel_normal"""
    import fmcmc_amd as F
    rng = np.random.default_rng(21)
    data = []
    for d in range(5):
        X = rng.standard_normal((50, 2))
        data.append((X, 1.0 + d + X @ np.array([2.0, -1.0]) + (1.0 + 0.2 * d) * rng.standard_normal(50)))
    b = F.model_batch(F.gaussian_linreg(X, y) for X, y in data)
    return F.MCMC_batch(np.array([0.0, 0.0, 0.0, 1.0]), b, 400, nchains=3, seed=5, kernel=F.kernel_normal(scale=0.05))


@pytest.mark.parametrize("kw", [dict(), dict(cols=[2, 0]), dict(quantiles=()), dict(quantiles=(0.5, 0.0, 1.0), cols=[3])])
def test_summary_of_a_batch_is_summary_of_every_dataset(T, tiny, kw):
    import fmcmc_amd as F
    assert len(tiny) == 5 and tiny.nchains == 3 and not tiny.ragged
    got = assert_batch_is_the_loop(F, tiny, **kw)
    again = tiny.summary(**kw)
    assert _bits_equal(again.statistics, got.statistics) and _bits_equal(again.quantiles, got.quantiles)
    if "quantiles" not in kw:
        assert "2. Quantiles for each variable:" in str(got[0]) and got[0].niter == 400


def test_effective_size_of_a_batch(T, tiny):
    import fmcmc_amd as F
    for kw in (dict(), dict(cols=[2, 0])):
        ess = F.effective_size(tiny, **kw)
        assert ess.shape == (5, len(kw.get("cols", range(4))))
        for d in range(5):
            assert _bits_equal(ess[d], F.effective_size(tiny[d], **kw))
        assert _bits_equal(tiny.effective_size(**kw), ess)
        assert _bits_equal(ess, F.summary(tiny, **kw).ess)


def _synthetic(T, F, D, Cm, k, rows, seed, nrows=None):
    """an McmcBatch built by hand over seeded series (every dataset around a level of its own), NaN behind each dataset's rows"""
    g = T.Generator(device="cpu").manual_seed(seed)
    e = T.randn((D * Cm, k, rows), generator=g, dtype=T.float64)
    x = e.clone()
    x[:, :, 1:] += 0.5 * e[:, :, :-1]
    x += 100.0 * T.arange(D, dtype=T.float64).repeat_interleave(Cm)[:, None, None] + T.arange(k, dtype=T.float64)[None, :, None]
    kw = {}
    if nrows is not None:
        for d, nr in enumerate(nrows):
            x[d * Cm:(d + 1) * Cm, :, nr:] = float("nan")
        kw = dict(nrows=np.asarray(nrows), steps=3 * np.asarray(nrows), converged=[True] * D)
    dc = F.DeviceChains(x.cuda(), None, None, 3 * np.arange(1, rows + 1), 3, ["v%d" % j for j in range(k)], 0, D * Cm)
    dc.accept_count = T.zeros(D * Cm, dtype=T.int64, device="cuda")
    return F.McmcBatch(dc, D, Cm, **kw)


def test_a_ragged_batch_takes_one_call_per_distinct_row_count(T, monkeypatch):
    import fmcmc_amd as F
    S = importlib.import_module("fmcmc_amd.summary")       # (fmcmc_amd.summary is the function)
    nrows = [40, 25, 40, 7, 25]
    ans = _synthetic(T, F, 5, 2, 3, 40, 31, nrows=nrows)
    assert ans.ragged
    calls = []
    real = S.enqueue_summary_groups

    def counted(dc, ngroups, cpg, row0, N, cols, probs, active=None, want_chains=True):
        calls.append((int(N), None if active is None else active.cpu().numpy().tolist()))
        return real(dc, ngroups, cpg, row0, N, cols, probs, active, want_chains)

    monkeypatch.setattr(S, "enqueue_summary_groups", counted)
    got = ans.summary()
    assert calls == [(7, [0, 0, 0, 1, 0]), (25, [0, 1, 0, 0, 1]), (40, [1, 0, 1, 0, 0])]
    ess = ans.effective_size()
    assert len(calls) == 6
    monkeypatch.undo()
    for d, nr in enumerate(nrows):
        one = F.summary(ans[d])
        assert_same_summary(got[d], one)
        assert (got[d].start, got[d].end, got[d].thin, got[d].niter) == (3, 3 * nr, 3, nr)       # the dataset's own labels
        assert _bits_equal(ess[d], F.effective_size(ans[d]))
        assert np.isfinite(got[d].statistics).all() and np.isfinite(got[d].quantiles).all()
    assert got.statistics.shape == (5, 3, 4)


def test_non_finite_rows_name_their_dataset(T):
    import fmcmc_amd as F
    ans = _synthetic(T, F, 4, 2, 2, 30, 32)
    ans.history._samples[5, 1, 11] = float("inf")
    with pytest.raises(ValueError, match=r"dataset 2: 1 non-finite value\(s\) among the rows to summarise \(columns \[1\]\)"):
        ans.summary()
    with pytest.raises(ValueError, match="dataset 2: 1 non-finite"):
        ans.effective_size()
    assert len(ans.summary(cols=[0])) == 4


def test_the_grouped_call_is_quicker_than_the_loop(T):
    """an ordering, not a number: 64 datasets x 4 chains x 500 rows x 3 columns, wall clock to the returned host object, best
    of three after a warm-up, both in this process.  The loop enqueues some twenty kernels, synchronises and copies back per
    dataset; the grouped call does that once.  (The ratio is printed with -s; tools/bench_batch_summary.py records it.)"""
    import fmcmc_amd as F
    ans = _synthetic(T, F, 64, 4, 3, 500, 33)

    def best(f):
        f()
        times = []
        for _ in range(3):
            T.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            T.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return min(times)

    loop = best(lambda: [F.summary(ans[d]) for d in range(64)])
    grouped = best(lambda: F.summary(ans))
    print("loop %.3f ms, grouped %.3f ms, ratio %.1f" % (1e3 * loop, 1e3 * grouped, loop / grouped))
    assert grouped < loop
