"""summary() / effective_size() of an McmcBatch and their C entry (fmcmc_summary_groups_dev), the parts that need no GPU: the
symbols, the work length, the refusals that come before any device work, the pure-numpy finish (summary_batch_finish) and the
bookkeeping of a ragged result, through a stand-in for the one call site (enqueue_summary_groups)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_abi import declared_functions


@pytest.fixture(scope="module")
def abi():
    from fmcmc_amd import _abi, build
    if build.needs_build():
        build.build()
    _abi.lib()
    return _abi


NEW = ["fmcmc_summary_groups_work_len", "fmcmc_summary_groups_dev"]


def test_the_new_entries_are_declared_and_exported_under_the_same_abi_version(abi):
    names = declared_functions()
    assert set(NEW) <= set(names) and set(NEW) <= set(abi.EXPORTS)
    L = abi.lib()
    assert all(hasattr(L, n) for n in NEW)
    assert L.fmcmc_abi_version() == 6 and abi.ABI_VERSION == 6
    assert "fmcmc_summary_groups_host" not in names                    # (no host-pointer variant)


def test_the_work_length_of_the_grouped_summary(abi):
    """ngroups chains_per_group p (72 + 4): the series work and the per-chain statistics; the select keeps its state in LDS"""
    L = abi.lib()
    for G, Cm, p, nprobs in [(1, 1, 1, 0), (6, 5, 5, 5), (256, 4, 5, 16), (301, 9, 64, 1)]:
        assert L.fmcmc_summary_groups_work_len(G, Cm, p, nprobs) == G * Cm * p * 76
        assert L.fmcmc_summary_groups_work_len(G, Cm, p, nprobs) == L.fmcmc_summary_work_len(G * Cm, p, 0)
    for bad in [(0, 4, 5, 5), (4, 0, 5, 5), (4, 4, 0, 5), (4, 4, 5, -1), (4, 4, 5, 17), (-1, 4, 5, 5), (1 << 31, 1 << 31, 1, 0),
                (1 << 20, 1 << 10, 64, 0)]:
        assert L.fmcmc_summary_groups_work_len(*bad) == 0, bad


@pytest.mark.parametrize("kw,code,substr", [
    (dict(G=0), "ERR_ARG", "at least 1"),
    (dict(Cm=0), "ERR_ARG", "at least 1"),
    (dict(Cm=-3), "ERR_ARG", "at least 1"),
    (dict(N=2), "ERR_ARG", "shorter than 3 rows"),
    (dict(row0=-1), "ERR_ARG", "outside the 100 rows"),
    (dict(row0=90, N=11), "ERR_ARG", "outside the 100 rows"),
    (dict(k=0), "ERR_ARG", "at least one parameter"),
    (dict(p=0), "ERR_ARG", "at least one column"),
    (dict(nprobs=17), "ERR_ARG", "nprobs = 17 outside [0, 16]"),
    (dict(nprobs=-1), "ERR_ARG", "nprobs = -1"),
    (dict(probs=[0.5, 1.5]), "ERR_ARG", "probs[1] = 1.5 is outside [0, 1]"),
    (dict(probs=[float("nan")]), "ERR_ARG", "probs[0]"),
    (dict(probs=None, nprobs=2), "ERR_ARG", "null argument"),
    (dict(samples=None), "ERR_ARG", "null argument"),
    (dict(cols=None), "ERR_ARG", "null argument"),
    (dict(work=None), "ERR_ARG", "null argument"),
    (dict(pooled=None), "ERR_ARG", "null argument"),
    (dict(G=1 << 20, Cm=1 << 20), "ERR_UNSUPPORTED", "exceed one launch"),
    (dict(G=1, Cm=1 << 31), "ERR_UNSUPPORTED", "exceed one launch"),
    (dict(G=1, Cm=1 << 30, p=1), "ERR_UNSUPPORTED", "fewer than 2^32 values"),
    (dict(N=3162278, S=4000000), "ERR_UNSUPPORTED", "AR order"),
])
def test_the_grouped_summary_checks_its_arguments_before_any_device_call(abi, kw, code, substr):
    """(the device pointers are made up and never followed: every one of these calls is refused first)"""
    a = dict(samples=8, G=3, Cm=2, k=7, S=100, row0=10, N=20, cols=8, p=5, active=None, probs=[0.5], nprobs=None, work=8,
             chain_stats=None, pooled=8)
    a.update(kw)
    pr = None if a["probs"] is None else np.ascontiguousarray(list(a["probs"]) + [0.5] * 17, dtype=np.float64)
    nprobs = a["nprobs"] if a["nprobs"] is not None else len(a["probs"])
    rc = abi.lib().fmcmc_summary_groups_dev(a["samples"], a["G"], a["Cm"], a["k"], a["S"], a["row0"], a["N"], a["cols"], a["p"],
                                            a["active"], None if pr is None else pr.ctypes.data_as(C.POINTER(C.c_double)), nprobs,
                                            a["work"], a["chain_stats"], a["pooled"], None)
    assert rc == getattr(abi, code)
    assert substr in abi.last_error() and "fmcmc_summary_groups_dev" in abi.last_error()


# ------------------------------------------------------------------------------------------------------- the host finish
def _device_arrays(x, probs, zero=None):
    """what fmcmc_summary_groups_dev leaves for the host series x [D][Cm][p][N], formed by numpy: pooled [D][5 p + 2 p nprobs]
    and chain_stats [D Cm][p][4] (spec0 made up: any positive number serves the finish; exactly 0 at the series `zero`)"""
    from fmcmc_amd.summary import type7_order_ranks
    D, Cm, p, N = x.shape
    mean, var = x.mean(axis=3), x.var(axis=3, ddof=1)
    spec0 = var * (1.5 + 0.1 * np.arange(p))
    if zero is not None:
        spec0[zero] = 0.0
    cs = np.stack([mean, var, spec0, np.full(mean.shape, 2.0)], axis=-1)              # [D][Cm][p][4]
    pooled_vals = x.transpose(0, 2, 1, 3).reshape(D, p, Cm * N)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.where(spec0 == 0.0, 0.0, N * var / spec0).sum(axis=1)
    ps = np.stack([pooled_vals.mean(axis=2), pooled_vals.var(axis=2, ddof=1), spec0.mean(axis=1), ess, np.zeros((D, p))], axis=-1)
    ranks = type7_order_ranks(Cm * N, np.asarray(probs, dtype=np.float64))
    os_ = np.sort(pooled_vals, axis=2)[:, :, ranks] if len(probs) else np.zeros((D, p, 0, 2))
    return np.concatenate([ps.reshape(D, -1), os_.reshape(D, -1)], axis=1), cs.reshape(D * Cm, p, 4), ps, os_, cs


def _same(a, b):
    u = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.shape(a) == np.shape(b) and np.array_equal(u(a), u(b))


@pytest.mark.parametrize("probs", [(0.025, 0.25, 0.5, 0.75, 0.975), (), (0.0, 1.0, 0.5)])
def test_summary_batch_finish_is_the_finish_of_summary_per_dataset(probs):
    S = importlib.import_module("fmcmc_amd.summary")       # (fmcmc_amd.summary is the function)
    D, Cm, p, N = 4, 3, 2, 50
    x = np.random.default_rng(3).standard_normal((D, Cm, p, N)) + 10.0 * np.arange(D)[:, None, None, None]
    pooled, chain, ps, os_, cs = _device_arrays(x, probs, zero=(0, 0, 0))
    assert cs[0, 0, 0, 2] == 0.0
    names = ["alpha", "beta"]
    got = S.summary_batch_finish(pooled, chain, Cm, N, probs, names, 11, 207, 4)
    assert len(got) == D
    for d in range(D):
        want = S.McmcSummary(S.finish_statistics(ps[d], Cm, N), S.type7_quantiles(os_[d], Cm * N, probs), probs, names, 11, 207, 4,
                             Cm, per_chain=S._per_chain(cs[d], N), ess=ps[d, :, 3].copy())
        g = got[d]
        assert isinstance(g, S.McmcSummary) and _same(g.statistics, want.statistics) and _same(g.quantiles, want.quantiles)
        assert _same(g.ess, want.ess) and g.quantiles.shape == (p, len(probs))
        for f in ("mean", "sd", "tsse", "ess", "spec0", "order"):
            assert _same(getattr(g.per_chain, f), getattr(want.per_chain, f)), f
        assert (g.start, g.end, g.thin, g.nchain, g.probs, g.varnames) == (11, 207, 4, Cm, tuple(probs), names)
        assert str(g) == str(want)
    only = S.summary_batch_finish(pooled, chain, Cm, N, probs, names, 11, 207, 4, datasets=[2, 0])
    assert len(only) == 2 and _same(only[0].statistics, got[2].statistics) and _same(only[1].quantiles, got[0].quantiles)
    stacked = S.McmcSummaryBatch(got)
    assert stacked.statistics.shape == (D, p, 4) and stacked.quantiles.shape == (D, p, len(probs)) and stacked.ess.shape == (D, p)
    assert stacked.per_chain.mean.shape == (D * Cm, p) and _same(stacked.per_chain.mean, cs[..., 0].reshape(D * Cm, p))
    assert _same(stacked.statistics[3], got[3].statistics) and "ndatasets=4" in repr(stacked)


# ------------------------------------------------------------------------------------------------- the ragged bookkeeping
class _FakeDevice:
    """stands in for enqueue_summary_groups: records every call and answers with torch CPU tensors made by numpy from the host
    series, NaN in the rows of the masked groups"""

    def __init__(self, x):
        self.x, self.calls = x, []                                     # x [D][Cm][k][rows]

    def __call__(self, dc, ngroups, cpg, row0, N, cols, probs, active=None, want_chains=True):
        import torch
        from fmcmc_amd.summary import _columns
        cols = _columns(dc, cols)
        mask = None if active is None else active.numpy().tolist()
        self.calls.append(dict(G=ngroups, Cm=cpg, row0=row0, N=N, cols=cols.tolist(), probs=tuple(probs), mask=mask,
                               want_chains=want_chains, dc=dc))
        pooled, chain, _ps, _os, _cs = _device_arrays(self.x[:, :, cols, row0:row0 + N], probs)
        if mask is not None:
            off = np.asarray(mask) == 0
            pooled[off] = np.nan
            chain.reshape(ngroups, cpg, -1)[off] = np.nan
        return torch.as_tensor(pooled), torch.as_tensor(chain) if want_chains else None, None, cols


def _host_batch(nrows, D=5, Cm=2, k=3, rows=40, thin=5):
    import torch
    import fmcmc_amd as F
    x = np.random.default_rng(4).standard_normal((D, Cm, k, rows)) + np.arange(D)[:, None, None, None]
    dc = F.DeviceChains(torch.as_tensor(x.reshape(D * Cm, k, rows)), None, None, thin * np.arange(1, rows + 1), thin,
                        ["a", "b", "c"], 0, D * Cm)
    kw = {} if nrows is None else dict(nrows=nrows, steps=thin * np.asarray(nrows), converged=[True] * D)
    return x, F.McmcBatch(dc, D, Cm, **kw)


def test_a_ragged_result_takes_one_call_per_distinct_row_count(monkeypatch):
    S = importlib.import_module("fmcmc_amd.summary")       # (fmcmc_amd.summary is the function)
    nrows = [40, 25, 40, 7, 25]
    x, ans = _host_batch(nrows)
    fake = _FakeDevice(x)
    monkeypatch.setattr(S, "enqueue_summary_groups", fake)
    got = ans.summary(quantiles=(0.1, 0.9), cols=[2, 0])
    assert [(c["N"], c["mask"]) for c in fake.calls] == [(7, [0, 0, 0, 1, 0]), (25, [0, 1, 0, 0, 1]), (40, [1, 0, 1, 0, 0])]
    for c in fake.calls:
        assert (c["G"], c["Cm"], c["row0"], c["cols"], c["probs"], c["want_chains"]) == (5, 2, 0, [2, 0], (0.1, 0.9), True)
        assert c["dc"] is ans.history
    assert isinstance(got, S.McmcSummaryBatch) and len(got) == 5
    for d, nr in enumerate(nrows):
        pooled, chain, *_ = _device_arrays(x[d:d + 1, :, [2, 0], :nr], (0.1, 0.9))
        want = S.summary_batch_finish(pooled, chain, 2, nr, (0.1, 0.9), ["c", "a"], 5, 5 * nr, 5)[0]
        assert _same(got[d].statistics, want.statistics) and _same(got[d].quantiles, want.quantiles) and str(got[d]) == str(want)
        assert (got[d].start, got[d].end, got[d].thin, got[d].niter, got[d].nchain) == (5, 5 * nr, 5, nr, 2)
        assert got[d].varnames == ["c", "a"] and np.isfinite(got[d].statistics).all()
    assert _same(got.statistics, np.stack([g.statistics for g in got])) and got.per_chain.sd.shape == (10, 2)

    fake.calls.clear()
    ess = S.effective_size(ans)
    assert [(c["N"], c["probs"], c["want_chains"]) for c in fake.calls] == [(7, (), False), (25, (), False), (40, (), False)]
    assert ess.shape == (5, 3) and _same(ess, ans.summary().ess)


def test_a_result_with_one_row_count_takes_one_unmasked_call(monkeypatch):
    import fmcmc_amd as F
    S = importlib.import_module("fmcmc_amd.summary")       # (fmcmc_amd.summary is the function)
    x, ans = _host_batch(None)
    fake = _FakeDevice(x)
    monkeypatch.setattr(S, "enqueue_summary_groups", fake)
    got = F.summary(ans)
    assert [(c["N"], c["mask"]) for c in fake.calls] == [(40, None)] and len(got) == 5 and got[4].end == 200
    assert got[0].probs == S.DEFAULT_QUANTILES and got[0].varnames == ["a", "b", "c"]


def test_non_finite_counts_raise_naming_the_dataset(monkeypatch):
    S = importlib.import_module("fmcmc_amd.summary")       # (fmcmc_amd.summary is the function)
    x, ans = _host_batch(None)
    fake = _FakeDevice(x)

    def counting(*a, **k):
        pooled, chain, work, cols = fake(*a, **k)
        pooled[3, 1 * 5 + 4] = 2.0                       # dataset 3, second column of the call: two non-finite values
        return pooled, chain, work, cols

    monkeypatch.setattr(S, "enqueue_summary_groups", counting)
    with pytest.raises(ValueError, match=r"dataset 3: 2 non-finite value\(s\) among the rows to summarise \(columns \[0\]\)"):
        ans.summary(cols=[1, 0])
    with pytest.raises(ValueError, match="dataset 3: 2 non-finite"):
        ans.effective_size()


def test_refusals_before_any_device_work(monkeypatch):
    import torch.distributed as dist
    import fmcmc_amd as F
    S = importlib.import_module("fmcmc_amd.summary")       # (fmcmc_amd.summary is the function)
    _x, ans = _host_batch(None)
    monkeypatch.setattr(S, "enqueue_summary_groups", lambda *a, **k: pytest.fail("the device was reached"))
    with pytest.raises(ValueError, match="at most 16 quantiles"):
        ans.summary(quantiles=np.linspace(0.0, 1.0, 17))
    with pytest.raises(ValueError, match="at most 16 quantiles"):
        F.summary(ans, quantiles=np.linspace(0.0, 1.0, 17))
    for other in (ans[0], ans.history, [ans], None):
        with pytest.raises(TypeError, match="McmcBatch"):
            S.summary_batch(other)
        with pytest.raises(TypeError, match="McmcBatch"):
            S.effective_size_batch(other)
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    for call in (ans.summary, ans.effective_size, lambda: F.summary(ans), lambda: F.effective_size(ans)):
        with pytest.raises(NotImplementedError, match="more than one rank"):
            call()


def test_the_public_names():
    import inspect
    import fmcmc_amd as F
    for name in ("McmcSummaryBatch", "summary_batch"):
        assert name in F.__all__ and hasattr(F, name)
    assert list(inspect.signature(F.McmcBatch.summary).parameters)[1:] == ["quantiles", "cols"]
    assert list(inspect.signature(F.McmcBatch.effective_size).parameters)[1:] == ["cols"]
    assert list(inspect.signature(F.summary_batch).parameters) == ["ans", "quantiles", "cols"]
