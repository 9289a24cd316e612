"""ess() of an McmcBatch on the GPU (summary.ess_batch on fmcmc_rank_ess_groups_dev): every dataset's EssDiag against ess(ans[d])
in every field to the bit, on a run, on a ragged result, with autoburnin and cols, beyond the grouped limit; and
MCMC_batch(stop_each = convergence_rhat(min_ess = ...)) on ONE grouped ESS call a check instead of one call per dataset."""
import importlib

import numpy as np
import pytest

from test_gpu_batch import linreg_data
from test_gpu_rank_ess import _bits
from test_gpu_rank_groups import hand_built

pytestmark = pytest.mark.gpu

FIELDS = ("bulk", "tail", "tail_q05", "tail_q95", "mean", "mcse_mean", "tau_bulk", "q05", "q95")


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def assert_equals_the_loop(ans, got, **kw):
    import fmcmc_amd as f
    assert isinstance(got, f.EssDiagBatch) and isinstance(got, list) and len(got) == len(ans)
    for d in range(len(ans)):
        one = f.ess(ans[d], **kw)
        for fld in FIELDS:
            assert _same(getattr(got[d], fld), getattr(one, fld)), (d, fld)
            assert _same(getattr(got, fld)[d], getattr(one, fld)), (d, fld)
        assert np.array_equal(got[d].lags, one.lags) and np.array_equal(got.lags[d], one.lags), d
        assert (got[d].nchains, got[d].niter, got[d].start, got[d].end) == (one.nchains, one.niter, one.start, one.end), d
        assert got[d].varnames == one.varnames and str(got[d]) == str(one) and repr(got[d]) == repr(one), d


@pytest.fixture(scope="module")
def run():
    """5 datasets x 3 chains, k = 3 (intercept, slope and sigma), 400 steps"""
    import fmcmc_amd as f
    Xs, ys, base = linreg_data(5, 50, 1, 5)
    batch = f.model_batch(f.gaussian_linreg(Xs[d], ys[d]) for d in range(5))
    rng = np.random.default_rng(61)
    init = np.asarray(base)[None, None, :] + 0.3 * rng.standard_normal((5, 3, len(base)))
    init[:, :, -1] = np.abs(init[:, :, -1]) + 0.5
    ans = f.MCMC_batch(init, batch, 400, nchains=3, seed=62, kernel=f.kernel_normal(scale=0.1))
    return ans, len(base)


def test_ess_of_a_small_batch_run(run):
    import fmcmc_amd as f
    ans, k = run
    assert k == 3
    got = f.ess(ans)
    assert got.bulk.shape == (5, k) and got.lags.shape == (5, k, 4) and np.isfinite(got.bulk).all() and np.isfinite(got.tail).all()
    assert_equals_the_loop(ans, got)
    assert_equals_the_loop(ans, ans.ess(autoburnin=True), autoburnin=True)
    assert_equals_the_loop(ans, f.ess_batch(ans, cols=[2, 0]), cols=[2, 0])
    assert_equals_the_loop(ans, ans.ess(True, [1]), autoburnin=True, cols=[1])


def test_ess_of_a_ragged_batch():
    import fmcmc_amd as f
    D, Cm = 4, 3
    x, _ = __import__("ess_cases").make_inputs(D * Cm, 300, 77, row0=0)
    x = x[:, [0, 1, 3], :301]
    ans = hand_built(x, D, Cm, names=["a", "b", "c"])
    assert_equals_the_loop(ans, f.ess(ans))
    rag = hand_built(x, D, Cm, nrows=[301, 100, 301, 57])
    assert rag.ragged
    got = f.ess(rag)
    assert [r.niter for r in got] == [301, 100, 301, 57] and [r.end for r in got] == [301, 100, 301, 57]
    assert_equals_the_loop(rag, got)
    half = rag.ess(autoburnin=True)
    assert [r.niter for r in half] == [150, 50, 150, 28] and [r.start for r in half] == [152, 51, 152, 30]
    assert_equals_the_loop(rag, half, autoburnin=True)
    short = hand_built(x, D, Cm, nrows=[301, 7, 301, 57])                        # 7 rows: the single form's refusal, named
    with pytest.raises(ValueError, match="dataset 1: .*at least eight"):
        f.ess(short)


def test_a_batch_beyond_the_limit_goes_dataset_by_dataset(monkeypatch):
    """2 datasets x 1 chain: 8194 rows are M = 8194 values, two more than a workgroup sorts; the dataset with 100 rows of the
    ragged form still goes through the grouped call"""
    import fmcmc_amd as f
    from fmcmc_amd import _abi as abi
    summary = importlib.import_module("fmcmc_amd.summary")
    N = abi.lib().fmcmc_rank_groups_max_values() + 2
    x = np.random.default_rng(91).standard_normal((2, 1, N)).round(2)
    assert not summary.rank_groups_fit(1, N)
    ans = hand_built(x, 2, 1)
    assert_equals_the_loop(ans, f.ess(ans))
    calls = []
    grouped = summary.enqueue_rank_ess_groups
    monkeypatch.setattr(summary, "enqueue_rank_ess_groups", lambda *a, **kw: calls.append(a[4]) or grouped(*a, **kw))
    rag = hand_built(x, 2, 1, nrows=[N, 100])
    got = f.ess(rag)
    assert calls == [100]
    monkeypatch.undo()
    assert_equals_the_loop(rag, got)


# ------------------------------------------------------------------------------------------------ stop_each with min_ess
def test_stop_each_with_min_ess_makes_one_grouped_call_a_check(monkeypatch):
    """the run of tests/test_gpu_batch_stop_rhat.py: test_min_ess_holds_a_dataset_back, twice: as it is (the grouped ESS call,
    no enqueue_rank_ess at all) and with rank_groups_fit saying no (dataset by dataset, the path before): the same converged,
    steps, rows and rhat_history to the bit"""
    import fmcmc_amd as F
    from test_gpu_batch_stop_rhat import RhatRef
    from test_gpu_parity import _bits_equal
    summary = importlib.import_module("fmcmc_amd.summary")
    ref = RhatRef(5, 3, 600, 100, with_ess=True)
    t, m = ref.threshold_and_min_ess()
    single_calls, group_calls = [], []
    one, many = summary.enqueue_rank_ess, summary.enqueue_rank_ess_groups
    monkeypatch.setattr(summary, "enqueue_rank_ess", lambda *a, **kw: single_calls.append(1) or one(*a, **kw))
    monkeypatch.setattr(summary, "enqueue_rank_ess_groups", lambda *a, **kw: group_calls.append(kw.get("active", a[-1])) or many(*a, **kw))
    ans = ref.run(F.convergence_rhat(100, threshold=t, min_ess=m))
    stop, _conv = ref.assert_result(ans, t, m)
    assert (stop != ref.stops(t)[0]).any()
    assert single_calls == [] and 1 <= len(group_calls) <= len(ref.bulks)        # at most one a check, none dataset by dataset
    assert all(a is not None and 1 <= int(a.sum()) <= ref.D for a in group_calls)  # masked to the datasets whose R-hat passed
    n_grouped = len(group_calls)
    monkeypatch.setattr(summary, "rank_groups_fit", lambda *a: False)
    loop = ref.run(F.convergence_rhat(100, threshold=t, min_ess=m))
    assert len(group_calls) == n_grouped and len(single_calls) >= n_grouped
    assert loop.converged.tolist() == ans.converged.tolist() and loop.steps.tolist() == ans.steps.tolist()
    assert loop.nrows.tolist() == ans.nrows.tolist() and len(loop.rhat_history) == len(ans.rhat_history)
    for (ta, va), (tb, vb) in zip(ans.rhat_history, loop.rhat_history):
        assert ta == tb and _bits_equal(va, vb)
    assert _bits_equal(loop.history._samples.cpu().numpy(), ans.history._samples.cpu().numpy())
