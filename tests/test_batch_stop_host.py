"""MCMC_batch(stop_each = ...), McmcBatch.gelman_diag() and their two C entries (fmcmc_gelman_groups_dev,
fmcmc_mcmc_run_batch_sel_dev), the parts that need no GPU: the symbols, the bulk plan, the refusals that come before any device
work, the argument checks of the grouped reduction and the bookkeeping of a ragged McmcBatch on host tensors."""
import ctypes as C
import inspect

import numpy as np
import pytest

from test_abi import declared_functions
from test_batch_host import _data


@pytest.fixture(scope="module")
def abi():
    from fmcmc_amd import _abi, build
    if build.needs_build():
        build.build()
    _abi.lib()
    return _abi


NEW = ["fmcmc_mcmc_run_batch_sel_dev", "fmcmc_gelman_groups_work_len", "fmcmc_gelman_groups_dev"]


def test_the_new_entries_are_declared_and_exported_under_the_same_abi_version(abi):
    names = declared_functions()
    assert set(NEW) <= set(names)
    assert set(NEW) <= set(abi.EXPORTS)
    L = abi.lib()
    assert all(hasattr(L, n) for n in NEW)
    assert L.fmcmc_abi_version() == 6 and abi.ABI_VERSION == 6
    assert not any(n.endswith("_host") and ("groups" in n or "_sel_" in n) for n in names)    # (no host-pointer variants)


def test_the_work_length_of_the_grouped_reduction(abi):
    L = abi.lib()
    for G, Cm, p in [(1, 2, 1), (6, 5, 5), (256, 4, 64)]:
        assert L.fmcmc_gelman_groups_work_len(G, Cm, p) == L.fmcmc_gelman_work_len(G * Cm, p) == G * Cm * (p + p * p)


@pytest.mark.parametrize("kw,code,substr", [
    (dict(p=65), "ERR_UNSUPPORTED", "FMCMC_MAX_K_WAVE = 64"),
    (dict(G=0), "ERR_ARG", "at least 1"),
    (dict(Cm=0), "ERR_ARG", "at least 1"),
    (dict(N=1), "ERR_ARG", "at least two"),
    (dict(row0=-1), "ERR_ARG", "at least two"),
    (dict(row0=90, N=11), "ERR_ARG", "at least two"),
    (dict(samples=None), "ERR_ARG", "null argument"),
])
def test_the_grouped_reduction_checks_its_arguments_before_any_device_call(abi, kw, code, substr):
    """(the pointers are never followed: every one of these calls is refused first)"""
    a = dict(samples=8, G=3, Cm=2, k=70, S=100, row0=10, N=20, cols=8, p=5, active=None, work=8, partials=8)
    a.update(kw)
    rc = abi.lib().fmcmc_gelman_groups_dev(a["samples"], a["G"], a["Cm"], a["k"], a["S"], a["row0"], a["N"], a["cols"], a["p"],
                                           a["active"], a["work"], a["partials"], None)
    assert rc == getattr(abi, code)
    assert substr in abi.last_error()


def _reference_plan(nsteps, burnin, freq):
    """R/mcmc.R:868-884 written out once more (what oracle.mcmc_with_conv_checker and MCMC_with_conv_checker run)"""
    if freq * 2 > nsteps:
        freq = 0
    if freq > 0:
        bulks = [freq] * ((nsteps - burnin) // freq)
        if (nsteps - burnin) % freq:
            bulks.append((nsteps - burnin) - sum(bulks))
    else:
        bulks = [nsteps]
    bulks[0] += burnin
    return bulks


@pytest.mark.parametrize("nsteps,burnin,freq,thin,expect", [
    (600, 0, 100, 1, [100] * 6),
    (650, 0, 100, 1, [100] * 6 + [50]),              # a remainder bulk
    (650, 30, 100, 3, [130] + [100] * 5 + [20]),      # burnin goes to the first bulk, the remainder is of nsteps - burnin
    (150, 0, 100, 1, [150]),                          # 2 freq > nsteps: one bulk
    (100, 7, 20, 25, [27, 20, 20, 20, 13]),           # freq < thin < freq + burnin: the first bulk keeps no row
])
def test_the_bulk_plan_is_that_of_mcmc_with_conv_checker(nsteps, burnin, freq, thin, expect):
    import fmcmc_amd as F
    from fmcmc_amd import engine
    from fmcmc_amd import mcmc
    plan = F.bulk_plan(nsteps, burnin, freq)
    assert plan == expect == _reference_plan(nsteps, burnin, freq)
    assert "bulk_plan(nsteps, burnin, freq)" in inspect.getsource(mcmc.MCMC_with_conv_checker)   # (one plan for both loops)
    rows = [engine.kept_rows(nb, burnin if bi == 0 else 0, thin) for bi, nb in enumerate(plan)]
    if (nsteps, thin) == (100, 25):
        assert rows[0] == 0


def test_stop_each_refusals_before_any_device_work():
    import fmcmc_amd as F
    b = F.model_batch(F.gaussian_linreg(X, y) for X, y in _data())
    with pytest.raises(ValueError, match="conv_checker"):
        F.MCMC_batch(np.zeros(4), b, 100, nchains=2, conv_checker=F.convergence_gelman(50))
    with pytest.raises(ValueError, match="conv_checker.*stop_each"):
        F.MCMC_batch(np.zeros(4), b, 100, nchains=2, conv_checker=F.convergence_gelman(50), stop_each=F.convergence_gelman(50))
    for other in (F.convergence_geweke(50), F.convergence_auto(50), object(), 50):
        with pytest.raises(TypeError, match="stop_each"):
            F.MCMC_batch(np.zeros(4), b, 100, nchains=2, stop_each=other)
    with pytest.raises(ValueError, match="Convergence test with the Gelman is only available when `nchains` > 1L."):
        F.MCMC_batch(np.zeros(4), b, 100, nchains=1, stop_each=F.convergence_gelman(50))
    with pytest.raises(TypeError, match="model_batch"):
        F.MCMC_batch(np.zeros(4), F.gaussian_linreg(*_data()[0]), 100, nchains=2, stop_each=F.convergence_gelman(50))
    with pytest.raises(ValueError, match="-burnin-"):
        F.MCMC_batch(np.zeros(4), b, 100, nchains=2, burnin=100, stop_each=F.convergence_gelman(50))


def _ragged(D=3, Cm=2, k=4, cap=6, nrows=(6, 2, 4), steps=(60, 20, 40), thin=10):
    import torch
    import fmcmc_amd as F
    s = torch.arange(D * Cm * k * cap, dtype=torch.float64).reshape(D * Cm, k, cap)
    lp = torch.arange(D * Cm * cap, dtype=torch.float64).reshape(D * Cm, cap)
    dc = F.DeviceChains(s, lp, None, thin * np.arange(1, cap + 1), thin, ["a", "b", "c", "d"], 0, D * Cm)
    dc.accept_count = torch.arange(D * Cm, dtype=torch.int64)
    hist = [(20, np.array([1.5, 1.1, 1.4])), (40, np.array([1.3, np.nan, 1.1])), (60, np.array([1.25, np.nan, np.nan]))]
    return s, lp, F.McmcBatch(dc, D, Cm, nrows=nrows, steps=steps, converged=[False, True, True], rhat_history=hist)


def test_a_ragged_result_gives_every_dataset_its_own_rows_and_labels():
    import torch
    import fmcmc_amd as F
    s, lp, ans = _ragged()
    assert ans.ragged and len(ans) == 3
    assert ans.nrows.tolist() == [6, 2, 4] and ans.steps.tolist() == [60, 20, 40] and ans.converged.tolist() == [False, True, True]
    assert [t for t, _ in ans.rhat_history] == [20, 40, 60] and np.isnan(ans.rhat_history[2][1][1])
    for d, nr in enumerate((6, 2, 4)):
        dc = ans[d]
        assert isinstance(dc, F.DeviceChains) and dc.nrows == nr and dc.chain_base == 2 * d and dc.nchains_total == 2
        assert tuple(dc.samples.shape) == (2, 4, nr) and tuple(dc.logpost.shape) == (2, nr) and dc.draws is None
        assert dc.iters.tolist() == [10 * (i + 1) for i in range(nr)]
        assert dc.samples.data_ptr() == s[2 * d:].data_ptr() and dc.capacity == 6       # slices of the call's buffers
        assert torch.equal(dc.samples, s[2 * d:2 * d + 2, :, :nr]) and torch.equal(dc.accept_count, torch.arange(2 * d, 2 * d + 2))
    # ans.chains: the rows every dataset has; ans.history: all of them
    assert ans.chains.nrows == 2 and tuple(ans.chains.samples.shape) == (6, 4, 2) and ans.chains.iters.tolist() == [10, 20]
    assert ans.history.nrows == 6
    assert torch.equal(ans.last_rows(), torch.stack([s[c, :, (5, 5, 1, 1, 3, 3)[c]] for c in range(6)]))
    host = ans.to_host()
    assert [h[0].data.shape for h in host] == [(6, 4), (2, 4), (4, 4)] and all(len(h) == 2 for h in host)
    assert host[2][1].mcpar == (10, 40, 10) and (host[2][1].data == s[5, :, :4].numpy().T).all()
    assert ans[-1].nrows == 4
    with pytest.raises(IndexError):
        ans[3]


def test_a_ragged_result_cannot_be_continued_and_says_why():
    from fmcmc_amd.mcmc import batch_initial
    import fmcmc_amd as F
    _s, _lp, ans = _ragged()
    with pytest.raises(ValueError, match="ragged.*step base"):
        batch_initial(ans, 3, 2)
    b = F.model_batch(F.gaussian_linreg(X, y) for X, y in _data())
    with pytest.raises(ValueError, match="ragged"):
        F.MCMC_batch(ans, b, 100, nchains=2)
    with pytest.raises(ValueError, match="at most the 6"):
        _ragged(nrows=(7, 2, 4))


def test_a_result_in_which_every_dataset_ran_every_bulk_continues_as_before():
    import torch
    from fmcmc_amd.mcmc import batch_initial
    s, _lp, ans = _ragged(nrows=(6, 6, 6), steps=(60, 60, 60))
    assert not ans.ragged and ans.chains is ans.history
    a, names = batch_initial(ans, 3, 2)
    assert torch.equal(a, s[:, :, -1]) and names == ["a", "b", "c", "d"]


def test_a_result_without_stop_each_is_the_result_of_before():
    import torch
    import fmcmc_amd as F
    D, Cm, k, S = 2, 3, 4, 5
    s = torch.arange(D * Cm * k * S, dtype=torch.float64).reshape(D * Cm, k, S)
    dc = F.DeviceChains(s, None, None, np.arange(1, S + 1), 1, None, 0, D * Cm)
    dc.accept_count = torch.zeros(D * Cm, dtype=torch.int64)
    ans = F.McmcBatch(dc, D, Cm)
    assert ans.chains is dc and not ans.ragged and ans.converged is None and ans.rhat_history == []
    assert ans.nrows.tolist() == [S, S] and torch.equal(ans.last_rows(), s[:, :, -1])
    assert ans[1].iters.tolist() == [1, 2, 3, 4, 5] and ans[1].nrows == S


def test_the_gelman_diag_of_a_batch_needs_two_chains_per_dataset():
    import torch
    import fmcmc_amd as F
    s = torch.zeros((3, 2, 8), dtype=torch.float64)
    ans = F.McmcBatch(F.DeviceChains(s, None, None, np.arange(1, 9), 1, None, 0, 3), 3, 1)
    for call in (ans.gelman_diag, lambda: F.gelman_diag(ans)):
        with pytest.raises(ValueError, match="only available when `nchains` > 1L"):
            call()
    sig = inspect.signature(F.McmcBatch.gelman_diag)
    assert list(sig.parameters)[1:] == ["confidence", "autoburnin", "multivariate", "cols"]
