"""The grouped rank-normalised split R-hat (fmcmc_rank_rhat_groups_dev, csrc/diag_rank_groups.hpp), rhat() of an McmcBatch and
MCMC_batch(stop_each = convergence_rhat(...)), the parts that need no GPU: the symbols, the lengths, the refusals that come before
any device work, the pure-numpy finish and verdict, the stacking of RhatDiagBatch and what stop_each accepts."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fmcmc_rank_groups_max_values", "fmcmc_rank_rhat_groups_work_len", "fmcmc_rank_rhat_groups_dev")


@pytest.fixture(scope="module")
def abi():
    from fmcmc_amd import _abi, build
    if build.needs_build():
        build.build()
    _abi.lib()
    return _abi


def test_the_new_entries_are_declared_exported_and_bound(abi):
    import fmcmc_amd as f
    header = open(os.path.join(ROOT, "include", "fmcmc_amd.h")).read()
    L = abi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in abi.EXPORTS, name
    assert "#define FMCMC_ABI_VERSION 6" in header and L.fmcmc_abi_version() == 6 == abi.ABI_VERSION
    for name in ("rhat_batch", "RhatDiagBatch"):
        assert hasattr(f, name) and name in f.__all__, name


def test_the_limit_and_the_work_length(abi):
    L = abi.lib()
    top = L.fmcmc_rank_groups_max_values()
    assert top >= 8192 and top % 2 == 0
    for good in [(1, 1, 1, 4), (256, 4, 4, 2000), (300, 1, 2, 8), (2, 2, top // 2, top // 2), (1, 1, 1, top + 1)]:
        assert L.fmcmc_rank_rhat_groups_work_len(*good) > 0, good
    for bad in [(0, 4, 4, 100), (4, 0, 4, 100), (4, 4, 0, 100), (4, 4, 4, 3), (-1, 4, 4, 100), (4, -2, 4, 100),
                (1, 1, 1, top + 2), (1, top // 2 + 1, 1, 4), (1, 1 << 40, 1, 4), (1 << 31, 1, 1, 4), (1 << 30, 1, 4, 4)]:
        assert L.fmcmc_rank_rhat_groups_work_len(*bad) == 0, bad


@pytest.mark.parametrize("kw, code, text", [
    (dict(samples=None), "ERR_ARG", "null argument"),
    (dict(cols=None), "ERR_ARG", "null argument"),
    (dict(work=None), "ERR_ARG", "null argument"),
    (dict(out=None), "ERR_ARG", "null argument"),
    (dict(G=0), "ERR_ARG", "at least 1"),
    (dict(Cm=0), "ERR_ARG", "at least 1"),
    (dict(Cm=-3), "ERR_ARG", "at least 1"),
    (dict(p=4), "ERR_ARG", "outside the k = 3"),
    (dict(p=0), "ERR_ARG", "p = 0"),
    (dict(k=0), "ERR_ARG", "k = 0"),
    (dict(N=3), "ERR_ARG", "N = 3"),
    (dict(row0=1), "ERR_ARG", "[1, 101)"),
    (dict(row0=-1, N=50), "ERR_ARG", "[-1, 49)"),
    (dict(N=101), "ERR_ARG", "outside the 100 rows"),
    (dict(Cm=2, S=5000, N=4098), "ERR_UNSUPPORTED", "fmcmc_rank_rhat_dev per group"),     # M = 8196
    (dict(Cm=4100, N=4), "ERR_UNSUPPORTED", "fmcmc_rank_rhat_dev per group"),
    (dict(Cm=1 << 20, S=1 << 13, N=1 << 13), "ERR_UNSUPPORTED", "2^32"),
    (dict(G=1 << 31, p=1), "ERR_UNSUPPORTED", "exceed one launch"),
])
def test_refusals_come_before_any_device_call(abi, kw, code, text):
    """(the device addresses are made up and never followed: every one of these calls is refused first)"""
    a = dict(samples=4096, G=3, Cm=2, k=3, S=100, row0=0, N=100, cols=8192, p=3, active=None, work=12288, scores=None, out=16384)
    a.update(kw)
    ptr = lambda v: None if v is None else C.c_void_p(v)
    rc = abi.lib().fmcmc_rank_rhat_groups_dev(ptr(a["samples"]), a["G"], a["Cm"], a["k"], a["S"], a["row0"], a["N"], ptr(a["cols"]),
                                              a["p"], ptr(a["active"]), ptr(a["work"]), ptr(a["scores"]), ptr(a["out"]), None)
    assert rc == getattr(abi, code), abi.last_error()
    assert text in abi.last_error() and "fmcmc_rank_rhat_groups_dev" in abi.last_error(), abi.last_error()


def test_the_limit_is_the_one_the_python_layer_asks_about(abi):
    from fmcmc_amd.summary import rank_groups_fit
    top = abi.lib().fmcmc_rank_groups_max_values()
    assert rank_groups_fit(4, 2000) and rank_groups_fit(1, top) and rank_groups_fit(1, top + 1) and not rank_groups_fit(1, top + 2)
    assert rank_groups_fit(top // 2, 2) and not rank_groups_fit(top // 2 + 1, 2)


# ------------------------------------------------------------------------------------------------------- the host finish
def _synthetic_out(D, p, Cm, seed):
    rng = np.random.default_rng(seed)
    m = 2 * Cm
    out = np.empty((D, p, 4 * m + 2))
    out[:, :, :4 * m] = rng.standard_normal((D, p, 2, m, 2)).reshape(D, p, 4 * m)
    out[:, :, 1:4 * m:2] = np.abs(out[:, :, 1:4 * m:2]) + 0.5        # the variances
    out[:, :, 4 * m] = 0.0
    out[:, :, 4 * m + 1] = rng.standard_normal((D, p))
    out[1, 0, 2 * m + 1:4 * m:2] = 0.0                                # a constant tail: NaN
    out[2, 1, 4 * m] = 3.0                                            # a non-finite count
    return out


def test_the_finish_of_the_grouped_call_is_rhat_finish_per_row():
    from fmcmc_amd.summary import rhat_finish, rhat_groups_finish
    D, p, Cm, nh = 4, 3, 3, 17
    out = _synthetic_out(D, p, Cm, 5)
    fin = rhat_groups_finish(out, Cm, nh)
    for d in range(D):
        one = rhat_finish(out[d], Cm, nh)
        for f in ("bulk", "tail", "rhat", "median", "non_finite"):
            a, b = getattr(fin, f)[d], getattr(one, f)
            assert a.shape == (p,) and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (d, f)
    assert np.isnan(fin.tail[1, 0]) and np.isnan(fin.rhat[1, 0]) and np.isfinite(fin.bulk[1, 0]) and fin.non_finite[2, 1] == 3.0


def test_rhat_diag_batch_stacks_its_elements():
    from fmcmc_amd import RhatDiag, RhatDiagBatch
    ds = [RhatDiag([1.0 + d, 1.2], [1.1, np.nan if d == 1 else 1.3], [0.5, d], 3, 100 + d, ["a", "b"], 1, 100 + d) for d in range(3)]
    b = RhatDiagBatch(ds)
    assert isinstance(b, list) and len(b) == 3 and b[2] is ds[2]
    for f in ("bulk", "tail", "rhat", "median"):
        got = getattr(b, f)
        assert got.shape == (3, 2)
        for d in range(3):
            assert np.array_equal(got[d].view(np.uint64), getattr(ds[d], f).view(np.uint64)), (f, d)
    assert np.isnan(b.rhat[1, 1]) and b.rhat[2, 0] == 3.0 and repr(b) == "<RhatDiagBatch ndatasets=3 nvar=2>"
    empty = RhatDiagBatch([])
    assert len(empty) == 0 and empty.bulk.shape[0] == 0


# ------------------------------------------------------------------------------------------------------- the verdict
def test_the_verdict_per_dataset_on_hand_made_values():
    from fmcmc_amd.summary import rhat_batch_verdicts
    t = 1.01
    r = np.array([[1.001, 1.009],                  # passes
                  [1.001, 1.01],                   # at the threshold: not below it
                  [1.0, np.nan],                   # a constant column
                  [np.nan, np.nan],
                  [1.5, 1.0],
                  [1.0, np.nextafter(1.01, 0.0)]])  # the last double below the threshold
    vals, passed = rhat_batch_verdicts(r, t)
    assert vals[[0, 1, 4]].tolist() == [1.009, 1.01, 1.5] and np.isnan(vals[[2, 3]]).all() and vals[5] == np.nextafter(1.01, 0.0)
    assert passed.tolist() == [True, False, False, False, False, True] and passed.dtype == bool
    # masked datasets: not tested, NaN, never pass -- whatever their row holds
    tested = np.array([True, True, True, False, True, False])
    vals, passed = rhat_batch_verdicts(r, t, tested)
    assert np.isnan(vals[[2, 3, 5]]).all() and vals[[0, 1, 4]].tolist() == [1.009, 1.01, 1.5]
    assert passed.tolist() == [True, False, False, False, False, False]
    vals, passed = rhat_batch_verdicts(r, t, np.zeros(6, dtype=bool))
    assert np.isnan(vals).all() and not passed.any()
    # the verdict of convergence_rhat.check_device on the same rows
    for d in range(6):
        val = float("nan") if np.isnan(r[d]).any() else float(r[d].max())
        v1, p1 = rhat_batch_verdicts(r[d:d + 1], t)
        assert bool(val < t) == bool(p1[0]) and (np.isnan(val) if np.isnan(v1[0]) else val == v1[0])


# ------------------------------------------------------------------------------------------------------- stop_each
def test_stop_each_takes_the_two_grouped_checkers_and_no_other():
    """the check of stop_each comes before the batch is looked at: a convergence_rhat gets as far as the refusal of a batch that
    is none, every other checker is refused first -- and all of it before any device work"""
    import fmcmc_amd as f
    for nchains in (1, 3):
        for chk in (f.convergence_rhat(100), f.convergence_rhat(100, 1.05, False, min_ess=50.0)):
            with pytest.raises(TypeError, match="-batch- must be a model_batch"):
                f.MCMC_batch(np.zeros(3), None, 100, nchains=nchains, stop_each=chk)
            assert chk.history == [] and chk.last is None
    with pytest.raises(TypeError, match="-batch- must be a model_batch"):
        f.MCMC_batch(np.zeros(3), None, 100, nchains=2, stop_each=f.convergence_gelman(100))
    with pytest.raises(ValueError, match="only available when `nchains` > 1L"):
        f.MCMC_batch(np.zeros(3), None, 100, nchains=1, stop_each=f.convergence_gelman(100))
    for other in (f.convergence_geweke(100), f.convergence_auto(100), f.convergence_heildel(100), object(), "rhat", 1.01):
        with pytest.raises(TypeError, match=r"convergence_gelman\(.*or a\s+convergence_rhat\("):
            f.MCMC_batch(np.zeros(3), None, 100, nchains=2, stop_each=other)


def test_the_signatures():
    import fmcmc_amd as f
    from fmcmc_amd.summary import enqueue_rank_rhat_groups
    sig = inspect.signature(f.McmcBatch.rhat)
    assert list(sig.parameters) == ["self", "autoburnin", "cols"]
    assert sig.parameters["autoburnin"].default is False and sig.parameters["cols"].default is None
    sig = inspect.signature(f.rhat_batch)
    assert list(sig.parameters) == ["ans", "autoburnin", "cols"] and sig.parameters["autoburnin"].default is False
    sig = inspect.signature(enqueue_rank_rhat_groups)
    assert list(sig.parameters) == ["dc", "ngroups", "chains_per_group", "row0", "N", "cols", "active", "want_scores"]
    assert sig.parameters["active"].default is None and sig.parameters["want_scores"].default is False
    with pytest.raises(TypeError, match="expects an McmcBatch"):
        f.rhat_batch(np.zeros((2, 10, 1)))
