"""Host-side tests of the rank-normalised split R-hat (no GPU): the C-ABI surface and its refusals, the host restatement
convergence.rhat_host against the definition written out (tests/rhat_cases.py: literal_rhat), the cases whose answer follows from
the definition alone, and the checker convergence_rhat."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import rhat_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fmcmc_rank_work_len", "fmcmc_rank_rhat_out_len", "fmcmc_rank_scores_dev", "fmcmc_rank_rhat_dev")


@pytest.fixture(scope="module")
def L():
    from fmcmc_amd import _abi as abi
    return abi.lib()


def test_new_symbols_declared_exported_and_bound(L):
    import fmcmc_amd as f
    from fmcmc_amd import _abi as abi
    header = open(os.path.join(ROOT, "include", "fmcmc_amd.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in abi.EXPORTS, name
    assert "#define FMCMC_ABI_VERSION 6" in header
    assert L.fmcmc_abi_version() == 6 == abi.ABI_VERSION
    for name in ("rhat", "RhatDiag", "rank_scores", "convergence_rhat", "rhat_host"):
        assert hasattr(f, name) and name in f.__all__, name
    assert hasattr(f.DeviceChains, "rhat") and hasattr(f.DeviceChains, "rank_scores")


def test_lengths(L):
    # M = 2 C floor(N / 2) values in T = ceil(M / 4096) tiles: 1280 + 3 M + 2 ceil(M / 2) + 128 T + 4 ceil(T / 2)
    assert L.fmcmc_rank_work_len(2, 3, 4) == 1280 + 3 * 8 + 2 * 4 + 128 + 4
    assert L.fmcmc_rank_work_len(2, 1, 4) == L.fmcmc_rank_work_len(2, 3, 4)            # the columns share the work
    assert L.fmcmc_rank_work_len(3, 1, 1367) == 1280 + 3 * 4098 + 2 * 2049 + 128 * 2 + 4
    assert L.fmcmc_rank_work_len(2, 3, 3) == 0 and L.fmcmc_rank_work_len(0, 3, 8) == 0
    assert L.fmcmc_rank_work_len(1 << 20, 1, 1 << 13) == 0                               # M = 2^33
    assert L.fmcmc_rank_rhat_out_len(4, 3) == 3 * (8 * 4 + 2)
    assert L.fmcmc_rank_rhat_out_len(0, 3) == 0


def _call(L, entry, nchains=2, k=3, S=100, row0=0, N=100, p=3, fold=0, what=0, null=()):
    """An entry with made-up device addresses: every call here must return before anything touches them."""
    fake = lambda name, addr: None if name in null else C.c_void_p(addr)
    head = (fake("samples", 4096), nchains, k, S, row0, N, fake("cols", 8192), p)
    if entry == "scores":
        return L.fmcmc_rank_scores_dev(*head, fold, what, fake("work", 12288), fake("out", 16384), fake("info", 20480), None)
    return L.fmcmc_rank_rhat_dev(*head, fake("work", 12288), fake("out", 16384), None)


@pytest.mark.parametrize("entry", ["scores", "rhat"])
@pytest.mark.parametrize("kw, code, text", [
    (dict(N=3), "ERR_ARG", "N = 3"),
    (dict(nchains=1 << 20, S=1 << 13, N=1 << 13), "ERR_UNSUPPORTED", "2^32"),
    (dict(nchains=1 << 16, S=1 << 16, N=1 << 16), "ERR_UNSUPPORTED", "2^32"),            # M = 2^32 exactly
    (dict(null=("samples",)), "ERR_ARG", "null"),
    (dict(null=("cols",)), "ERR_ARG", "null"),
    (dict(null=("work",)), "ERR_ARG", "null"),
    (dict(null=("out",)), "ERR_ARG", "null"),
    (dict(row0=1), "ERR_ARG", "[1, 101)"),
    (dict(row0=-1, N=50), "ERR_ARG", "[-1, 49)"),
    (dict(p=4), "ERR_ARG", "outside the k = 3"),
    (dict(p=0), "ERR_ARG", "p = 0"),
    (dict(k=0), "ERR_ARG", "k = 0"),
    (dict(nchains=0), "ERR_ARG", "nchains = 0"),
])
def test_refusals_come_before_any_device_call(L, entry, kw, code, text):
    from fmcmc_amd import _abi as abi
    assert _call(L, entry, **kw) == getattr(abi, code)
    assert text in abi.last_error(), abi.last_error()


@pytest.mark.parametrize("kw, text", [(dict(null=("info",)), "null"), (dict(fold=2), "fold = 2"), (dict(what=-1), "what = -1")])
def test_refusals_of_the_scores_entry(L, kw, text):
    from fmcmc_amd import _abi as abi
    assert _call(L, "scores", **kw) == abi.ERR_ARG
    assert text in abi.last_error(), abi.last_error()


def test_a_column_outside_k_is_refused_by_the_python_layer():
    """cols lives on the device, so the C entries can only refuse more columns than parameters; which column is outside k is
    the Python layer's to say, before anything is enqueued (a stand-in for the chains: nothing here touches a device)."""
    from types import SimpleNamespace
    from fmcmc_amd.summary import _columns
    dc = SimpleNamespace(_samples=np.zeros((2, 3, 10)))
    for cols in ([3], [0, -1], []):
        with pytest.raises(ValueError, match="must name at least one of the 3 parameters"):
            _columns(dc, cols)


# ------------------------------------------------------------------------------------------------ the host restatement
@pytest.mark.parametrize("Cn, N, seed", [(1, 4, 1), (2, 5, 2), (3, 12, 3), (2, 31, 4)])
def test_rhat_host_against_the_definition_written_out(Cn, N, seed):
    from fmcmc_amd import rhat_host
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((Cn, N, 3))
    data[:, :, 1] = np.round(data[:, :, 1], 1)                    # ties
    data[:, :, 2] = data[:, :, 2] ** 3 + np.arange(Cn)[:, None]   # skewed, chains apart
    bulk, tail, rhat, med = rc.literal_rhat(data)
    got = rhat_host(data)
    assert np.array_equal(got.median, med)
    # the two differ in the order of their sums alone: a few units of roundoff of the sums, carried through a square root
    for a, b in ((got.bulk, bulk), (got.tail, tail), (got.rhat, rhat)):
        assert np.allclose(a, b, rtol=64 * rc.U * N, atol=0.0), (a, b)
    assert np.array_equal(got.rhat, np.maximum(got.bulk, got.tail))


def test_rhat_host_takes_an_mcmc_list():
    import fmcmc_amd as f
    data = np.random.default_rng(5).standard_normal((3, 20, 2))
    ml = f.McmcList([f.Mcmc(data[c], start=1, end=20, thin=1) for c in range(3)])
    a, b = f.rhat_host(ml), f.rhat_host(data)
    assert np.array_equal(a.rhat, b.rhat) and np.array_equal(a.median, b.median)
    with pytest.raises(ValueError, match="N >= 4"):
        f.rhat_host(data[:, :3])
    data[1, 7, 1] = np.nan
    with pytest.raises(ValueError, match=r"1 non-finite value\(s\) among the rows to rank \(columns \[1\]\)"):
        f.rhat_host(data)


def test_identical_chains_give_the_within_chain_floor():
    from fmcmc_amd import rhat_host
    x = rc.identical_chains()
    nh = x.shape[1] // 2
    want = float(np.sqrt(np.longdouble(nh - 1) / np.longdouble(nh)))
    got = rhat_host(x)
    assert got.bulk[0] == want and got.tail[0] == want and got.rhat[0] == want


def test_shifted_chains_show_in_the_bulk():
    from fmcmc_amd import rhat_host
    got = rhat_host(rc.shifted_chains())
    # med lies between the two groups, five standard deviations from each: folded, they have one distribution again
    assert got.bulk[0] > 1.5 and got.tail[0] < 1.05
    assert got.rhat[0] == got.bulk[0]


def test_scaled_chains_show_in_the_tail_alone():
    from fmcmc_amd import rhat_host
    got = rhat_host(rc.scaled_chains())
    assert got.bulk[0] < 1.05 and got.tail[0] > 1.2
    assert got.rhat[0] == got.tail[0]


def test_an_odd_window_ignores_its_middle_row():
    from fmcmc_amd import rhat_host
    x = np.random.default_rng(21).standard_normal((3, 41, 2))
    y = x.copy()
    y[:, 20, :] = 1e6 * (1.0 + np.arange(3))[:, None]
    a, b = rhat_host(x), rhat_host(y)
    for name in ("bulk", "tail", "rhat", "median"):
        assert np.array_equal(getattr(a, name).view(np.uint64), getattr(b, name).view(np.uint64)), name


def test_a_constant_column_is_nan_without_a_warning():
    from fmcmc_amd import rhat_host
    x = np.random.default_rng(22).standard_normal((2, 30, 2))
    x[:, :, 1] = 3.25
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = rhat_host(x)
    assert np.isnan(got.bulk[1]) and np.isnan(got.tail[1]) and np.isnan(got.rhat[1]) and got.median[1] == 3.25
    assert np.isfinite(got.rhat[0])


def test_zeros_of_both_signs_tie():
    from fmcmc_amd import rhat_host
    from fmcmc_amd.convergence import rank_z
    _, twice = rank_z(np.array([[-0.0, 0.0, 1.0, -1.0], [0.0, -0.0, 2.0, -0.0]]))
    assert twice.tolist() == [[8.0, 8.0, 14.0, 2.0], [8.0, 8.0, 16.0, 8.0]]           # five zeros share the ranks 2 .. 6
    rng = np.random.default_rng(23)
    x = rng.choice([-1.0, 0.0, 1.0, 2.0], size=(2, 40, 1))
    y = np.where((x == 0.0) & (rng.uniform(size=x.shape) < 0.5), -0.0, x)
    a, b = rhat_host(x), rhat_host(y)
    assert np.array_equal(a.rhat.view(np.uint64), b.rhat.view(np.uint64))


def test_rhat_finish_on_hand_made_moments():
    from fmcmc_amd.summary import rhat_finish
    # one column, C = 1 (two split chains) of N' = 10 rows: bulk means 0 and 1, variances 1 and 3; a constant tail
    out = np.array([0.0, 1.0, 1.0, 3.0, 0.5, 0.0, 0.5, 0.0, 0.0, 7.5])
    fin = rhat_finish(out, 1, 10)
    B, W = 10 * 0.5, 2.0
    assert fin.bulk[0] == np.sqrt((B / W + 9) / 10) and np.isnan(fin.tail[0]) and np.isnan(fin.rhat[0])
    assert fin.median[0] == 7.5 and fin.non_finite[0] == 0.0


def test_rhat_diag_prints_a_table():
    from fmcmc_amd import RhatDiag
    d = RhatDiag([1.001, 1.2], [1.004, np.nan], [0.5, 2.0], 4, 100, ["alpha", "beta"], 1, 100)
    assert np.array_equal(d.rhat[:1], [1.004]) and np.isnan(d.rhat[1])
    text = str(d)
    assert "4 chains of 100 rows" in text and "Bulk" in text and "Tail" in text and "R-hat" in text
    assert "alpha" in text and "beta" in text and "NA" in text
    assert repr(d).startswith("<RhatDiag nvar=2")


# ------------------------------------------------------------------------------------------------ the checker
def test_convergence_rhat_has_the_checkers_duck_type():
    import fmcmc_amd as f
    chk = f.convergence_rhat()
    assert (chk.freq, chk.threshold, chk.autoburnin) == (1000, 1.01, True)
    chk = f.convergence_rhat(freq=250, threshold=1.05, autoburnin=False)
    assert (chk.freq, chk.threshold, chk.autoburnin) == (250, 1.05, False)
    assert chk.history == [] and chk.msg == "" and chk.last is None
    chk.history.append((500, 1.2, np.array([1.2])))
    chk.msg, chk.last = "Rank-normalised split R-hat: %.4f." % 1.2, 1.2
    assert chk.msg == "Rank-normalised split R-hat: 1.2000."
    chk.flush()
    assert chk.history == [] and chk.msg == "" and chk.last is None
    assert callable(chk.check_device) and callable(chk)
    with pytest.raises(TypeError):
        chk(np.zeros((2, 10, 1)))


def test_the_checker_is_short_of_rows_without_a_device():
    """fewer than 4 rows in the window: not converged, nothing enqueued (a stand-in for the chains)."""
    from types import SimpleNamespace
    import fmcmc_amd as f
    chk = f.convergence_rhat(freq=3, autoburnin=False)
    assert chk.check_device(SimpleNamespace(iters=np.arange(1, 4), nrows=3), np.arange(2)) is False
    assert chk.history == [] and chk.msg == ""
