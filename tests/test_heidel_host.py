"""Host tests (no GPU) of the Heidelberger-Welch diagnostic's host finish (fmcmc_amd/summary.py: pcramer, heidel_candidates,
heidel_finish) against the single-chain restatement of coda::heidel.diag (fmcmc_amd/convergence.py: heidel_diag, _pcramer).

The finish is fed what the device would hand it -- per window {n, mean, spec0}, per candidate Q -- computed here with numpy in
float64 the way heidel_diag computes them, so any difference is the finish's own.  tests/test_gpu_heidel.py uploads the same
synthetic series (`synthetic_set`)."""
import numpy as np
import pytest

from test_gpu_summary import ar1


# ------------------------------------------------------------------------------------------------ inputs
def synthetic_set(N, thin, start, seed, shift_sd=1.5, shift_frac=0.15):
    """[N][10] columns: four stationary AR(1) (phi 0 .. 0.9, mean 3), two with a level shift of `shift_sd` sd over their first
    `shift_frac` of the rows, two with a linear drift, one with mean near zero, one constant; and the iteration labels."""
    rng = np.random.default_rng(seed)
    cols = [ar1(phi, N, rng, mu=3.0) for phi in (0.0, 0.3, 0.6, 0.9)]
    for phi in (0.0, 0.5):
        y = ar1(phi, N, rng, mu=3.0)
        y[:int(shift_frac * N)] += shift_sd * y.std()
        cols.append(y)
    for slope in (4.0, -8.0):
        cols.append(ar1(0.2, N, rng, mu=3.0) + slope * np.arange(N) / N)
    cols.append(ar1(0.4, N, rng, mu=0.0))
    cols.append(np.full(N, 2.5))
    return np.stack(cols, axis=1), start + thin * np.arange(N, dtype=np.int64)


# (N, thin, first label, seed, shift in sd).  The shifts are small on purpose: coda's four-term series for pcramer is made for
# moderate arguments and falls back towards 0 for large ones, so a shift of 6 sd drives the statistic I out of its range and
# the test "passes" at the first candidate (seen with heidel_diag: 4 sd at N = 600, 2 sd at N = 2000 already do).  Shifts of
# 1.5 sd (N = 600) and 1 sd (N = 2000) keep I where the series holds: the first candidates fail, a later one passes.
# N = 2003 and N = 607 at thin = 3: niter / 10 is off the thinning grid, so the candidate labels (201.3, 91.7, ...) are not
# iterations of the chain and `start` must be the label of the first row kept (202, 94, ...), as heidel_diag and coda report.
CASES = [(600, 3, 31, 1), (600, 3, 31, 2), (2000, 1, 1, 3, 1.0), (2000, 1, 1, 4, 1.0), (2003, 1, 1, 5, 1.0), (607, 3, 31, 6)]


def windows_of(iters):
    """The windows heidel_diag takes, restated from it (nothing of fmcmc_amd.summary): candidate labels, the first row each
    keeps, the first row of the S0 window."""
    from fmcmc_amd.convergence import _window_rows
    iters = np.asarray(iters, dtype=np.float64)
    labels = np.arange(iters[0], iters[-1] / 2 + 1e-9, iters.size / 10.0)
    return labels, np.array([_window_rows(iters, st)[0] for st in labels]), _window_rows(iters, iters[-1] / 2)[0]


def numpy_windows(data, iters):
    """What fmcmc_heidel_dev returns for one chain `data` [N][p], with numpy in float64 as heidel_diag computes it:
    n [ncand], mean / spec0 / Q [ncand][1][p], S0 [1][p], the label of the first row of every tail."""
    from fmcmc_amd.convergence import spectrum0_ar
    labels, rows, half = windows_of(iters)
    p = data.shape[1]
    mean, spec0, Q = (np.empty((rows.size, 1, p)) for _ in range(3))
    for s, lo in enumerate(rows):
        for j in range(p):
            Y = data[lo:, j]
            ybar = Y.mean()
            B = np.cumsum(Y) - ybar * np.arange(1, Y.size + 1)
            mean[s, 0, j], spec0[s, 0, j], Q[s, 0, j] = ybar, spectrum0_ar(Y)[0], np.sum(B * B)
    S0 = np.array([[spectrum0_ar(data[half:, j])[0] for j in range(p)]])
    return data.shape[0] - rows, mean, spec0, Q, S0, np.asarray(iters, dtype=np.float64)[rows]


# ------------------------------------------------------------------------------------------------ tests
def test_vectorised_pcramer_equals_the_scalar_one():
    from fmcmc_amd.convergence import _pcramer
    from fmcmc_amd.summary import pcramer
    q = np.concatenate([np.logspace(-3, 1, 401), np.linspace(0.05, 2.0, 200)])              # 601 values
    got = np.append(pcramer(q[:600].reshape(3, 200)).ravel(), pcramer(q[600]))
    want = np.array([_pcramer(v) for v in q])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert 0.94 < pcramer(0.461) < 0.96 and pcramer(1e-3) == 0.0          # the 5 % point of the statistic is 0.461
    assert np.isnan(pcramer(np.nan))


def test_host_finish_reproduces_heidel_diag():
    from fmcmc_amd.convergence import heidel_diag
    from fmcmc_amd.summary import heidel_finish
    first = later = never = nseries = 0
    for case in CASES:
        data, iters = synthetic_set(*case)
        want = heidel_diag(data, iters)
        n, mean, spec0, Q, S0, starts = numpy_windows(data, iters)
        labels = windows_of(iters)[0]
        hd = heidel_finish(n, mean, spec0, Q, S0, starts, candidates=labels)
        got = hd.table[0]
        assert hd.table.shape == (1, data.shape[1], 6) and hd.cvm.shape == (1, data.shape[1], labels.size)
        assert np.array_equal(hd.candidates, labels) and labels[0] == iters[0]
        for col in (0, 1, 3):                                              # stest, start, htest: equal, NaN where NA
            assert np.array_equal(got[:, col], want[:, col], equal_nan=True), (case, col, got[:, col], want[:, col])
        for col in (2, 4, 5):                                              # pvalue, mean, halfwidth
            assert np.array_equal(np.isnan(got[:, col]), np.isnan(want[:, col])), (case, col)
            np.testing.assert_allclose(got[:, col], want[:, col], rtol=1e-12, atol=0.0, equal_nan=True)
        for name, col in zip(hd.columns, range(6)):
            assert np.array_equal(getattr(hd, name), hd.table[:, :, col], equal_nan=True)
        # the inputs do what they were built for
        assert np.all(got[:4, 0] == 1) and np.all(got[4:6, 1] > iters[0]), (case, got)
        assert got[8, 0] == 1 and got[8, 3] == 0, (case, got[8])           # mean near zero: stationary, half-width test fails
        assert got[9, 0] == 0 and np.all(np.isnan(got[9, 1:])), got[9]    # constant: S0 = 0 -> (0, NA, NA, NA, NA, NA)
        first += int(np.sum(got[:, 1] == iters[0]))
        later += int(np.sum(got[:, 1] > iters[0]))
        never += int(np.sum((got[:, 0] == 0) & np.isfinite(got[:, 2])))
        nseries += data.shape[1]
    print("\n%d series: %d start at the first candidate, %d later, %d never" % (nseries, first, later, never))
    assert nseries == 60 and first >= 12 and later >= 12 and never >= 6


def test_outcomes_of_the_reference_alone():
    """Precondition of the comparison above, from heidel_diag alone: all three outcomes occur in the inputs."""
    from fmcmc_amd.convergence import heidel_diag
    data, iters = synthetic_set(*CASES[0])
    want = heidel_diag(data, iters)
    assert np.any(want[:, 1] == iters[0]) and np.any(want[:, 1] > iters[0])
    assert np.any((want[:, 0] == 0) & np.isfinite(want[:, 2]))
    assert set(want[4:6, 1]) <= set(31.0 + 60.0 * np.arange(1, 15))      # the shifted columns start at a later candidate


def test_start_is_an_iteration_of_the_chain():
    """Off the thinning grid the candidate label is not an iteration: heidel_diag reports the first row kept, so does the finish."""
    from fmcmc_amd.convergence import heidel_diag
    from fmcmc_amd.summary import heidel_finish
    seen = 0
    for case in CASES[4:]:
        data, iters = synthetic_set(*case)
        want = heidel_diag(data, iters)
        got = heidel_finish(*numpy_windows(data, iters)).table[0]
        assert np.array_equal(got[:, 1], want[:, 1], equal_nan=True), (case, got[:, 1], want[:, 1])
        late = got[np.isfinite(got[:, 1]) & (got[:, 1] > iters[0]), 1]
        assert np.all(np.isin(late, iters)) and not np.any(np.isin(late, windows_of(iters)[0])), (case, late)
        seen += late.size
    assert seen >= 4


def test_candidates_and_the_empty_sequence():
    from fmcmc_amd.summary import heidel_candidates
    for iters in (31 + 3 * np.arange(600), 31 + 3 * np.arange(607), np.arange(1, 2004), np.arange(1, 5), 7 + 2 * np.arange(55)):
        for a, b in zip(heidel_candidates(iters), windows_of(iters)):
            assert np.array_equal(a, b), iters.size
    labels, rows, half = heidel_candidates(31 + 3 * np.arange(600))
    assert np.array_equal(labels, 31.0 + 60.0 * np.arange(labels.size)) and labels[-1] <= 1828 / 2 < labels[-1] + 60
    assert np.array_equal(rows, 20 * np.arange(labels.size)) and half == 295            # label 916 is the first >= 914
    labels, rows, half = heidel_candidates(np.arange(1, 5))                             # N = 4: steps of 0.4 iterations
    assert np.array_equal(rows, [0, 1, 1]) and half == 1
    with pytest.raises(ValueError, match="wrong sign in 'by' argument"):
        heidel_candidates(5001 + np.arange(1000))                                       # start > end / 2


def test_printed_layout():
    from fmcmc_amd.summary import heidel_finish
    data, iters = synthetic_set(*CASES[0])
    text = str(heidel_finish(*numpy_windows(data, iters), varnames=["v%d" % j for j in range(10)]))
    lines = text.split("\n")
    assert lines[1].split() == ["Stationarity", "start", "p-value"] and lines[2].split() == ["test", "iteration"]
    assert lines[3].split()[:3] == ["v0", "passed", "31"] and lines[12].split() == ["v9", "failed", "NA", "NA"]
    assert lines[14].split() == ["Halfwidth", "Mean", "Halfwidth"] and lines[25].split() == ["v9", "NA", "NA", "NA"]


def test_exports():
    import fmcmc_amd
    from fmcmc_amd import _abi as abi
    from test_abi import declared_functions
    for name in ("fmcmc_heidel_work_len", "fmcmc_heidel_out_len", "fmcmc_heidel_dev"):
        assert name in abi.EXPORTS and name in declared_functions(), name
    for name in ("heidel", "HeidelDiag"):
        assert name in fmcmc_amd.__all__ and hasattr(fmcmc_amd, name)
    assert hasattr(fmcmc_amd.DeviceChains, "heidel") and abi.ABI_VERSION == 6


def test_argument_errors_come_before_any_device_call():
    import ctypes as C
    from fmcmc_amd import _abi as abi
    L = abi.lib()

    def call(N, half, cand, nchains=2, p=3, S=100):
        cand = np.asarray(cand, dtype=np.int64)
        rc = L.fmcmc_heidel_dev(1, nchains, 3, S, 0, N, 1, p, half, cand.ctypes.data_as(C.POINTER(C.c_int64)), cand.size, 1, 1, None)
        return rc, abi.last_error()

    for args, text in (((50, 25, [0, 5, 3]), "must ascend"), ((50, 25, [0, 5, 48]), "needs 3"), ((50, 48, [0, 5]), "needs 3"),
                       ((50, 4, [5, 10]), "before cand_rows"), ((101, 50, [0]), "outside"), ((2, 0, [0]), "shorter than 3")):
        rc, msg = call(*args)
        assert rc == abi.ERR_ARG and text in msg, (args, rc, msg)
    rc, msg = call(50, 25, [0, 5], nchains=2 ** 40, p=3)
    assert rc == abi.ERR_UNSUPPORTED and "exceed" in msg
    assert L.fmcmc_heidel_work_len(2, 3, 5) == 2 * 3 * 72 and L.fmcmc_heidel_out_len(2, 3, 5) == 6 * 2 * 3 * 4 + 5 * 2 * 3
    assert L.fmcmc_heidel_work_len(2 ** 40, 3, 5) == 0 and L.fmcmc_heidel_out_len(2 ** 40, 3, 5) == 0
