"""Host self-check of tests/gelman_ref.py, the yardstick of tests/test_gpu_gelman_narrow.py; no GPU.

 * A float64 restatement of the kernel's order of operations (gelman_ref.emulate_work / emulate_partial) lies within the
   a-priori bounds of gelman_ref at every (family, p, N) the GPU module runs, with ratio < 1: the bounds are not too tight for
   correct arithmetic, the inputs are not too hard for it.
 * The float64 numpy definition (np.mean, np.cov) lies OUTSIDE them on data offset by 1e8: numpy cannot judge the kernel
   there, longdouble can.
 * gelman_diag_finish on the longdouble partial agrees with the longdouble restatement of coda::gelman.diag to 1e-10 on the
   end-to-end inputs: the reference sits a decade inside that check's 1e-9.
"""
import numpy as np
import pytest

import gelman_ref as R
from test_abi import abi  # noqa: F401  (the fixture that builds / loads the library)
from test_gelman_diag_host import coda_gelman_ld


def _center(x, cols, row0):
    return x[0, cols, row0].copy()


def _cond_cases():
    for family in R.FAMILIES:
        for i, (p, N) in enumerate((p, N) for p in R.COND_P for N in R.COND_N):
            yield family, p, N, i


def test_the_emulation_lies_within_the_bounds_at_every_shape_edge():
    worst = (0.0, 0.0, 0.0)
    for p, N, i in R.edge_cases():
        x, cols, row0 = R.edge_input(p, N, i)
        ctr = _center(x, cols, row0)
        work = R.emulate_work(x, cols, row0, N, ctr)
        rx, rS = R.work_ratios(work, x, cols, row0, N, ctr)
        rp = R.partial_ratio(R.emulate_partial(work, p), work, p)
        worst = tuple(max(a, b) for a, b in zip(worst, (rx, rS, rp)))
        assert rx < 1 and rS < 1 and rp < 1, (p, N, rx, rS, rp)
    print("shape edges, emulation: worst ratio xbar %.3f, S %.3f, chain sum %.3f" % worst)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_emulation_lies_within_the_bounds_in_every_family(family):
    worst = (0.0, 0.0, 0.0)
    for fam, p, N, i in _cond_cases():
        if fam != family:
            continue
        x, cols, row0 = R.edge_input(p, N, i, Cn=3, family=family)
        ctr = _center(x, cols, row0)
        work = R.emulate_work(x, cols, row0, N, ctr)
        rx, rS = R.work_ratios(work, x, cols, row0, N, ctr)
        rp = R.partial_ratio(R.emulate_partial(work, p), work, p)
        worst = tuple(max(a, b) for a, b in zip(worst, (rx, rS, rp)))
        assert rx < 1 and rS < 1 and rp < 1, (family, p, N, rx, rS, rp)
        if family == "constant":
            j = p // 2
            Sc = work[:, p:].reshape(-1, p, p)
            zero = np.zeros(1).view(np.uint64)[0]
            assert np.all(Sc[:, j, :].view(np.uint64) == zero) and np.all(Sc[:, :, j].copy().view(np.uint64) == zero)
            assert np.array_equal(work[:, j], np.array([R.constant_value(c) for c in range(3)]) - ctr[j])
    print("%s, emulation: worst ratio xbar %.3f, S %.3f, chain sum %.3f" % ((family,) + worst))


def test_the_null_center_and_the_chain_counts_lie_within_the_bounds():
    for p in (5, 20, 40, 64):
        x, cols, row0 = R.edge_input(p, 65, 1)
        work = R.emulate_work(x, cols, row0, 65, None)
        rx, rS = R.work_ratios(work, x, cols, row0, 65, None)
        assert rx < 1 and rS < 1, (p, rx, rS)
    for m, p, N in R.E2E:                                        # the end-to-end shapes
        x, cols, row0 = R.e2e_input(m, p, N)
        work = R.emulate_work(x, cols, row0, N, _center(x, cols, row0))
        rx, rS = R.work_ratios(work, x, cols, row0, N, _center(x, cols, row0))
        assert rx < 1 and rS < 1 and R.partial_ratio(R.emulate_partial(work, p), work, p) < 1, (m, p, N, rx, rS)
    x = R.make_chains(2, 4, 52, 8)                               # the repeated column of the GPU module
    work = R.emulate_work(x, [3, 3, 0], 1, 49, x[0, [3, 3, 0], 1])
    assert max(R.work_ratios(work, x, [3, 3, 0], 1, 49, x[0, [3, 3, 0], 1])) < 1
    for Cn in (1, 2, 3, 4, 5, 8, 9):
        x, cols, row0 = R.edge_input(17, 65, 2, Cn=Cn)
        work = R.emulate_work(x, cols, row0, 65, _center(x, cols, row0))
        rp = R.partial_ratio(R.emulate_partial(work, 17), work, 17)
        print("chains %d, emulation: chain sum ratio %.3f" % (Cn, rp))
        assert rp < 1


def test_float64_numpy_is_outside_the_bounds_on_offset_data():
    """Why longdouble is the yardstick: np.mean / np.cov of the same float64 data miss the bounds the kernel's order keeps.
    The window is laid out as the definition takes it (test_abi.numpy_gelman_partial: a C-contiguous [m][N][p] array, rows =
    iterations), where numpy's column means are plain running sums of N numbers near 1e8.  (On a transposed view of a [p][N]
    array numpy sums pairwise and stays at 0.7 of the bound at these shapes: what numpy is worth depends on the strides.)"""
    worst_np, worst_em = 0.0, 0.0
    for fam, p, N, i in _cond_cases():
        if fam != "offset":
            continue
        x, cols, row0 = R.edge_input(p, N, i, Cn=3, family="offset")
        ctr = _center(x, cols, row0)
        win = np.ascontiguousarray(x[:, cols, row0:row0 + N].transpose(0, 2, 1))
        npw = np.concatenate([win.mean(1) - ctr, np.array([np.cov(c.T, ddof=1).reshape(p * p) for c in win])], axis=1)
        worst_np = max(worst_np, *R.work_ratios(npw, x, cols, row0, N, ctr))
        worst_em = max(worst_em, *R.work_ratios(R.emulate_work(x, cols, row0, N, ctr), x, cols, row0, N, ctr))
    print("offset 1e8: numpy float64 at %.2f of the bound, the emulation at %.3f" % (worst_np, worst_em))
    assert worst_np > 1 and worst_em < 1


@pytest.mark.parametrize("m,p,N", R.E2E)
def test_the_reference_sits_a_decade_inside_the_end_to_end_bound(abi, m, p, N):
    from fmcmc_amd.summary import gelman_diag_finish
    x, cols, row0 = R.e2e_input(m, p, N)
    part = R.longdouble_partial(x, cols, row0, N, _center(x, cols, row0)).astype(np.float64)
    g = gelman_diag_finish(part, p, N)
    est, upper = coda_gelman_ld(x[:, cols, row0:row0 + N].transpose(0, 2, 1))
    err = max(np.abs(g.psrf[:, 0] / est - 1).max(), np.abs(g.psrf[:, 1] / upper - 1).max())
    print("m=%d p=%d N=%d: finish(longdouble partial) within %.2e of coda in longdouble" % (m, p, N, err))
    assert err < 1e-10
    assert (g.mpsrf is None) == (p == 1)
