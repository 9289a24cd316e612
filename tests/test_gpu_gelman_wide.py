"""GPU tests of the Gelman-Rubin window reduction above 64 columns (csrc/gelman.hip: gelman_cov_mfma, one workgroup per chain
and pair of 64-column super-blocks), of convergence_gelman on it and of gelman_diag().

Yardsticks:
 * the partial vector against its numpy definition (test_abi.numpy_gelman_partial) within the project's own tolerance of
   test_gelman_partial_kernel_wide: rtol 1e-9, atol 1e-11 max|ref|.  A float64 emulation of the kernel's arithmetic (shift by the
   first row, one pass, four row quarters) sits at 1.4e-4 of that tolerance at these shapes, as numpy does against longdouble;
 * `work` against longdouble and the partial against its definition from the device's `work`, within the a-priori bounds of
   tests/gelman_ref.py (derived from the kernel's order of operations, proven sane by tests/test_gelman_narrow_host.py);
 * psrf / mpsrf of fmcmc_gelman_finish on the device partial against the oracle's coda restatement, rtol 1e-9 as in
   tests/test_k256_host.py;
 * equalities that need no tolerance: placement in the launch, repetition, symmetry, what a call leaves of NaN-filled buffers;
 * p <= 64 against the bits the library of the commit before p > 64 produced (tests/golden/gelman_narrow_bits.json), and every
   width against the bits of the commit before the two kernels became one (tests/golden/gelman_bits.json); tests/golden/make_gelman_bits.py wrote both.
Every buffer is filled with NaN before a call and carries GUARD more elements than documented, which must stay NaN.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from gelman_dev import BITS_SHAPES, _bits, bit_checksums, bits_case, device_partial, make_chains, narrow_case, pick_columns
from test_abi import numpy_gelman_partial

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# (chains, p, N, k, row0): the row stride S is odd and larger than the window; p = 200 is a sorted subset of 256 columns
SHAPES = [(3, 65, 2, 65, 7), (3, 80, 17, 80, 1), (2, 129, 65, 129, 3), (3, 200, 333, 256, 101), (4, 256, 333, 256, 0),
          (2, 128, 15, 128, 5), (2, 128, 16, 128, 5), (2, 128, 17, 128, 5), (2, 128, 63, 128, 5), (2, 128, 64, 128, 5),
          (2, 128, 65, 128, 5)]


@functools.lru_cache(maxsize=None)
def case(Cn, p, N, k, row0):
    """Input, device result and numpy reference of one shape, computed once and shared (read-only)."""
    S = row0 + N + 2
    S += 1 - S % 2
    x = make_chains(Cn, k, S, 1000 * p + N)
    cols = pick_columns(k, p, p)
    work, part = device_partial(x, cols, row0, N)
    win = x[:, cols, row0:row0 + N].transpose(0, 2, 1)           # [m][N][p]
    ref = numpy_gelman_partial(win, x[0, cols, row0])
    for a in (x, work, part, win, ref):
        a.setflags(write=False)
    return x, cols, work, part, win, ref


# ------------------------------------------------------------------------------------------------ 1. the partial
@pytest.mark.parametrize("Cn,p,N,k,row0", SHAPES)
def test_partial_equals_its_numpy_definition(Cn, p, N, k, row0):
    x, cols, work, part, win, ref = case(Cn, p, N, k, row0)
    assert not np.isnan(work).any() and not np.isnan(part).any()
    tol = 1e-9 * np.abs(ref) + 1e-11 * np.abs(ref).max()
    print("worst |partial - ref| / tolerance: %.2e" % (np.abs(part - ref) / tol).max())
    assert np.allclose(part, ref, rtol=1e-9, atol=1e-11 * np.abs(ref).max())
    # the per-chain block: {xbar - center, S_c}
    xb = win.mean(1) - x[0, cols, row0]
    assert np.allclose(work[:, :p], xb, rtol=1e-9, atol=1e-11 * np.abs(xb).max())
    Sc = work[:, p:].reshape(Cn, p, p)
    assert np.array_equal(_bits(Sc), _bits(Sc.transpose(0, 2, 1)))     # exactly symmetric


@pytest.mark.parametrize("Cn,p,N", [(3, 65, 17), (3, 200, 70)])
def test_work_and_partial_within_the_a_priori_bounds(Cn, p, N):
    """The yardstick of tests/test_gpu_gelman_narrow.py above 64 columns (the same arithmetic per element): `work` against
    longdouble within the bounds derived in tests/gelman_ref.py, the partial against its definition evaluated in longdouble
    from the device's own `work` within the chain-sum bound."""
    import gelman_ref as R
    k, row0 = p + 3, 5
    x = make_chains(Cn, k, row0 + N + 4, 2000 * p + N)
    cols = np.random.default_rng(p).permutation(k)[:p].astype(np.int32)
    work, part = device_partial(x, cols, row0, N)
    rx, rS = R.work_ratios(work, x, cols, row0, N, x[0, cols, row0])
    rp = R.partial_ratio(part, work, p)
    print("p = %d N = %d: worst ratio xbar %.3f, S %.3f, chain sum %.3f" % (p, N, rx, rS, rp))
    assert rx < 1 and rS < 1 and rp < 1
    assert part[0] == Cn


# ------------------------------------------------------------------------------------------------ 2. finish on the device partial
@pytest.mark.parametrize("Cn,p,N,k,row0", [(4, 256, 333, 256, 0), (3, 200, 333, 256, 101)])
def test_finish_on_the_device_partial_equals_the_oracle(O, Cn, p, N, k, row0):
    """(Most of this test's seconds at p = 256 are the oracle's own cyclic Jacobi eigenvalue sweeps, as in
    tests/test_k256_host.py; the device call and fmcmc_gelman_finish take milliseconds.)"""
    from fmcmc_amd import _abi as abi
    x, cols, work, part, win, ref = case(Cn, p, N, k, row0)
    psrf = np.empty(p); mps = C.c_double(); dp = C.POINTER(C.c_double)
    pc = np.array(part)
    assert abi.lib().fmcmc_gelman_finish(pc.ctypes.data_as(dp), p, N, psrf.ctypes.data_as(dp), C.byref(mps)) == abi.OK
    opsrf, ompsrf = O.gelman(win)
    print("worst psrf distance %.2e, mpsrf %.2e (relative)" % (np.abs(psrf / opsrf - 1).max(), abs(mps.value / ompsrf - 1)))
    assert np.allclose(psrf, opsrf, rtol=1e-9) and abs(mps.value - ompsrf) < 1e-9 * ompsrf


# ------------------------------------------------------------------------------------------------ 3. equalities
@pytest.mark.parametrize("p,N", [(200, 70), (65, 33)])
def test_a_chain_does_not_depend_on_the_launch(p, N):
    row0 = 3
    x = make_chains(5, p, row0 + N + 2, p)
    cols = np.arange(p, dtype=np.int32)
    center = x[0, cols, row0].copy()
    w5, p5 = device_partial(x, cols, row0, N, center)
    w5b, p5b = device_partial(x, cols, row0, N, center)
    assert np.array_equal(_bits(w5), _bits(w5b)) and np.array_equal(_bits(p5), _bits(p5b))       # two calls
    wr, _ = device_partial(x[::-1], cols, row0, N, center)                                       # another place in the launch
    assert np.array_equal(_bits(wr[::-1]), _bits(w5))
    for c in (0, 2, 4):                                                                          # a launch of its own
        w1, _ = device_partial(x[c:c + 1], cols, row0, N, center)
        assert np.array_equal(_bits(w1[0]), _bits(w5[c]))


@pytest.mark.parametrize("Cn,p,N,k,row0", [(3, 65, 2, 65, 7), (2, 129, 65, 129, 3)])
def test_padded_super_blocks_leave_no_nan(Cn, p, N, k, row0):
    """The last super-block holds one live column: the NaN the buffers were filled with is gone from every documented element,
    and the padded columns (which read column 0 and multiply by 0) put none into the live ones."""
    x, cols, work, part, win, ref = case(Cn, p, N, k, row0)
    assert np.isfinite(work).all() and np.isfinite(part).all()
    assert part[0] == Cn


# ------------------------------------------------------------------------------------------------ 4. p <= 64 is untouched
@pytest.mark.parametrize("p", [64, 50])
def test_at_most_64_columns_give_the_bits_of_the_parent(p):
    fx = json.load(open(os.path.join(GOLDEN, "gelman_narrow_bits.json")))["p%d" % p]
    work, part = narrow_case(p)
    assert bit_checksums(work) == fx["work"]
    assert bit_checksums(part) == fx["partial"]


@pytest.mark.parametrize("p,N", BITS_SHAPES)
def test_every_width_gives_the_bits_of_the_two_kernels_before_the_merge(p, N):
    """gelman_cov_mfma against what gelman_chain_mfma (p <= 64) and gelman_pair_mfma (above) left, written by the library of the
    commit before the merge (tests/golden/make_gelman_bits.py): every NA at both ends of its range, 2 to 4 super-blocks."""
    fx = json.load(open(os.path.join(GOLDEN, "gelman_bits.json")))["p%d_N%d" % (p, N)]
    work, part = bits_case(p, N)
    assert bit_checksums(work) == fx["work"]
    assert bit_checksums(part) == fx["partial"]


# ------------------------------------------------------------------------------------------------ 5. the checker and gelman_diag
def test_check_device_and_gelman_diag_at_200_columns(O):
    import torch
    import fmcmc_amd as f
    Cn, p, S = 3, 200, 700
    x = make_chains(Cn, p, S, 5)
    dc = f.DeviceChains(torch.as_tensor(x).cuda(), None, None, np.arange(1, S + 1), 1, None, 0, Cn)
    chk = f.convergence_gelman(100, threshold=1.10)
    verdict = chk.check_device(dc, np.arange(p))
    end, val, psrf = chk.history[-1]
    win = x[:, :, 350:].transpose(0, 2, 1)                       # coda's autoburnin: iterations 351 .. 700
    opsrf, ompsrf = O.gelman(win)
    assert end == S and verdict == bool(ompsrf < 1.10)
    assert np.allclose(psrf, opsrf, rtol=1e-9) and abs(val - ompsrf) < 1e-9 * ompsrf
    g = f.gelman_diag(dc)
    assert isinstance(g, f.GelmanDiag) and (g.start, g.end) == (351, 700) and g.psrf.shape == (p, 2)
    assert np.array_equal(_bits(g.psrf[:, 0]), _bits(psrf)) and g.mpsrf == val
    assert np.all(g.psrf[:, 1] >= g.psrf[:, 0])
    gm = dc.gelman_diag(multivariate=False, autoburnin=False, cols=[3, 150])
    assert gm.mpsrf is None and gm.varnames == ["par4", "par151"] and (gm.start, gm.end) == (1, 700)
    o2, _ = O.gelman(x[:, [3, 150], :].transpose(0, 2, 1))
    assert np.allclose(gm.psrf[:, 0], o2, rtol=1e-9)
