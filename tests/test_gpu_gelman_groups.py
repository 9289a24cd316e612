"""The grouped Gelman-Rubin reduction (fmcmc_gelman_groups_dev, csrc/gelman.hip: gelman_cov_mfma over all chains, then
gelman_group_sum_kernel) on the GPU, without any sampling: seeded random [G Cm][k][S] tensors.

The contract is bitwise: the head of row g of `partials` is what fmcmc_gelman_partial_dev gives for the chains of group g alone,
centred on the window's first row of the group's first chain.  The shapes are the edges of the two kernels: Cm in {2, 3, 4, 5, 9}
(the four strided sums of the group sum: fewer chains than sums, one each, one more, two rounds and a tail), p in {1, 5, 16, 17,
64} (the 16-column blocks), windows of N in {2, 15, 16, 17, 63, 64, 65, 257} rows (the 16-row groups, the four waves, the
three load buffers) that start at row0 > 0 and end before the last row of the buffers."""
import ctypes as C
import warnings

import numpy as np
import pytest

from test_gpu_parity import _bits_equal

pytestmark = pytest.mark.gpu

S, ROW0 = 300, 7
WINDOWS = [2, 15, 16, 17, 63, 64, 65, 257]
SENTINEL = -7.25


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def random_chains(T, nchains, k, seed, rows=S):
    """[nchains][k][rows] on the device: column j of every chain scatters around 100 + 3 j (a centre far from 0, so that the
    subtraction of the group's centre is part of what is compared), every chain around a mean of its own"""
    g = T.Generator(device="cpu").manual_seed(seed)
    x = T.randn((nchains, k, rows), generator=g, dtype=T.float64)
    x += 0.3 * T.randn((nchains, k, 1), generator=g, dtype=T.float64) + (100.0 + 3.0 * T.arange(k, dtype=T.float64))[None, :, None]
    return x.cuda()


def columns(T, k, p):
    """p of the k columns, not the identity: backwards from the last but one"""
    cols = np.arange(k - 2, k - 2 - p, -1, dtype=np.int32)
    assert cols.min() >= 0 and cols.size == p
    return cols, T.as_tensor(cols).cuda()


def groups_dev(T, x, G, Cm, row0, N, cols_d, active=None, fill=SENTINEL):
    """fmcmc_gelman_groups_dev on sentinel-prefilled rows -> (partials [G][plen + 2] on the host, work on the device, code)"""
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    p = int(cols_d.numel())
    plen = int(L.fmcmc_gelman_partial_len(p))
    partials = T.full((G, plen + 2), fill, dtype=T.float64, device=x.device)
    work = T.empty(int(L.fmcmc_gelman_groups_work_len(G, Cm, p)), dtype=T.float64, device=x.device)
    rc = L.fmcmc_gelman_groups_dev(x.data_ptr(), G, Cm, x.shape[1], x.shape[2], row0, N, cols_d.data_ptr(), p,
                                   active.data_ptr() if active is not None else None, work.data_ptr(), partials.data_ptr(),
                                   C.c_void_p(T.cuda.current_stream().cuda_stream))
    T.cuda.synchronize()
    return partials.cpu().numpy(), work, rc


def slice_partial(T, x, g, Cm, row0, N, cols_d):
    """fmcmc_gelman_partial_dev on the chains of group g alone, centred as enqueue_gelman and check_device centre it"""
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import gelman_partial_dev
    L = abi.lib()
    p = int(cols_d.numel())
    own = x[g * Cm:(g + 1) * Cm]
    center = own[0, cols_d.long(), row0].contiguous()
    partial = T.full((int(L.fmcmc_gelman_partial_len(p)),), SENTINEL, dtype=T.float64, device=x.device)
    work = T.empty(int(L.fmcmc_gelman_work_len(Cm, p)), dtype=T.float64, device=x.device)
    gelman_partial_dev(own, Cm, x.shape[1], x.shape[2], row0, N, cols_d, center, work, partial)
    T.cuda.synchronize()
    return partial.cpu().numpy()


@pytest.fixture(scope="module")
def data(T):
    """one tensor per width, shared by the cases of that width and never written: 3 groups of up to 9 chains"""
    made = {}

    def get(p):
        if p not in made:
            made[p] = random_chains(T, 27, p + 2, 1000 + p)
        return made[p]
    return get


@pytest.mark.parametrize("Cm", [2, 3, 4, 5, 9])
@pytest.mark.parametrize("p", [1, 5, 16, 17, 64])
def test_every_row_is_the_partial_of_its_group_alone(T, data, p, Cm):
    from fmcmc_amd import _abi as abi
    G = 3
    x = data(p)[:G * Cm]
    cols, cols_d = columns(T, p + 2, p)
    for N in WINDOWS:
        assert ROW0 > 0 and S > ROW0 + N
        got, _work, rc = groups_dev(T, x, G, Cm, ROW0, N, cols_d)
        assert rc == abi.OK, abi.last_error()
        for g in range(G):
            ref = slice_partial(T, x, g, Cm, ROW0, N, cols_d)
            assert ref[0] == Cm and np.isfinite(ref).all()
            assert _bits_equal(got[g, :-2], ref), "p = %d, Cm = %d, N = %d, group %d" % (p, Cm, N, g)
        # the two sums of rm_invariant's test, against the window itself.  They are formed from the chains' means and
        # variances: sum x^2 = sum over chains and columns of (N - 1) s2 + N xbar^2, each term within a few N u of the exact
        # one, and at most 9 x 64 x 257 = 1.5e5 values near 100 enter: 1e-10 relative is several hundred times that.
        w = x[:, cols_d.long(), ROW0:ROW0 + N].cpu().numpy().reshape(G, -1)
        np.testing.assert_allclose(got[:, -2], w.sum(axis=1), rtol=1e-10)
        np.testing.assert_allclose(got[:, -1], (w * w).sum(axis=1), rtol=1e-10)


def test_masked_groups_keep_their_rows(T, data):
    """inactive first, middle and last groups: their sentinel-prefilled rows are untouched, the others are the slices' partials"""
    from fmcmc_amd import _abi as abi
    G, Cm, p, N = 5, 3, 5, 65
    x = data(p)[:G * Cm]
    cols, cols_d = columns(T, p + 2, p)
    mask = T.as_tensor(np.array([0, 1, 0, 1, 0], dtype=np.int32)).cuda()
    got, _work, rc = groups_dev(T, x, G, Cm, ROW0, N, cols_d, mask)
    assert rc == abi.OK, abi.last_error()
    for g in (0, 2, 4):
        assert (got[g] == SENTINEL).all()
    for g in (1, 3):
        assert _bits_equal(got[g, :-2], slice_partial(T, x, g, Cm, ROW0, N, cols_d))
    ones, _w, rc = groups_dev(T, x, G, Cm, ROW0, N, cols_d, T.ones(G, dtype=T.int32, device="cuda"))
    full, _w, rc2 = groups_dev(T, x, G, Cm, ROW0, N, cols_d, None)
    assert rc == rc2 == abi.OK and _bits_equal(ones, full) and _bits_equal(full[[1, 3]], got[[1, 3]])


def test_an_all_zero_mask_returns_ok_and_writes_nothing(T, data):
    from fmcmc_amd import _abi as abi
    G, Cm, p = 4, 2, 17
    x = data(p)[:G * Cm]
    _cols, cols_d = columns(T, p + 2, p)
    got, _work, rc = groups_dev(T, x, G, Cm, ROW0, 64, cols_d, T.zeros(G, dtype=T.int32, device="cuda"))
    assert rc == abi.OK, abi.last_error()
    assert (got == SENTINEL).all()


def test_wider_than_a_wavefront_is_refused(T):
    from fmcmc_amd import _abi as abi
    x = random_chains(T, 4, 66, 3, rows=40)
    cols_d = T.arange(65, dtype=T.int32).cuda()
    _got, _work, rc = groups_dev(T, x, 2, 2, 0, 40, cols_d)
    assert rc == abi.ERR_UNSUPPORTED and "FMCMC_MAX_K_WAVE" in abi.last_error()


@pytest.mark.parametrize("p", [1, 3])
def test_a_group_of_constant_columns_is_not_converged_as_check_device_says(T, p):
    """group 1 of 3: every column constant (column j holds j + 1 in every chain and row).  At p = 1 rm_invariant's variance of
    all entries is 0; at p = 3 it is not (the columns differ) and W = 0 fails the finish instead.  Both are check_device's
    verdicts on the dataset alone; the other groups give its verdict and its statistic to the bit."""
    import fmcmc_amd as F
    G, Cm, k, rows = 3, 4, p + 1, 120
    x = random_chains(T, G * Cm, k, 50 + p, rows=rows)
    x[Cm:2 * Cm] = (T.arange(k, dtype=T.float64) + 1.0)[None, :, None].cuda()
    iters = np.arange(1, rows + 1)
    cols = np.arange(p, dtype=np.int32)
    cols_d = T.as_tensor(cols).cuda()
    from fmcmc_amd.convergence import _window
    row0, N = _window(iters)
    got, _work, rc = groups_dev(T, x, G, Cm, row0, N, cols_d)
    assert rc == 0
    plen = got.shape[1] - 2
    for g in range(G):
        theirs, mine = F.convergence_gelman(10, threshold=3.0), F.convergence_gelman(10, threshold=3.0)
        dc = F.DeviceChains(x[g * Cm:(g + 1) * Cm], None, None, iters, 1, None, 0, Cm)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a = theirs.check_device(dc, cols)
            b = mine._finish(got[g], p, N, int(iters[-1]), plen, Cm)
        assert a == b == (g != 1), "group %d" % g
        if g == 1:
            assert theirs.last is None and mine.last is None
            if p == 1:
                cnt = Cm * p * N
                assert (got[g, plen + 1] - got[g, plen] ** 2 / cnt) / (cnt - 1) < 1e-10
        else:
            assert theirs.last == mine.last and np.isfinite(mine.last)


def _batch_of(T, F, D, Cm, k, rows, seed, **kw):
    x = random_chains(T, D * Cm, k, seed, rows=rows)
    dc = F.DeviceChains(x, None, None, np.arange(1, rows + 1), 1, ["v%d" % j for j in range(k)], 0, D * Cm)
    dc.accept_count = T.zeros(D * Cm, dtype=T.int64, device="cuda")
    return F.McmcBatch(dc, D, Cm, **kw)


def _same_diag(g, h):
    assert _bits_equal(g.psrf[:, 0], h.psrf[:, 0]) and _bits_equal(g.psrf[:, 1], h.psrf[:, 1])
    assert g.mpsrf == h.mpsrf and g.varnames == h.varnames and (g.start, g.end, g.confidence) == (h.start, h.end, h.confidence)


@pytest.mark.parametrize("kw", [dict(), dict(autoburnin=False), dict(cols=[3, 0]), dict(confidence=0.9, multivariate=False),
                                dict(cols=[2])])
def test_gelman_diag_of_a_batch_is_gelman_diag_of_every_dataset(T, kw):
    import fmcmc_amd as F
    D, Cm, k = 4, 3, 5
    ans = _batch_of(T, F, D, Cm, k, 120, 9)
    got = ans.gelman_diag(**kw)
    assert isinstance(got, F.GelmanDiagBatch) and len(got) == D
    p = len(kw.get("cols", range(k)))
    assert got.psrf.shape == (D, p, 2) and got.mpsrf.shape == (D,)
    for d in range(D):
        h = F.gelman_diag(ans[d], **kw)
        _same_diag(got[d], h)
        assert _bits_equal(got.psrf[d], h.psrf)
        assert (np.isnan(got.mpsrf[d]) and h.mpsrf is None) or got.mpsrf[d] == h.mpsrf
    again = F.gelman_diag(ans, **kw)
    assert _bits_equal(again.psrf, got.psrf)


def test_gelman_diag_of_a_ragged_batch_uses_every_datasets_own_rows(T):
    import fmcmc_amd as F
    D, Cm, k = 4, 2, 3
    nrows = np.array([120, 60, 90, 60])
    ans = _batch_of(T, F, D, Cm, k, 120, 10, nrows=nrows, steps=nrows, converged=[False, True, True, True])
    got = ans.gelman_diag()
    for d in range(D):
        assert ans[d].nrows == nrows[d]
        h = F.gelman_diag(ans[d])
        _same_diag(got[d], h)
        assert h.end == nrows[d] and h.start == nrows[d] // 2 + 1
