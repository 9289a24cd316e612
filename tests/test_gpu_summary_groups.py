"""The grouped posterior summary (fmcmc_summary_groups_dev, csrc/summary.hip: stages 1-2 over all chains, then one pool and one
select workgroup per (group, column)) on the GPU, without any sampling: seeded [G Cm][k][S] tensors.

The contract is bitwise and there is no tolerance: row g of `pooled`, the group's rows of `chain_stats` and the slots 0..67 of its
series in `work` are what fmcmc_summary_dev writes for the chains of group g alone; the order statistics are also those of
np.sort of the group's pooled values.  Every group and column sits at an offset of its own (+-1e6 g), so one value that leaks
across a group boundary moves an order statistic.  Every window starts at an odd row of a buffer with an odd row stride and
ends before its last row, so every segment of the select starts on an odd offset.  The outputs are prefilled with a sentinel and
carry guard elements behind them that must stay untouched."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_parity import _bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 5
ROW0 = 3
ACS, HEAD = 72, 68                 # doubles per series in `work`, and how many of them the kernels write
DEFAULT = (0.025, 0.25, 0.5, 0.75, 0.975)
SIXTEEN = (0.0, 1.0, 0.5, 0.5, 0.01, 0.99, 0.25, 0.75, 0.1, 0.9, 0.333, 0.667, 0.025, 0.975, 0.5, 0.0)


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def stride_for(N):
    """an odd row stride that leaves rows behind the window [ROW0, ROW0 + N)"""
    S = ROW0 + N + 2
    return S + 1 - S % 2


def offsets(G, Cm, k):
    """[G Cm][k][1]: +-1e6 g per (group, column), both signs among the columns of a group and among the groups of a column"""
    g = np.repeat(np.arange(G), Cm)[:, None]
    j = np.arange(k)[None, :]
    return (1e6 * g * np.where((g + j) % 2 == 0, 1.0, -1.0) + 10.0 * j)[:, :, None]


def random_groups(T, G, Cm, k, N, seed):
    """host [G Cm][k][S] and its device copy: an AR(1)-like series per (chain, column) around the offset of its group and column"""
    rng = np.random.default_rng(seed)
    S = stride_for(N)
    e = rng.standard_normal((G * Cm, k, S))
    x = e.copy()
    x[:, :, 1:] += 0.6 * e[:, :, :-1]
    x += offsets(G, Cm, k)
    return x, T.as_tensor(x).cuda()


def _call(T, entry, x, head, N, cols, probs, tail, lens):
    """entry(samples, *head, k, S, ROW0, N, cols, p, *tail(probs, nprobs, work, chain_stats, pooled), stream) on sentinel-filled
    buffers of lens = (work, chain_stats or None, pooled) doubles plus GUARD -> the three host arrays without the guards"""
    cols_d = T.as_tensor(np.asarray(cols, dtype=np.int32)).cuda()
    probs_h = np.ascontiguousarray(probs, dtype=np.float64)
    bufs = [None if n is None else T.full((int(n) + GUARD,), SENTINEL, dtype=T.float64, device="cuda") for n in lens]
    ptr = [None if b is None else b.data_ptr() for b in bufs]
    rc = entry(x.data_ptr(), *head, x.shape[1], x.shape[2], ROW0, N, cols_d.data_ptr(), len(cols),
               *tail(probs_h.ctypes.data_as(C.POINTER(C.c_double)), len(probs), *ptr), C.c_void_p(T.cuda.current_stream().cuda_stream))
    T.cuda.synchronize()
    out = []
    for b, n in zip(bufs, lens):
        if b is None:
            out.append(None)
            continue
        h = b.cpu().numpy()
        assert (h[int(n):] == SENTINEL).all(), "the guard elements behind a buffer were written"
        out.append(h[:int(n)])
    return rc, out


def groups_dev(T, x, G, Cm, N, cols, probs, active=None, want_chains=True):
    """fmcmc_summary_groups_dev -> pooled [G][plen], chain [G Cm][p][4] (or None), acov [G Cm p][72], rest of work, code"""
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    p, nprobs = len(cols), len(probs)
    plen = int(L.fmcmc_summary_pooled_len(p, nprobs))
    series = G * Cm * p
    wl = int(L.fmcmc_summary_groups_work_len(G, Cm, p, nprobs))
    assert wl == series * (ACS + 4)
    act = None if active is None else T.as_tensor(np.asarray(active, dtype=np.int32)).cuda()
    rc, (work, chain, pooled) = _call(
        T, L.fmcmc_summary_groups_dev, x, (G, Cm), N, cols, probs,
        lambda pr, npr, w, c, po: (None if act is None else act.data_ptr(), pr, npr, w, c, po),
        (wl, series * 4 if want_chains else None, G * plen))
    assert rc == abi.OK, abi.last_error()
    return SimpleNamespace(pooled=pooled.reshape(G, plen), chain=None if chain is None else chain.reshape(G * Cm, p, 4),
                           acov=work[:series * ACS].reshape(series, ACS), tail=work[series * ACS:].reshape(series, 4))


def single_dev(T, own, N, cols, probs):
    """fmcmc_summary_dev on the chains `own` alone -> pooled [plen], chain [Cm][p][4], acov [Cm p][72]"""
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    Cm, p, nprobs = int(own.shape[0]), len(cols), len(probs)
    plen = int(L.fmcmc_summary_pooled_len(p, nprobs))
    rc, (work, chain, pooled) = _call(T, L.fmcmc_summary_dev, own, (Cm,), N, cols, probs, lambda pr, npr, w, c, po: (pr, npr, w, c, po),
                                      (int(L.fmcmc_summary_work_len(Cm, p, nprobs)), Cm * p * 4, plen))
    assert rc == abi.OK, abi.last_error()
    return SimpleNamespace(pooled=pooled, chain=chain.reshape(Cm, p, 4), acov=work[:Cm * p * ACS].reshape(Cm * p, ACS))


def sorted_order_stats(xh, g, Cm, N, cols, probs):
    """[p][nprobs][2] from np.sort of the pooled host values of group g at type7_order_ranks"""
    from fmcmc_amd.summary import type7_order_ranks
    ranks = type7_order_ranks(Cm * N, np.asarray(probs, dtype=np.float64))
    return np.stack([np.sort(xh[g * Cm:(g + 1) * Cm, c, ROW0:ROW0 + N].ravel())[ranks] for c in cols])


def check_groups(T, xh, xd, G, Cm, N, cols, probs, groups=None, exact_sort=True):
    """every (or each listed) group of the grouped call against the single call on its chains and against np.sort"""
    got = groups_dev(T, xd, G, Cm, N, cols, probs)
    p, nprobs = len(cols), len(probs)
    for g in (range(G) if groups is None else groups):
        what = "G = %d, Cm = %d, N = %d, cols = %s, nprobs = %d, group %d" % (G, Cm, N, list(cols), nprobs, g)
        ref = single_dev(T, xd[g * Cm:(g + 1) * Cm], N, cols, probs)
        assert _bits_equal(got.pooled[g], ref.pooled), what
        assert _bits_equal(got.chain[g * Cm:(g + 1) * Cm], ref.chain), what
        rows = slice(g * Cm * p, (g + 1) * Cm * p)
        assert _bits_equal(got.acov[rows, :HEAD], ref.acov[:, :HEAD]), what
        assert (got.acov[rows, HEAD:] == SENTINEL).all() and (got.tail[rows] == SENTINEL).all(), what
        if nprobs:
            os_ = got.pooled[g, 5 * p:].reshape(p, nprobs, 2)
            want = sorted_order_stats(xh, g, Cm, N, cols, probs)
            assert _bits_equal(os_, want) if exact_sort else np.array_equal(os_, want), what
    return got


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("N", [3, 4, 17, 1025])
@pytest.mark.parametrize("Cm", [1, 2, 4, 5, 9])
def test_every_group_is_the_single_call_on_its_chains(T, Cm, N):
    G, k = 3, 4
    xh, xd = random_groups(T, G, Cm, k, N, 100 * Cm + N)
    assert xd.shape[2] % 2 == 1 and ROW0 % 2 == 1 and ROW0 + N < xd.shape[2]
    check_groups(T, xh, xd, G, Cm, N, [2, 0, 3], DEFAULT)


def test_one_group_is_the_whole_single_call(T):
    Cm, N, cols = 4, 17, [2, 0, 3]
    xh, xd = random_groups(T, 1, Cm, 4, N, 7)
    got = check_groups(T, xh, xd, 1, Cm, N, cols, DEFAULT)
    ref = single_dev(T, xd, N, cols, DEFAULT)
    assert _bits_equal(got.pooled.ravel(), ref.pooled) and _bits_equal(got.chain, ref.chain)
    assert _bits_equal(got.acov[:, :HEAD], ref.acov[:, :HEAD])


def test_three_hundred_and_one_groups(T):
    G, Cm, N = 301, 2, 17
    xh, xd = random_groups(T, G, Cm, 4, N, 8)
    check_groups(T, xh, xd, G, Cm, N, [3, 3], DEFAULT)


@pytest.mark.parametrize("Cm,N", [(2, 4095), (2, 4096), (2, 4097),       # around one batch of the pair walk: 2 x 4 x 512 rows
                                  (4, 4864), (4, 4865), (1, 19457)])      # 19456 keys are staged in LDS, one more is not
def test_around_the_pair_walk_batch_and_the_lds_limit(T, Cm, N):
    G = 2
    xh, xd = random_groups(T, G, Cm, 2, N, Cm + N)
    check_groups(T, xh, xd, G, Cm, N, [1], DEFAULT)


@pytest.mark.parametrize("probs", [(), (0.5,), DEFAULT, SIXTEEN])
@pytest.mark.parametrize("cols", [[2, 0, 3], [3, 3], [1]])
def test_columns_and_probs(T, cols, probs):
    assert len(SIXTEEN) == 16 and 0.0 in SIXTEEN and 1.0 in SIXTEEN and len(set(SIXTEEN)) < 16
    G, Cm, N = 3, 4, 129
    xh, xd = random_groups(T, G, Cm, 4, N, 11)
    check_groups(T, xh, xd, G, Cm, N, cols, probs)


# ------------------------------------------------------------------------------------------------------------------ keys
def test_ties_and_a_constant_column(T):
    """two decimals: many equal values; group 1's column 0 is one constant: every target keeps one prefix through all passes"""
    G, Cm, N = 3, 4, 257
    xh, _ = random_groups(T, G, Cm, 2, N, 12)
    xh = np.round(xh, 2)
    xh[Cm:2 * Cm, 0, :] = -1e6 + 0.25
    got = check_groups(T, xh, T.as_tensor(xh).cuda(), G, Cm, N, [0, 1], SIXTEEN)
    assert (got.pooled[1, 10:10 + 32] == -1e6 + 0.25).all() and got.pooled[1, 1] == 0.0


def test_thirty_two_leaders_are_alive_at_once(T):
    """32 distinct magnitudes whose keys differ in the first digit, eight of each in a group, and 16 probs whose lo and hi fall
    on the two sides of a boundary between magnitudes: 32 targets with 32 different prefixes after the first pass, more than
    one walk's four histograms"""
    G, Cm, N, b = 2, 4, 64, 8
    mags = np.array([s * 2.0 ** (16 * (i - 8)) for i in range(16) for s in (1.0, -1.0)])
    assert len(set(mags)) == 32 and Cm * N == 32 * b
    rng = np.random.default_rng(13)
    S = stride_for(N)
    xh = rng.standard_normal((G * Cm, 1, S))
    for g in range(G):
        vals = rng.permutation(np.repeat(mags * (1.0 + g), b))
        xh[g * Cm:(g + 1) * Cm, 0, ROW0:ROW0 + N] = vals.reshape(Cm, N)
    probs = tuple(((2 * q + 1) * b - 0.5) / (Cm * N - 1) for q in range(16))
    want = sorted_order_stats(xh, 0, Cm, N, [0], probs)
    assert len(set(want.ravel())) == 32
    check_groups(T, xh, T.as_tensor(xh).cuda(), G, Cm, N, [0], probs)


def test_signed_zeros_subnormals_the_largest_doubles_and_one_sided_groups(T):
    """group 0 all negative, group 1 all positive, group 2 the edge values: -0.0 beside +0.0 (equal to np.sort's as values: it
    does not order them), subnormals beside +-DBL_MAX"""
    G, Cm, N = 3, 2, 33
    rng = np.random.default_rng(14)
    S = stride_for(N)
    xh = np.abs(rng.standard_normal((G * Cm, 1, S))) + 0.5
    xh[:Cm] *= -1.0
    big, tiny = np.finfo(np.float64).max, 5e-324
    edge = np.array([0.0, -0.0, tiny, -tiny, 3 * tiny, big, -big, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0])
    xh[2 * Cm:, 0, ROW0:ROW0 + N] = rng.choice(edge, size=(Cm, N))
    xh[2 * Cm, 0, ROW0:ROW0 + 4] = [0.0, -0.0, -0.0, 0.0]
    check_groups(T, xh, T.as_tensor(xh).cuda(), G, Cm, N, [0], SIXTEEN, exact_sort=False)


# ---------------------------------------------------------------------------------------------- position, mask, non-finite
def test_a_group_gives_the_same_bits_wherever_it_sits(T):
    Cm, N, cols, p = 2, 17, [2, 0], 2
    _, x301 = random_groups(T, 301, Cm, 3, N, 15)
    blk = x301[600:602].clone()
    x5 = x301[:10].clone()
    x5[4:6] = blk
    runs = [(groups_dev(T, blk, 1, Cm, N, cols, DEFAULT), 0), (groups_dev(T, x5, 5, Cm, N, cols, DEFAULT), 2),
            (groups_dev(T, x301, 301, Cm, N, cols, DEFAULT), 300)]
    a = runs[0][0]
    for r, g in runs[1:]:
        assert _bits_equal(r.pooled[g], a.pooled[0]) and _bits_equal(r.chain[g * Cm:(g + 1) * Cm], a.chain)
        assert _bits_equal(r.acov[g * Cm * p:(g + 1) * Cm * p], a.acov)


def test_the_mask(T):
    G, Cm, N, cols, p = 5, 3, 65, [1, 2], 2
    _, xd = random_groups(T, G, Cm, 3, N, 16)
    full = groups_dev(T, xd, G, Cm, N, cols, DEFAULT)
    ones = groups_dev(T, xd, G, Cm, N, cols, DEFAULT, active=[1] * G)
    for f in ("pooled", "chain", "acov", "tail"):
        assert _bits_equal(getattr(ones, f), getattr(full, f)), f
    mask = [0, 1, 0, 1, 0]
    for want_chains in (True, False):
        got = groups_dev(T, xd, G, Cm, N, cols, DEFAULT, active=mask, want_chains=want_chains)
        for g in range(G):
            ch, se = slice(g * Cm, (g + 1) * Cm), slice(g * Cm * p, (g + 1) * Cm * p)
            stats = got.chain[ch].reshape(-1, 4) if want_chains else got.tail[se]
            if mask[g]:
                assert _bits_equal(got.pooled[g], full.pooled[g]) and _bits_equal(got.acov[se], full.acov[se])
                assert _bits_equal(stats, full.chain[ch].reshape(-1, 4))
            else:
                assert (got.pooled[g] == SENTINEL).all() and (got.acov[se] == SENTINEL).all() and (stats == SENTINEL).all()
        if want_chains:
            assert (got.tail == SENTINEL).all()
    none = groups_dev(T, xd, G, Cm, N, cols, DEFAULT, active=[0] * G)
    assert (none.pooled == SENTINEL).all() and (none.chain == SENTINEL).all() and (none.acov == SENTINEL).all()


def test_non_finite_values_are_counted_in_their_group_alone(T):
    G, Cm, N, cols = 3, 2, 40, [0, 1]
    xh, xd = random_groups(T, G, Cm, 2, N, 17)
    clean = groups_dev(T, xd, G, Cm, N, cols, DEFAULT)
    assert (clean.pooled[:, [4, 9]] == 0.0).all()
    bad = xd.clone()
    bad[2, 1, ROW0 + 5] = float("nan")
    bad[3, 1, ROW0 + N - 1] = float("inf")
    bad[0, 1, ROW0 + N] = float("nan")          # (behind the window: not counted)
    got = groups_dev(T, bad, G, Cm, N, cols, DEFAULT)
    assert got.pooled[1, 4] == 0.0 and got.pooled[1, 9] == 2.0
    for g in (0, 2):
        assert _bits_equal(got.pooled[g], clean.pooled[g]) and _bits_equal(got.chain[g * Cm:(g + 1) * Cm], clean.chain[g * Cm:(g + 1) * Cm])
    ref = single_dev(T, bad[Cm:2 * Cm], N, cols, DEFAULT)
    assert _bits_equal(got.pooled[1], ref.pooled) and _bits_equal(got.chain[Cm:2 * Cm], ref.chain)


# -------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw,code", [(dict(G=0), "ERR_ARG"), (dict(Cm=0), "ERR_ARG"), (dict(N=2), "ERR_ARG"),
                                     (dict(nprobs=17), "ERR_ARG"), (dict(probs=[1.5]), "ERR_ARG"), (dict(samples=None), "ERR_ARG"),
                                     (dict(pooled=None), "ERR_ARG"), (dict(work=None), "ERR_ARG"), (dict(cols=None), "ERR_ARG"),
                                     (dict(probs=None), "ERR_ARG"), (dict(Cm=1 << 31, G=1), "ERR_UNSUPPORTED")])
def test_refusals_come_before_any_device_call(T, kw, code):
    """the buffers keep their sentinel: nothing ran"""
    from fmcmc_amd import _abi as abi
    G, Cm, N, k = 2, 2, 10, 2
    _, xd = random_groups(T, G, Cm, k, N, 18)
    bufs = dict(work=T.full((G * Cm * k * 76,), SENTINEL, dtype=T.float64, device="cuda"),
                pooled=T.full((G * 64,), SENTINEL, dtype=T.float64, device="cuda"),
                cols=T.arange(k, dtype=T.int32).cuda(), samples=xd)
    a = dict(G=G, Cm=Cm, N=N, nprobs=None, probs=[0.5], **{n: b.data_ptr() for n, b in bufs.items()})
    a.update(kw)
    pr = None if a["probs"] is None else np.ascontiguousarray(a["probs"] + [0.5] * 16, dtype=np.float64)
    nprobs = a["nprobs"] if a["nprobs"] is not None else (1 if pr is None else len(a["probs"]))
    rc = abi.lib().fmcmc_summary_groups_dev(a["samples"], a["G"], a["Cm"], k, xd.shape[2], ROW0, a["N"], a["cols"], k, None,
                                            None if pr is None else pr.ctypes.data_as(C.POINTER(C.c_double)), nprobs, a["work"],
                                            None, a["pooled"], None)
    T.cuda.synchronize()
    assert rc == getattr(abi, code) and "fmcmc_summary_groups_dev" in abi.last_error()
    assert (bufs["work"] == SENTINEL).all() and (bufs["pooled"] == SENTINEL).all()


def test_groups_that_are_not_the_chains_of_the_result_are_refused(T):
    import fmcmc_amd as F
    from fmcmc_amd.summary import enqueue_summary_groups
    _, xd = random_groups(T, 3, 2, 2, 10, 19)
    dc = F.DeviceChains(xd, None, None, np.arange(1, xd.shape[2] + 1), 1, None, 0, 6)
    with pytest.raises(ValueError, match="4 groups of 2 chains are not the 6 chains"):
        enqueue_summary_groups(dc, 4, 2, 0, 10, None, DEFAULT)
    pooled, chain, _work, cols = enqueue_summary_groups(dc, 3, 2, 0, 10, None, DEFAULT)
    assert tuple(pooled.shape) == (3, 2 * 5 + 2 * 5 * 2) and tuple(chain.shape) == (6, 2, 4) and cols.tolist() == [0, 1]
