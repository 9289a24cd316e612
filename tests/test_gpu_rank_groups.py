"""The grouped rank-normalised split R-hat on the GPU (fmcmc_rank_rhat_groups_dev, csrc/diag_rank_groups.hpp: one workgroup per
(group, column), the keys sorted in LDS) and rhat() of an McmcBatch on top of it.  Every group's `out` and scores are held bit
for bit to fmcmc_rank_rhat_dev / fmcmc_rank_scores_dev on that group alone (tests/test_gpu_rank_rhat.py: raw, make_inputs), one
shape also to scipy's rankdata and the oracle's qnorm; the moments to np.longdouble under the bounds of tests/rhat_cases.py.  The
raw entry is called with NaN-filled buffers GUARD elements longer than documented, which must stay NaN."""
import functools
import os

import numpy as np
import pytest

import rhat_cases as rc
from gelman_dev import GUARD
from test_gpu_rank_rhat import NCOLS, _bits, make_inputs, pooled_median, raw, split, twice_ranks

pytestmark = pytest.mark.gpu

ALL = tuple(range(NCOLS))
P = 1 << 11                         # the power of two nearest 2048 that a group's keys are padded to (rank_groups_pad)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the raw call
def groups_raw(x, G, Cm, row0, N, cols, active=None, scores=True, stream=None, stage=None):
    """L.fmcmc_rank_rhat_groups_dev on x [G Cm][k][S]: work, scores and out NaN-filled and GUARD longer than documented ->
    (out [G][p][8 Cm + 2], scores [G][p][2][2 Cm][N'] or None).  stream / stage as tests/test_gpu_rank_rhat.py: raw has them."""
    import torch
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    Cn, k, S = x.shape
    assert Cn == G * Cm
    p, nh = len(cols), N // 2
    M = 2 * Cm * nh
    lens = [L.fmcmc_rank_rhat_groups_work_len(G, Cm, p, N), G * p * 2 * M if scores else 0, G * p * (8 * Cm + 2)]
    assert lens[0] > 0
    nan = lambda n: torch.full((int(n) + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    bufs = [nan(n) for n in lens]
    cd = torch.as_tensor(np.asarray(cols, dtype=np.int32)).cuda()
    ad = None if active is None else torch.as_tensor(np.asarray(active, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    xd = torch.as_tensor(x).cuda() if stage is None else stage()
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        if stage is not None:
            xd.copy_(torch.as_tensor(x).pin_memory(), non_blocking=True)
        rcode = L.fmcmc_rank_rhat_groups_dev(xd.data_ptr(), G, Cm, k, S, row0, N, cd.data_ptr(), p,
                                             None if ad is None else ad.data_ptr(), bufs[0].data_ptr(),
                                             bufs[1].data_ptr() if scores else None, bufs[2].data_ptr(), st.cuda_stream)
    assert rcode == abi.OK, (rcode, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    assert np.isnan(host[0]).all()                                                # work is not touched
    assert all(np.isnan(h[int(n):]).all() for h, n in zip(host, lens))          # nothing past the documented lengths
    out = host[2][:lens[2]].reshape(G, p, 8 * Cm + 2)
    return out, (host[1][:lens[1]].reshape(G, p, 2, 2 * Cm, nh) if scores else None)


def single(x, g, Cm, row0, N, cols):
    """the single form on group g alone: (out [p][8 Cm + 2], scores [p][2][2 Cm][N'])"""
    xg = np.ascontiguousarray(x[g * Cm:(g + 1) * Cm])
    out = raw("rhat", xg, row0, N, cols)
    z = np.stack([raw("scores", xg, row0, N, cols, (fold, 0))[0] for fold in (0, 1)], axis=1)
    return out, z


# (ngroups, cpg, N): M = 4 and 8; odd N; M = P - 2, P, P + 2; M at the limit with two groups; (5, 3, 400); more workgroups than
# CUs.  make_inputs gives row0 = 3 and an odd S throughout.
SHAPES = [(1, 1, 4), (3, 1, 5), (2, 2, 4), (2, 3, 5), (2, 7, 1025), (2, 1, P - 2), (2, 2, P // 2), (2, 1, P + 2), (2, 2, 4096),
          (5, 3, 400), (300, 1, 8)]


def test_the_shapes_are_the_edges_they_claim():
    from fmcmc_amd import _abi as abi
    top = abi.lib().fmcmc_rank_groups_max_values()
    M = [2 * c * (n // 2) for _g, c, n in SHAPES]
    assert {4, 8, P - 2, P, P + 2, top, 1200} <= set(M) and max(M) == top
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fmcmc_amd", "csrc",
                            "diag_rank_groups.hpp")).read()
    assert "while (P < M) P <<= 1;" in src                                       # the pad is the next power of two


@functools.lru_cache(maxsize=None)
def groups_case(G, Cm, N):
    cols = (0, 5) if G == 300 else ALL
    x, row0 = make_inputs(G * Cm, N, 1000 * G + 100 * Cm + N)
    out, z = groups_raw(x, G, Cm, row0, N, cols)
    for a in (out, z):
        a.setflags(write=False)
    return x, row0, cols, out, z


@pytest.mark.parametrize("G, Cm, N", SHAPES)
def test_every_group_bit_for_bit_the_single_form(G, Cm, N):
    x, row0, cols, out, z = groups_case(G, Cm, N)
    m = 2 * Cm
    for g in range(G):
        want_out, want_z = single(x, g, Cm, row0, N, cols)
        assert _same(out[g], want_out), (g, np.nonzero(_bits(out[g]) != _bits(want_out)))
        assert _same(z[g], want_z), g
        for j, col in enumerate(cols):
            assert out[g, j, 4 * m] == 0.0
            assert _bits(out[g, j, 4 * m + 1]) == _bits(pooled_median(split(x[g * Cm:(g + 1) * Cm], row0, N, col))), (g, col)


def test_scores_against_rankdata_and_the_oracles_qnorm(O):
    G, Cm, N = 5, 3, 400
    x, row0, cols, out, z = groups_case(G, Cm, N)
    M = 2 * Cm * (N // 2)
    for g in range(G):
        for j, col in enumerate(cols):
            v = split(x[g * Cm:(g + 1) * Cm], row0, N, col)
            for fold, w in enumerate((v, np.abs(v - pooled_median(v)))):
                arg = np.ascontiguousarray((0.5 * twice_ranks(w) - 0.375) / (M + 0.25))
                want = np.empty_like(arg)
                O.lib().fmcmc_oracle_detmath(3, O._p(arg.ravel()), O._p(want.reshape(-1)), arg.size)
                assert _same(z[g, j, fold], want), (g, col, fold)


# ------------------------------------------------------------------------------------------------ active
def test_inactive_groups_keep_their_prefill():
    G, Cm, N = 5, 3, 400
    x, row0, cols, out, z = groups_case(G, Cm, N)
    mask = [1, 0, 1, 1, 0]
    mo, mz = groups_raw(x, G, Cm, row0, N, cols, active=mask)
    for g, on in enumerate(mask):
        if on:
            assert _same(mo[g], out[g]) and _same(mz[g], z[g]), g
        else:
            assert np.isnan(mo[g]).all() and np.isnan(mz[g]).all(), g
    ones, _ = groups_raw(x, G, Cm, row0, N, cols, active=[1] * G, scores=False)
    assert _same(ones, out)
    none, nz = groups_raw(x, G, Cm, row0, N, cols, active=[0] * G)
    assert np.isnan(none).all() and np.isnan(nz).all()


# ------------------------------------------------------------------------------------------------ independence of the launch
def test_two_launches_agree_with_and_without_scores():
    G, Cm, N = 2, 7, 1025
    x, row0, cols, out, z = groups_case(G, Cm, N)
    again, z2 = groups_raw(x, G, Cm, row0, N, cols)
    assert _same(again, out) and _same(z2, z)
    bare, none = groups_raw(x, G, Cm, row0, N, cols, scores=False)
    assert none is None and _same(bare, out)


def test_a_group_elsewhere_in_a_larger_call():
    G, Cm, N = 5, 3, 400
    x, row0, cols, out, z = groups_case(G, Cm, N)
    other, _ = make_inputs(4 * Cm, N, 4242)
    y = np.ascontiguousarray(np.concatenate([other[:2 * Cm], x[3 * Cm:4 * Cm], other[2 * Cm:], x[:Cm]]))
    yo, yz = groups_raw(y, 6, Cm, row0, N, cols)
    assert _same(yo[2], out[3]) and _same(yz[2], z[3]) and _same(yo[5], out[0]) and _same(yz[5], z[0])


def test_a_column_alone_and_among_three_in_another_order():
    G, Cm, N = 5, 3, 400
    x, row0, cols, out, z = groups_case(G, Cm, N)
    three, z3 = groups_raw(x, G, Cm, row0, N, (3, 0, 1))
    for j, col in enumerate((3, 0, 1)):
        alone, z1 = groups_raw(x, G, Cm, row0, N, (col,))
        assert _same(alone[:, 0], three[:, j]) and _same(alone[:, 0], out[:, col]), col
        assert _same(z1[:, 0], z3[:, j]) and _same(z1[:, 0], z[:, col]), col


def test_a_side_stream_behind_a_busy_stream():
    """the rows reach the device ON the side stream, behind a kernel that keeps it busy: a call that left its caller's stream
    would read the NaN prefill"""
    import torch
    G, Cm, N = 5, 3, 400
    x, row0, cols, out, z = groups_case(G, Cm, N)
    side = torch.cuda.Stream()

    def stage():
        xd = torch.full(x.shape, float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(4_000_000)             # a few milliseconds
        return xd

    got, gz = groups_raw(x, G, Cm, row0, N, cols, stream=side, stage=stage)
    assert _same(got, out) and _same(gz, z)


# ------------------------------------------------------------------------------------------------ the reduction and R-hat
@pytest.mark.parametrize("G, Cm, N", [(2, 2, 4), (3, 7, 1025)])
def test_moments_and_rhat_within_the_derived_bounds(G, Cm, N):
    """the means and variances of every group against np.longdouble moments of its bit-exact scores within
    rhat_cases.moment_bounds, then rhat_groups_finish against rhat_host of the group within rhat_cases.rhat_bound (as
    tests/test_gpu_rank_rhat.py holds the single form)"""
    from fmcmc_amd import rhat_host
    from fmcmc_amd.summary import rhat_groups_finish
    x, row0, cols, out, zs = groups_case(G, Cm, N)
    nh, m = N // 2, 2 * Cm
    fin = rhat_groups_finish(out, Cm, nh)
    for g in range(G):
        host = rhat_host(np.ascontiguousarray(x[g * Cm:(g + 1) * Cm, :, row0:row0 + N].transpose(0, 2, 1)))
        mom = out[g, :, :4 * m].reshape(NCOLS, 2, m, 2)
        for j in range(NCOLS):
            for fold, name in enumerate(("bulk", "tail")):
                z = zs[g, j, fold].astype(np.longdouble)
                e_mean, e_var = rc.moment_bounds(z)
                mean, var = z.mean(axis=1), z.var(axis=1, ddof=1)
                dm = np.abs(mom[j, fold, :, 0] - mean).astype(np.float64)
                dv = np.abs(mom[j, fold, :, 1] - var).astype(np.float64)
                print("group %d col %d %s: |mean err| %.3g (bound %.3g)  |var err| %.3g (bound %.3g)"
                      % (g, j, name, dm.max(), e_mean.max(), dv.max(), e_var.max()))
                assert (dm <= e_mean).all() and (dv <= e_var).all(), (g, j, name)
                want, have = getattr(host, name)[j], getattr(fin, name)[g, j]
                if var.sum() == 0:                   # the constant column (and a fold that makes one)
                    assert np.isnan(have) and np.isnan(want), (g, j, name)
                    continue
                s_mean, s_var = rc.score_shift_bounds(z)
                tol = rc.rhat_bound(mean, var, e_mean + s_mean, e_var + s_var, nh)
                print("group %d col %d %s: device %.17g host %.17g  |diff| %.3g (bound %.3g)"
                      % (g, j, name, have, want, abs(have - want), tol))
                assert abs(have - want) <= tol, (g, j, name)


# ------------------------------------------------------------------------------------------------ rhat(ans)
def hand_built(x, D, Cm, nrows=None, names=None):
    """an McmcBatch over x [D Cm][k][S] (all S rows kept, labels 1 .. S); nrows [D]: a ragged one, the rows beyond are NaN"""
    import torch
    import fmcmc_amd as f
    x = np.array(x, dtype=np.float64)
    S = x.shape[2]
    if nrows is not None:
        for d, nr in enumerate(nrows):
            x[d * Cm:(d + 1) * Cm, :, nr:] = np.nan
    dc = f.DeviceChains(torch.as_tensor(np.ascontiguousarray(x)).cuda(), None, None, np.arange(1, S + 1), 1, names, 0, D * Cm)
    return f.McmcBatch(dc, D, Cm, nrows=nrows)


def assert_equals_the_loop(ans, got, **kw):
    import fmcmc_amd as f
    assert isinstance(got, f.RhatDiagBatch) and len(got) == len(ans)
    for d in range(len(ans)):
        one = f.rhat(ans[d], **kw)
        for fld in ("bulk", "tail", "rhat", "median"):
            assert _same(getattr(got[d], fld), getattr(one, fld)), (d, fld)
            assert _same(getattr(got, fld)[d], getattr(one, fld)), (d, fld)
        assert (got[d].nchains, got[d].niter, got[d].start, got[d].end) == (one.nchains, one.niter, one.start, one.end), d
        assert got[d].varnames == one.varnames, d


def test_rhat_of_a_hand_built_batch_ragged_and_not():
    import fmcmc_amd as f
    D, Cm = 4, 3
    x, _ = make_inputs(D * Cm, 300, 77, row0=0)
    x = x[:, [0, 1, 3, 5], :301]
    ans = hand_built(x, D, Cm, names=["a", "b", "c", "d"])
    assert not ans.ragged
    assert_equals_the_loop(ans, f.rhat(ans))
    assert_equals_the_loop(ans, ans.rhat(autoburnin=True, cols=[2, 0]), autoburnin=True, cols=[2, 0])
    rag = hand_built(x, D, Cm, nrows=[301, 100, 301, 57])
    assert rag.ragged
    got = f.rhat(rag)
    assert [r.niter for r in got] == [301, 100, 301, 57] and [r.end for r in got] == [301, 100, 301, 57]
    assert_equals_the_loop(rag, got)
    assert_equals_the_loop(rag, rag.rhat(autoburnin=True), autoburnin=True)


def test_a_batch_beyond_the_limit_goes_dataset_by_dataset():
    """one narrow column, 2 datasets x 1 chain: 8194 rows are M = 8194 values, two more than a workgroup sorts; the dataset with
    100 rows of the ragged form still goes through the grouped call"""
    import fmcmc_amd as f
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import rank_groups_fit
    top = abi.lib().fmcmc_rank_groups_max_values()
    N = top + 2
    x = np.random.default_rng(91).standard_normal((2, 1, N)).round(2)
    assert not rank_groups_fit(1, N)
    ans = hand_built(x, 2, 1)
    assert_equals_the_loop(ans, f.rhat(ans))
    assert_equals_the_loop(hand_built(x, 2, 1, nrows=[N, 100]), f.rhat(hand_built(x, 2, 1, nrows=[N, 100])))
    with pytest.raises(NotImplementedError, match="fmcmc_rank_rhat_dev per group"):
        from fmcmc_amd.summary import enqueue_rank_rhat_groups
        enqueue_rank_rhat_groups(ans.history, 2, 1, 0, N, None)


def test_non_finite_values_are_counted_per_group_and_refused_by_name():
    import fmcmc_amd as f
    G, Cm, N = 3, 2, 64
    x, row0 = make_inputs(G * Cm, N, 55)
    x = x.copy()
    x[3, 2, row0 + 5] = np.nan                       # group 1: chain 3, column 2, twice
    x[2, 2, row0 + 40] = np.inf
    x[4, 0, row0 + N // 2 - 1] = -np.inf             # group 2: column 0, once
    x[0, 1, row0 - 1] = np.nan                       # outside the window: not counted
    out, z = groups_raw(x, G, Cm, row0, N, ALL)
    assert out[:, :, 8 * Cm].tolist() == [[0.0] * 6, [0, 0, 2.0, 0, 0, 0], [1.0, 0, 0, 0, 0, 0]]
    for g in range(G):                               # the single form ranks the same bits, NaN and all
        want_out, want_z = single(x, g, Cm, row0, N, ALL)
        assert _same(out[g], want_out) and _same(z[g], want_z), g
    ans = hand_built(x[:, :, row0:row0 + N], G, Cm)
    with pytest.raises(ValueError, match=r"dataset 1: 2 non-finite value\(s\) among the rows to rank \(columns \[2\]\)"):
        f.rhat(ans)
    with pytest.raises(ValueError, match=r"dataset 2: 1 non-finite value\(s\) among the rows to rank \(columns \[0\]\)"):
        f.rhat(ans, cols=[0, 1])
    assert np.isfinite(f.rhat(ans, cols=[1, 3]).bulk).all()


def test_a_column_outside_k_counts_as_non_finite():
    """cols lives on the device: the entry reads nothing for an index outside k, as fmcmc_rank_rhat_dev does"""
    G, Cm, N = 2, 2, 10
    x, row0 = make_inputs(G * Cm, N, 56)
    out, z = groups_raw(x, G, Cm, row0, N, (1, NCOLS, -1))
    for g in range(G):
        want_out, want_z = single(x, g, Cm, row0, N, (1, NCOLS, -1))
        assert _same(out[g], want_out) and _same(z[g], want_z), g
    assert out[:, 1:, 8 * Cm].tolist() == [[20.0, 20.0]] * 2 and (out[:, 0, 8 * Cm] == 0.0).all()


def test_rhat_of_a_small_batch_run():
    """5 datasets x 3 chains, n = 50, 400 steps of MCMC_batch: rhat(ans) against rhat(ans[d]), every field to the bit"""
    import fmcmc_amd as f
    from test_gpu_batch import linreg_data
    Xs, ys, base = linreg_data(5, 50, 3, 5)
    batch = f.model_batch(f.gaussian_linreg(Xs[d], ys[d]) for d in range(5))
    rng = np.random.default_rng(61)
    init = np.asarray(base)[None, None, :] + 0.3 * rng.standard_normal((5, 3, len(base)))
    init[:, :, -1] = np.abs(init[:, :, -1]) + 0.5
    ans = f.MCMC_batch(init, batch, 400, nchains=3, seed=62, kernel=f.kernel_normal(scale=0.1))
    got = f.rhat(ans)
    assert got.bulk.shape == (5, len(base)) and np.isfinite(got.rhat).all()
    assert_equals_the_loop(ans, got)
    assert_equals_the_loop(ans, ans.rhat(autoburnin=True), autoburnin=True)
