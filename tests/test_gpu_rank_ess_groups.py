"""The grouped rank-normalised effective sample size on the GPU (fmcmc_rank_ess_groups_dev, csrc/diag_ess_groups.hpp: one
workgroup per (group, column) from the sort to the cut).  Every group's row of `out` is held bit for bit, NaN prefill included,
to fmcmc_rank_ess_dev on that group alone (tests/test_gpu_rank_ess.py: raw, parts); one shape also to the host's longdouble
sums and ess_host under the bounds of tests/ess_cases.py, which come from the order of the sums and never from a kernel's output.
The raw entry is called with NaN-filled buffers GUARD elements longer than documented, which must stay NaN."""
import functools
import os
import re

import numpy as np
import pytest

import ess_cases as ec
from gelman_dev import GUARD
from test_gpu_rank_ess import _bits, parts, raw, split

pytestmark = pytest.mark.gpu

ALL = tuple(range(ec.NCOLS))
T, FRONT, LAGS, TOP = 2048, 16, 256, 8192            # EA_T, EA_FRONT, EA_LAGS (csrc/diag_ess.hpp), RG_MAX_VALUES


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ the raw call
def groups_raw(x, G, Cm, row0, N, cols, active=None, stream=None, stage=None, keep=None):
    """L.fmcmc_rank_ess_groups_dev on x [G Cm][k][S]: work and out NaN-filled and GUARD longer than documented ->
    out [G][p][4 (4 Cm + 2 + N // 2 - 2) + 7]; the scores of a masked group in work must still be NaN, those of the others
    written.  stream / stage as tests/test_gpu_rank_rhat.py: raw has them; keep: a list that receives the device input."""
    import torch
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    Cn, k, S = x.shape
    assert Cn == G * Cm
    p, n = len(cols), N // 2
    M, width = 2 * Cm * n, 4 * (4 * Cm + 2 + n - 2) + 7
    lens = [L.fmcmc_rank_ess_groups_work_len(G, Cm, p, N), L.fmcmc_rank_ess_groups_out_len(G, Cm, p, N)]
    assert lens == [G * p * M, G * p * width]
    nan = lambda cnt: torch.full((int(cnt) + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    bufs = [nan(cnt) for cnt in lens]
    cd = torch.as_tensor(np.asarray(cols, dtype=np.int32)).cuda()
    ad = None if active is None else torch.as_tensor(np.asarray(active, dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    xd = torch.as_tensor(x).cuda() if stage is None else stage()
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        if stage is not None:
            xd.copy_(torch.as_tensor(x).pin_memory(), non_blocking=True)
        rcode = L.fmcmc_rank_ess_groups_dev(xd.data_ptr(), G, Cm, k, S, row0, N, cd.data_ptr(), p,
                                            None if ad is None else ad.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                                            st.cuda_stream)
    assert rcode == abi.OK, (rcode, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    assert all(np.isnan(h[int(cnt):]).all() for h, cnt in zip(host, lens))      # nothing past the documented lengths
    if active is not None:
        z = host[0][:lens[0]].reshape(G, -1)
        assert all(np.isnan(z[g]).all() for g in range(G) if not active[g])       # a masked group writes no scores either
    if keep is not None:
        keep.append(xd.cpu().numpy())
    return host[1][:lens[1]].reshape(G, p, width)


def single(x, g, Cm, row0, N, cols):
    """the single form on group g alone: out [p][.]"""
    return raw(np.ascontiguousarray(x[g * Cm:(g + 1) * Cm]), row0, N, cols)


# (ngroups, cpg, N).  n = 4 (cap 2); odd N; the smallest group of two chains; (2, 3, 39 / 40): n = 19, 20 around a 16-row operand;
# cap = 255, 256, 257 around one lag block; cap = 511, 513 around the second round's end; n + 16 = T - 1, T, T + 1 around the
# tile of rows; M at the limit (three tiles of rows at n = 4096); the workload's group, padded to P = 8192; (5, 3, 400); more
# workgroups than CUs.  make_inputs gives row0 = 3 and an odd S throughout.
SHAPES = [(1, 1, 8), (3, 1, 9), (2, 2, 8), (2, 3, 39), (2, 3, 40), (2, 1, 514), (2, 1, 516), (2, 1, 518), (2, 1, 1026),
          (2, 1, 1030), (2, 1, 4062), (2, 1, 4064), (2, 1, 4066), (2, 2, 4096), (2, 1, 8192), (2, 4, 2000), (5, 3, 400),
          (300, 1, 16)]


def test_the_shapes_are_the_edges_they_claim():
    from fmcmc_amd import _abi as abi
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fmcmc_amd", "csrc")
    ess, grp = open(os.path.join(csrc, "diag_ess.hpp")).read(), open(os.path.join(csrc, "diag_ess_groups.hpp")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, ess).group(1))
    assert (const("EA_T"), const("EA_FRONT"), const("EA_LAGS")) == (T, FRONT, LAGS)
    assert abi.lib().fmcmc_rank_groups_max_values() == TOP
    assert "T1 < 512u ? 512u" in ess and "cap < 256u ? cap : 256u" in grp and "ess_next_round(T1, cap)" in grp
    n = [N // 2 for _g, _c, N in SHAPES]
    caps = {v - 2 for v in n}
    assert {2, LAGS - 1, LAGS, LAGS + 1, 2 * LAGS - 1, 2 * LAGS + 1} <= caps and min(n) == 4
    assert {T - 1, T, T + 1} <= {v + FRONT for v in n}
    M = [2 * c * (N // 2) for _g, c, N in SHAPES]
    assert max(M) == TOP and M.count(TOP) == 2 and 8000 in M and (2, 4, 2000) in SHAPES
    assert any(N % 2 for _g, _c, N in SHAPES) and max(g for g, _c, _n in SHAPES) > 256
    assert -(-(4096 + FRONT - 15) // T) == 3                                     # n = 4096: three tiles of rows at lag block 0


@functools.lru_cache(maxsize=None)
def groups_case(G, Cm, N):
    cols = (0, 3) if G == 300 else ALL
    x, row0 = ec.make_inputs(G * Cm, N, 1000 * G + 100 * Cm + N)
    out = groups_raw(x, G, Cm, row0, N, cols)
    out.setflags(write=False)
    return x, row0, cols, out


@pytest.mark.parametrize("G, Cm, N", SHAPES)
def test_every_group_bit_for_bit_the_single_form(G, Cm, N):
    x, row0, cols, out = groups_case(G, Cm, N)
    n = N // 2
    for g in range(G):
        want = single(x, g, Cm, row0, N, cols)
        assert _same(out[g], want), (g, np.nonzero(_bits(out[g]) != _bits(want)))
    for kinds, info in parts(out[0], Cm, N):                                     # (and S(t) is written below L only)
        assert info[0] == 0.0 and all(L >= min(LAGS, n - 2) and K >= 1 for _mu, _var, L, K, _S in kinds)


def test_one_shape_against_the_host():
    """(5, 3, 400), groups 0 and 4: the means and every S(t) against np.longdouble under ess_cases' bounds, the tail quantiles
    to the bit, and ess_groups_finish against ess_host within ess_cases.ess_bound with the same cut"""
    from fmcmc_amd import ess_host
    from fmcmc_amd.summary import ess_groups_finish
    G, Cm, N = 5, 3, 400
    x, row0, cols, out = groups_case(G, Cm, N)
    fin = ess_groups_finish(out, Cm, N)
    names = ("bulk", "tail_q05", "tail_q95", "mean")
    for g in (0, 4):
        xg = x[g * Cm:(g + 1) * Cm]
        dev = parts(out[g], Cm, N)
        host = ess_host(ec.window(xg, row0, N))
        for j in (0, 1, 3):
            series, q = ec.series_of(split(xg, row0, N, j))
            assert _bits(dev[j][1][1]) == _bits(q[0]) and _bits(dev[j][1][2]) == _bits(q[1])
            for kind, name in enumerate(names):
                mean, var, L, K, S = dev[j][0][kind]
                r = ec.host_case(series[kind], kind, L=L)
                err = np.abs(S - r.S).astype(np.float64)
                assert (np.abs(mean - r.mu) <= r.e_mean).all() and (err <= r.ES).all(), (g, j, kind)
                have, want = getattr(fin, name)[g, j], getattr(host, name)[j]
                if np.isnan(want):
                    assert np.isnan(have)
                    continue
                print("group %d col %d %s: device %.17g host %.17g |diff| %.3g (bound %.3g) gap %.3g K %d"
                      % (g, j, name, have, want, abs(have - want), r.bound, r.gap, r.g.K))
                assert r.gap > 0.0 and fin.lags[g, j, kind] == host.lags[j, kind] == K == r.g.K
                assert abs(have - want) <= r.bound, (g, j, name)
        assert np.isnan(fin.bulk[g, 2]) and np.isnan(fin.mcse_mean[g, 2])          # the constant column


# ------------------------------------------------------------------------------------------------ the cut, group by group
def _mixed():
    """4 groups x 2 chains x 1200 rows, one column: AR(1), a ramp (every round to the cap), an alternating series (cut at the
    first pair), iid: the workgroups leave the loop over the rounds after different numbers of trips"""
    Cm, N, row0 = 2, 1200, 3
    rng = np.random.default_rng(17)
    series = [ec.ar1(rng, 0.6, Cm, N), ec.ramp(Cm, N, 61), ec.alternating(Cm, N, 2), rng.standard_normal((Cm, N))]
    S = row0 + N + 2
    S += 1 - S % 2
    x = np.full((4 * Cm, 1, S), 1e9)
    for g, v in enumerate(series):
        x[g * Cm:(g + 1) * Cm, 0, row0:row0 + N] = v
    return x, Cm, row0, N


def test_groups_that_leave_the_rounds_at_different_trips():
    x, Cm, row0, N = _mixed()
    out = groups_raw(x, 4, Cm, row0, N, (0,))
    cap = N // 2 - 2
    got = [parts(out[g], Cm, N)[0][0] for g in range(4)]
    for g in range(4):
        assert _same(out[g], single(x, g, Cm, row0, N, (0,))), g
    for kind in (0, 3):
        assert got[1][kind][2] == cap and got[1][kind][3] == cap // 2               # the ramp: L, K at the cap
        assert got[2][kind][2] == LAGS and got[2][kind][3] == 1                     # alternating: one round, K = 1
        assert got[0][kind][2] == LAGS and 1 < got[0][kind][3] < LAGS // 2 and got[3][kind][2] == LAGS
    # each of the two alone in a call of its own: the same row again
    for g in (1, 2):
        alone = groups_raw(np.ascontiguousarray(x[g * Cm:(g + 1) * Cm]), 1, Cm, row0, N, (0,))
        assert _same(alone[0], out[g]), g


# ------------------------------------------------------------------------------------------------ active
def test_inactive_groups_keep_their_prefill():
    G, Cm, N = 5, 3, 400
    x, row0, cols, out = groups_case(G, Cm, N)
    mask = [1, 0, 1, 1, 0]
    mo = groups_raw(x, G, Cm, row0, N, cols, active=mask)
    for g, on in enumerate(mask):
        assert _same(mo[g], out[g]) if on else np.isnan(mo[g]).all(), g
    assert _same(groups_raw(x, G, Cm, row0, N, cols, active=[1] * G), out)
    assert np.isnan(groups_raw(x, G, Cm, row0, N, cols, active=[0] * G)).all()


# ------------------------------------------------------------------------------------------------ independence of the launch
def test_two_launches_agree_and_the_samples_are_not_written():
    G, Cm, N = 2, 3, 40
    x, row0, cols, out = groups_case(G, Cm, N)
    keep = []
    again = groups_raw(x, G, Cm, row0, N, cols, keep=keep)
    assert _same(again, out) and _same(keep[0], x)


def test_a_group_elsewhere_in_a_larger_call():
    G, Cm, N = 5, 3, 400
    x, row0, cols, out = groups_case(G, Cm, N)
    other, _ = ec.make_inputs(4 * Cm, N, 4242)
    y = np.ascontiguousarray(np.concatenate([other[:2 * Cm], x[3 * Cm:4 * Cm], other[2 * Cm:], x[:Cm]]))
    yo = groups_raw(y, 6, Cm, row0, N, cols)
    assert _same(yo[2], out[3]) and _same(yo[5], out[0])


def test_a_column_alone_and_among_three_in_another_order():
    G, Cm, N = 5, 3, 400
    x, row0, cols, out = groups_case(G, Cm, N)
    three = groups_raw(x, G, Cm, row0, N, (3, 0, 1))
    for j, col in enumerate((3, 0, 1)):
        alone = groups_raw(x, G, Cm, row0, N, (col,))
        assert _same(alone[:, 0], three[:, j]) and _same(alone[:, 0], out[:, col]), col


def test_a_side_stream_behind_a_busy_stream():
    """the rows reach the device ON the side stream, behind a kernel that keeps it busy: a call that left its caller's stream
    would read the NaN prefill"""
    import torch
    G, Cm, N = 5, 3, 400
    x, row0, cols, out = groups_case(G, Cm, N)
    side = torch.cuda.Stream()

    def stage():
        xd = torch.full(x.shape, float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(4_000_000)             # a few milliseconds
        return xd

    assert _same(groups_raw(x, G, Cm, row0, N, cols, stream=side, stage=stage), out)


# ------------------------------------------------------------------------------------------------ odd values, refusals
def test_non_finite_values_and_negative_zero_as_the_single_form_has_them():
    import fmcmc_amd as f
    from test_gpu_rank_groups import hand_built
    G, Cm, N = 3, 2, 64
    x, row0 = ec.make_inputs(G * Cm, N, 55)
    x = x.copy()
    x[3, 2, row0 + 5] = np.nan                       # group 1: chain 3, column 2, twice
    x[2, 2, row0 + 40] = np.inf
    x[4, 0, row0 + N // 2 - 1] = -np.inf             # group 2: column 0, once
    x[0, 1, row0 - 1] = np.nan                       # outside the window: not counted
    x[0, 1, row0:row0 + N][x[0, 1, row0:row0 + N] == 0.0] = -0.0                  # group 0: -0.0 among the ties, read as +0.0
    assert np.signbit(x[0, 1, row0:row0 + N]).any() and (x[1, 1, row0:row0 + N] == 0.0).any()
    out = groups_raw(x, G, Cm, row0, N, ALL)
    assert out[:, :, -7].tolist() == [[0.0] * 4, [0, 0, 2.0, 0], [1.0, 0, 0, 0]]
    for g in range(G):                               # the single form works on the same bits, NaN keys and all
        assert _same(out[g], single(x, g, Cm, row0, N, ALL)), g
    ans = hand_built(x[:, :, row0:row0 + N], G, Cm)
    with pytest.raises(ValueError, match=r"dataset 1: 2 non-finite value\(s\) among the rows to rank \(columns \[2\]\)"):
        f.ess(ans)
    with pytest.raises(ValueError, match=r"dataset 2: 1 non-finite value\(s\) among the rows to rank \(columns \[0\]\)"):
        f.ess(ans, cols=[0, 1])
    assert np.isfinite(f.ess(ans, cols=[1, 3]).bulk).all()


def test_a_column_outside_k_counts_as_non_finite():
    """cols lives on the device: the entry reads nothing for an index outside k, as fmcmc_rank_ess_dev does"""
    G, Cm, N = 2, 2, 10
    x, row0 = ec.make_inputs(G * Cm, N, 56)
    out = groups_raw(x, G, Cm, row0, N, (1, ec.NCOLS, -1))
    for g in range(G):
        assert _same(out[g], single(x, g, Cm, row0, N, (1, ec.NCOLS, -1))), g
    assert out[:, 1:, -7].tolist() == [[20.0, 20.0]] * 2 and (out[:, 0, -7] == 0.0).all()


def test_refusals_launch_nothing():
    import torch
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    S = TOP + 8
    x = torch.zeros((2, 1, S), dtype=torch.float64, device="cuda")
    cols = torch.zeros(1, dtype=torch.int32, device="cuda")
    buf = torch.full((1 << 16,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = lambda N, G=2, Cm=1, **kw: [kw.get("x", x.data_ptr()), G, Cm, 1, S, 0, N, kw.get("cols", cols.data_ptr()), 1, None,
                                       kw.get("work", buf.data_ptr()), kw.get("out", buf.data_ptr()), st]
    assert L.fmcmc_rank_ess_groups_dev(*args(TOP + 2)) == abi.ERR_UNSUPPORTED
    assert "fmcmc_rank_ess_dev per group is the form for larger groups" in abi.last_error() and "8194 values" in abi.last_error()
    assert L.fmcmc_rank_ess_groups_work_len(2, 1, 1, TOP + 2) == 0 and L.fmcmc_rank_ess_groups_out_len(2, 1, 1, TOP + 2) == 0
    assert L.fmcmc_rank_ess_groups_dev(*args(7)) == abi.ERR_ARG and "shorter than 8 rows" in abi.last_error()
    for name in ("x", "cols", "work", "out"):
        assert L.fmcmc_rank_ess_groups_dev(*args(8, **{name: None})) == abi.ERR_ARG and "null argument" in abi.last_error(), name
    assert L.fmcmc_rank_ess_groups_dev(*args(8, G=0)) == abi.ERR_ARG and "each must be at least 1" in abi.last_error()
    assert L.fmcmc_rank_ess_groups_dev(*args(8, Cm=0)) == abi.ERR_ARG
    assert L.fmcmc_rank_ess_groups_dev(*args(S + 1)) == abi.ERR_ARG and "outside" in abi.last_error()
    assert L.fmcmc_rank_ess_groups_dev(*args(8, G=2 ** 31)) == abi.ERR_UNSUPPORTED and "exceed one launch" in abi.last_error()
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()                    # nothing was launched
    from fmcmc_amd.summary import enqueue_rank_ess_groups
    from test_gpu_rank_groups import hand_built
    ans = hand_built(np.random.default_rng(3).standard_normal((2, 1, TOP + 2)), 2, 1)
    with pytest.raises(NotImplementedError, match="fmcmc_rank_ess_dev per group"):
        enqueue_rank_ess_groups(ans.history, 2, 1, 0, TOP + 2, None)
    with pytest.raises(ValueError, match="at least eight"):
        enqueue_rank_ess_groups(ans.history, 2, 1, 0, 7, None)
    with pytest.raises(ValueError, match="are not the 2 chains"):
        enqueue_rank_ess_groups(ans.history, 3, 1, 0, 8, None)
