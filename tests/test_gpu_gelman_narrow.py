"""GPU tests of the Gelman-Rubin window reduction at 64 columns and fewer (csrc/gelman.hip: gelman_cov_mfma<1..4, true>, one
workgroup per chain) and of gelman_sum_kernel, at their edges.

Yardsticks (tests/gelman_ref.py, proven sane on the host by tests/test_gelman_narrow_host.py):
 * `work` = {xbar - center, S_c} per chain against a two-pass longdouble evaluation, within the a-priori bounds derived there
   from the kernel's order of operations: (N + 32) u sqrt(E_a E_b) for S_c, (N + 16) u sqrt(E_a) + 2 u (|m_a| + |center_a|)
   for xbar.  None of them comes from a measurement;
 * the partial against its definition evaluated in longdouble from the device's own `work`, within (C + 8) u sum_c |term_c|:
   this judges gelman_sum_kernel alone;
 * equalities that need no tolerance: symmetry, placement in the launch, repetition, alignment of the window, independence
   of a column pair from the other columns of the call (also across the two kernels), duplicated columns, what a NaN or an
   Inf reaches;
 * gelman_diag_finish on the device partial against coda::gelman.diag restated in longdouble, 1e-9 as in
   tests/test_gelman_diag_host.py.
Every buffer is filled with NaN before a call and carries GUARD more elements than documented, which must stay NaN.
"""
import numpy as np
import pytest

import gelman_ref as R
from gelman_dev import FIRST_ROW, _bits, _same_bits, device_partial
from test_gelman_diag_host import coda_gelman_ld

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _S(work, p):
    return work[:, p:].reshape(work.shape[0], p, p)


def check_case(x, cols, row0, N, center=FIRST_ROW):
    """The four properties of one call; returns (work, partial, the three ratios)."""
    p = len(cols)
    work, part = device_partial(x, cols, row0, N, center)
    assert not np.isnan(work).any() and not np.isnan(part).any()
    ctr = x[0, cols, row0] if isinstance(center, str) else center
    rx, rS = R.work_ratios(work, x, cols, row0, N, ctr)
    rp = R.partial_ratio(part, work, p)
    assert rx < 1 and rS < 1 and rp < 1, ("p %d N %d row0 %d: ratio xbar %.3g, S %.3g, chain sum %.3g" % (p, N, row0, rx, rS, rp))
    assert part[0] == x.shape[0]
    Sc = _S(work, p)
    assert _same_bits(Sc, Sc.transpose(0, 2, 1))                        # exactly symmetric
    return work, part, (rx, rS, rp)


# ------------------------------------------------------------------------------------------------ 1. shape edges
def _edges(p, rows):
    worst = (0.0, 0.0, 0.0)
    for i, N in enumerate(rows):
        x, cols, row0 = R.edge_input(p, N, i)
        assert x.shape[1] > p and x.shape[2] > row0 + N and (p == 1 or np.any(np.diff(cols) < 0))
        _, _, r = check_case(x, cols, row0, N)
        worst = tuple(max(a, b) for a, b in zip(worst, r))
    print("p = %d, plain: worst ratio xbar %.3f, S %.3f, chain sum %.3f" % ((p,) + worst))


@pytest.mark.parametrize("p", R.FULL_P)
def test_every_row_edge(p):
    """1 to 5 groups of 16 rows (waves with no group), every residue of a wave's group count modulo the three buffers, the
    scalar tail load beside the vector load; row0 in {0, 1, 7}, odd and even row strides, an unsorted column subset."""
    assert {(0, 1, 7)[i % 3] for i in range(len(R.FULL_N))} == {0, 1, 7}
    assert {R.layout(p, N, i)[1] % 2 for i, N in enumerate(R.FULL_N)} == {0, 1}
    _edges(p, R.FULL_N)


@pytest.mark.parametrize("p", R.SHORT_P)
def test_every_column_edge(p):
    _edges(p, R.SHORT_N)


# ------------------------------------------------------------------------------------------------ 2. conditioning
@pytest.mark.parametrize("family", R.FAMILIES)
def test_every_input_family(family):
    worst = (0.0, 0.0, 0.0)
    for i, (p, N) in enumerate((p, N) for p in R.COND_P for N in R.COND_N):
        x, cols, row0 = R.edge_input(p, N, i, Cn=3, family=family)
        work, _, r = check_case(x, cols, row0, N)
        worst = tuple(max(a, b) for a, b in zip(worst, r))
        if family == "constant":
            j = p // 2
            Sc = _S(work, p)
            assert not _bits(Sc[:, j, :]).any() and not _bits(Sc[:, :, j]).any()         # +0.0 to the bit
            assert _same_bits(work[:, j], np.array([R.constant_value(c) for c in range(3)]) - x[0, cols[j], row0])
    print("%s: worst ratio xbar %.3f, S %.3f, chain sum %.3f" % ((family,) + worst))


# ------------------------------------------------------------------------------------------------ 3. chains
@pytest.mark.parametrize("Cn", [1, 2, 3, 4, 5, 8, 9])
def test_the_chain_sum_at_every_split_of_the_chains(Cn):
    x, cols, row0 = R.edge_input(17, 65, 2, Cn=Cn)
    _, _, r = check_case(x, cols, row0, 65)
    print("chains %d: chain sum ratio %.3f" % (Cn, r[2]))


def test_partials_of_two_shards_add():
    """What the all-reduce relies on: five chains as 2 + 3 with one center."""
    p, N = 17, 65
    x, cols, row0 = R.edge_input(p, N, 2, Cn=5)
    ctr = x[0, cols, row0].copy()
    w5, p5 = device_partial(x, cols, row0, N, ctr)
    wa, pa = device_partial(x[:2], cols, row0, N, ctr)
    wb, pb = device_partial(x[2:], cols, row0, N, ctr)
    assert _same_bits(np.concatenate([wa, wb]), w5)
    added = pa + pb
    assert added[0] == 5 and pa[0] == 2 and pb[0] == 3
    r = R.partial_ratio(added, w5, p)
    print("2 + 3 chains: the added partials at %.3f of the joint chain-sum bound" % r)
    assert r < 1


# ------------------------------------------------------------------------------------------------ 4. null center
@pytest.mark.parametrize("p", [5, 20, 40, 64])
def test_a_null_center_gives_the_uncentred_mean(p):
    x, cols, row0 = R.edge_input(p, 65, 1)
    work, _, r = check_case(x, cols, row0, 65, center=None)
    assert np.all(np.abs(work[:, :p] - 3.0) < 2.0)                      # (the data sit around 3: nothing was subtracted)
    print("p = %d, null center: worst ratio xbar %.3f, S %.3f, chain sum %.3f" % ((p,) + r))


# ------------------------------------------------------------------------------------------------ 5. equalities
@pytest.mark.parametrize("p,N", [(17, 65), (64, 33), (1, 5)])
def test_a_chain_does_not_depend_on_the_launch(p, N):
    x, cols, row0 = R.edge_input(p, N, 1, Cn=5)
    ctr = x[0, cols, row0].copy()
    w5, p5 = device_partial(x, cols, row0, N, ctr)
    w5b, p5b = device_partial(x, cols, row0, N, ctr)
    assert _same_bits(w5, w5b) and _same_bits(p5, p5b)                                  # two calls
    wr, _ = device_partial(x[::-1], cols, row0, N, ctr)                                 # the batch reversed
    assert _same_bits(wr[::-1], w5)
    for c in (0, 2, 4):                                                                 # alone
        w1, _ = device_partial(x[c:c + 1], cols, row0, N, ctr)
        assert _same_bits(w1[0], w5[c])


@pytest.mark.parametrize("p,N,row0", [(17, 65, 1), (64, 130, 7), (5, 19, 3)])
def test_a_window_of_a_long_history_equals_its_rows_uploaded_alone(p, N, row0):
    """row0 odd in a history with an odd row stride: the pair loads are 8-byte aligned only; the same rows as a tensor of
    their own (S = N, row0 = 0, even stride where N is even) are loaded 16-byte aligned."""
    k, S = p + 2, row0 + N + 10
    S += 1 - S % 2
    x = R.make_chains(3, k, S, 31 * p + N)
    cols = np.random.default_rng(p).permutation(k)[:p].astype(np.int32)
    ctr = x[0, cols, row0].copy()
    wl, pl = device_partial(x, cols, row0, N, ctr)
    ws, ps = device_partial(np.ascontiguousarray(x[:, :, row0:row0 + N]), cols, 0, N, ctr)
    assert _same_bits(wl, ws) and _same_bits(pl, ps)


def test_a_pair_of_columns_does_not_depend_on_the_other_columns():
    """xbar[a] and S_c[a, b] of a call with cols = [a, b] carry the bits of the p = 64 call, of a p = 17 call that holds a and b
    at other positions (b before a) and of a p = 200 call on four super-blocks: the row-to-lane and row-to-wave assignment
    depends on N alone, every product and the dbar_a dbar_b correction commute, nothing of another column enters an element."""
    k, N, row0 = 256, 81, 3
    x = R.make_chains(3, k, row0 + N + 4, 99)
    ctr_all = x[0, :, row0].copy()
    rng = np.random.default_rng(4)
    c64 = rng.permutation(64)[:64].astype(np.int32)
    a, b = int(c64[5]), int(c64[41])                                    # different column blocks of the p = 64 call
    c17 = np.concatenate([[b], rng.permutation(np.setdiff1d(np.arange(k), [a, b]))[:15], [a]]).astype(np.int32)
    c17[[0, 3]] = c17[[3, 0]]                                           # b at position 3, a at position 16 (the second block)
    c200 = np.concatenate([rng.permutation(np.setdiff1d(np.arange(k), [a, b]))[:198], [a, b]]).astype(np.int32)
    c200[[70, 198]] = c200[[198, 70]]                                   # a in the second super-block,
    c200[[3, 199]] = c200[[199, 3]]                                     # b in the first: the off-diagonal pair holds (b, a)
    w2, _ = device_partial(x, [a, b], row0, N, ctr_all[[a, b]])
    S2 = _S(w2, 2)
    for cols in (c64, c17, c200):
        p = len(cols)
        ia, ib = int(np.where(cols == a)[0][0]), int(np.where(cols == b)[0][0])
        w, _ = device_partial(x, cols, row0, N, ctr_all[cols])
        Sc = _S(w, p)
        assert _same_bits(w[:, ia], w2[:, 0]) and _same_bits(w[:, ib], w2[:, 1]), p
        assert _same_bits(Sc[:, ia, ib], S2[:, 0, 1]) and _same_bits(Sc[:, ib, ia], S2[:, 0, 1]), p
        assert _same_bits(Sc[:, ia, ia], S2[:, 0, 0]) and _same_bits(Sc[:, ib, ib], S2[:, 1, 1]), p


def test_a_repeated_column():
    """cols = [3, 3, 0]: the covariance of the column with its duplicate carries the variance's bits."""
    N, row0 = 49, 1
    x = R.make_chains(2, 4, row0 + N + 2, 8)
    work, part = device_partial(x, [3, 3, 0], row0, N)
    Sc = _S(work, 3)
    assert _same_bits(Sc[:, 0, 1], Sc[:, 0, 0]) and _same_bits(Sc[:, 1, 1], Sc[:, 0, 0]) and _same_bits(Sc[:, 1, 0], Sc[:, 0, 0])
    assert _same_bits(Sc[:, 0, 2], Sc[:, 1, 2]) and _same_bits(work[:, 0], work[:, 1])
    rx, rS = R.work_ratios(work, x, [3, 3, 0], row0, N, x[0, [3, 3, 0], row0])
    assert rx < 1 and rS < 1 and R.partial_ratio(part, work, 3) < 1


# ------------------------------------------------------------------------------------------------ 6. non-finite data
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("p,jpos", [(17, 9), (17, 0), (40, 33)])
def test_a_non_finite_value_reaches_its_own_column_only(bad, p, jpos):
    """One NaN / +Inf in column cols[jpos] of chain 1 reaches row and column jpos of that chain's S_c, its xbar[jpos] and the
    partial elements they feed; every other element has the bits of the clean run.  jpos = 0 is the column the padded
    lanes read (and multiply by 0, which a NaN survives: their products must stay out of the live elements)."""
    N, c = 65, 1
    x, cols, row0 = R.edge_input(p, N, 2, Cn=3)
    w0, p0 = device_partial(x, cols, row0, N)
    xb = x.copy()
    xb[c, cols[jpos], row0 + 37] = bad
    w1, p1 = device_partial(xb, cols, row0, N, x[0, cols, row0])
    hit_w = np.zeros((3, p + p * p), dtype=bool)
    S_hit = np.zeros((p, p), dtype=bool)
    S_hit[jpos, :] = S_hit[:, jpos] = True
    hit_w[c, jpos] = True
    hit_w[c, p:] = S_hit.ravel()
    one = np.zeros(p, dtype=bool)
    one[jpos] = True
    hit_p = np.concatenate([[False], one, S_hit.ravel(), S_hit.ravel(), one, one, one, one])
    assert np.array_equal(_bits(w1)[~hit_w], _bits(w0)[~hit_w])
    assert np.array_equal(_bits(p1)[~hit_p], _bits(p0)[~hit_p])
    assert not np.isfinite(w1[hit_w]).any() and not np.isfinite(p1[hit_p]).any()
    assert np.isfinite(w0).all() and np.isfinite(p0).all()


# ------------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("m,p,N", R.E2E)
def test_gelman_diag_finish_on_the_device_partial(O, m, p, N):
    from fmcmc_amd.summary import gelman_diag_finish
    x, cols, row0 = R.e2e_input(m, p, N)
    _, part, _ = check_case(x, cols, row0, N)
    g = gelman_diag_finish(part, p, N)
    win = x[:, cols, row0:row0 + N].transpose(0, 2, 1)
    est, upper = coda_gelman_ld(win)
    e_est, e_up = np.abs(g.psrf[:, 0] / est - 1).max(), np.abs(g.psrf[:, 1] / upper - 1).max()
    print("m=%d p=%d N=%d: point est. %.2e, upper %.2e of coda in longdouble" % (m, p, N, e_est, e_up))
    assert e_est < 1e-9 and e_up < 1e-9
    if p == 1:
        assert g.mpsrf is None
    else:
        _, ompsrf = O.gelman(np.ascontiguousarray(win))
        print("mpsrf %.2e of the oracle" % abs(g.mpsrf / ompsrf - 1))
        assert abs(g.mpsrf - ompsrf) < 1e-9 * ompsrf
