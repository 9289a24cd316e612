"""References, a-priori bounds and inputs for the tests of the Gelman-Rubin window reduction (csrc/gelman.hip).  A plain module:
tests/test_gelman_narrow_host.py (no GPU) proves the bounds and the inputs sane, tests/test_gpu_gelman_narrow.py and
tests/test_gpu_gelman_wide.py hold the device to them.

The yardstick is np.longdouble (64-bit significand), not float64 numpy: on data offset by 1e8 np.cov / np.mean miss the bounds
below several times over while the kernel's own order of operations stays inside them (test_gelman_narrow_host).

The bounds, with u = 2^-53, m_a the window mean and S_ab the ddof-1 covariance (both in longdouble), Delta_a = x[row0, a] - m_a
and E_a = S_aa + N / (N - 1) Delta_a^2:

    |S_dev[a, b] - S_ab|                  <= (N + 32) u sqrt(E_a E_b)
    |xbar_dev[a] - (m_a - center_a)|      <= (N + 16) u sqrt(E_a) + 2 u (|m_a| + |center_a|)

Derivation (first order in u; the kernel is gelman_cov_mfma, the same arithmetic at every width).  The kernel shifts
by the window's FIRST ROW, d_t = x_t - x_row0, forms sum_t d_a d_b and sum_t d_a in one pass and finishes as
(sum d_a d_b - sum d_a sum d_b / N) / (N - 1) and (x_row0 + sum d_a / N) - center.
 * The shift is a row of the window, so sum_t d_a^2 = sum_t (x_t - m_a)^2 + N Delta_a^2 = (N - 1) E_a exactly, and by
   Cauchy-Schwarz sum_t |d_a d_b| <= (N - 1) sqrt(E_a E_b) and (sum_t |d_a|)(sum_t |d_b|) / N <= (N - 1) sqrt(E_a E_b).
   Every error below is relative to one of these two sums; the final division by N - 1 turns them into sqrt(E_a E_b).
 * d = x - shift is rounded once: 2 u on a product, u on a column sum.
 * A column sum is a recursive sum over one lane class (every fourth group of four rows) of one wave's quarter of the
   window, at most min(N, N / 16 + 4) terms, then two shuffle additions and three wave joins: at most
   (min(N - 1, N / 16 + 3) + 5) u.
 * A product accumulator takes FOUR products per matrix instruction (the four lane classes), so it is a recursive sum over
   the wave's whole quarter: at most min(N, N / 4 + 16) products (rows past the window add an exact 0), then three wave joins:
   (min(N - 1, N / 4 + 15) + 3) u, and u more where the product is rounded before it is added.
 * The correction sum d_a sum d_b / N carries both column-sum errors, the rounded d of both, a product and a division:
   (2 min(N - 1, N / 16 + 3) + 14) u; the subtraction and the division by N - 1 add 2 u of the result.
 * Together: (2 + 1 + min(N - 1, N / 4 + 15) + 3 + 2 min(N - 1, N / 16 + 3) + 14 + 2) u, which is 25 u at N = 2,
   (N + 21 + 2 min(N - 1, N / 16 + 3)) u up to N = 21 and (3 N / 8 + 43) u beyond: below (N + 32) u for every N >= 2
   (closest at N = 21: 50.6 against 53).
 * The mean: the column sum's (N / 16 + 8) u and the rounding of d, times sum |d_a| / N <= sqrt(E_a); a division (u sqrt(E_a));
   the addition of the shift (u |m_a|) and the subtraction of center (u |m_a - center_a|): (N / 16 + 10) u sqrt(E_a) +
   2 u |m_a| + u |center_a|, below the bound.
The reference's own error is a two-pass longdouble evaluation at u_ld = 2^-64: 2^-11 of every bound.

The chain sum (gelman_sum_kernel) is judged ALONE, from the device's own `work` rows: every element of the partial but the
first is a sum over the C local chains of a term of at most two rounded products (s2 xbar^2), four threads each summing every
fourth chain and three joins: at most (C / 4 + 3 + 2) u sum_c |term_c| <= (C + 8) u sum_c |term_c|.  Element 0 is C exactly.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

FAMILIES = ("plain", "offset", "jump", "trend", "scales", "constant")
FULL_P, FULL_N = (1, 16, 17, 33, 64), (2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 191, 192, 193,
                                       1000, 1001)
SHORT_P, SHORT_N = (2, 15, 31, 32, 47, 48, 49, 63), (2, 17, 65)
COND_P, COND_N = (3, 17, 64), (17, 193, 1001)
E2E = ((2, 1, 17), (3, 2, 65), (3, 17, 193), (4, 64, 333))        # (chains, p, N) of the end-to-end check


def _check_longdouble():
    assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit significand here: no yardstick"


# ------------------------------------------------------------------------------------------------ inputs
def make_chains(Cn, k, S, seed):
    """[C][k][S]: noise, an offset per chain and column, a slow random walk (as in tests/gelman_dev.py)."""
    rng = np.random.default_rng(seed)
    return (0.5 * rng.standard_normal((Cn, k, S)) + 0.2 * rng.standard_normal((Cn, k, 1)) + 3.0
            + 0.01 * np.cumsum(rng.standard_normal((Cn, k, S)), axis=2))


def constant_value(c):
    return 2.718281828459045 + 0.125 * c


def make_family(name, Cn, k, S, seed, row0=0, N=None, const_col=0):
    """[C][k][S] of one input family, deterministic per seed.  `jump` and `trend` refer to the window [row0, row0 + N);
    `constant` makes column const_col of chain c the value constant_value(c) in every row."""
    N = S - row0 if N is None else N
    x = make_chains(Cn, k, S, seed)
    if name == "plain":
        pass
    elif name == "offset":
        x = x + 1e8
    elif name == "jump":
        x[:, :, row0] += 1e4
    elif name == "trend":
        x = x + 5.0 * (np.arange(S) - row0) / max(N - 1, 1)
    elif name == "scales":
        # -60, 60, -60 + step, 60 - step, ...: neighbours far apart; s2^2 and s2 xbar^2 stay within 1e-241 .. 1e242
        e = np.linspace(-60.0, 60.0, k) if k > 1 else np.array([60.0])
        order = np.empty(k, dtype=int)
        order[0::2] = np.arange((k + 1) // 2)
        order[1::2] = k - 1 - np.arange(k // 2)
        x = x * (10.0 ** np.round(e[order]))[None, :, None]
    elif name == "constant":
        for c in range(Cn):
            x[c, const_col, :] = constant_value(c)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(x)


def layout(p, N, i):
    """(k, S, row0, cols) of the i-th case: row0 in {0, 1, 7}, the row stride odd and even in turn and larger than the window,
    k > p, cols an unsorted permutation of a subset of the k columns."""
    row0 = (0, 1, 7)[i % 3]
    S = row0 + N + 3
    S += (S + i // 3) % 2                       # parity alternates with i // 3, so every row0 meets both
    k = p + 3
    cols = np.random.default_rng(100 * p + i).permutation(k)[:p].astype(np.int32)
    if p > 1 and np.all(np.diff(cols) > 0):
        cols = cols[::-1].copy()
    return k, S, row0, cols


def edge_cases():
    """(p, N, i) of the shape-edge tests, i numbering the cases of one p."""
    for p in FULL_P:
        for i, N in enumerate(FULL_N):
            yield p, N, i
    for p in SHORT_P:
        for i, N in enumerate(SHORT_N):
            yield p, N, i


def edge_input(p, N, i, Cn=2, family="plain"):
    """x [C][k][S], cols, row0 of one shape-edge or conditioning case (the constant column is the middle one of cols)."""
    k, S, row0, cols = layout(p, N, i)
    x = make_family(family, Cn, k, S, 7000 * p + N, row0, N, const_col=int(cols[p // 2]))
    return x, cols, row0


def e2e_input(m, p, N):
    """The end-to-end inputs: `plain`, x [m][k][S], cols, row0."""
    return edge_input(p, N, m, Cn=m)


# ------------------------------------------------------------------------------------------------ the window reduction
def _moments(x, cols, row0, N):
    _check_longdouble()
    w = np.asarray(x)[:, np.asarray(cols), row0:row0 + N].astype(LD)            # [C][p][N]
    m = w.sum(2) / LD(N)
    r = w - m[:, :, None]
    m = m + r.sum(2) / LD(N)                                                    # (second pass of the mean)
    r = w - m[:, :, None]
    S = np.matmul(r, r.transpose(0, 2, 1)) / LD(N - 1)
    return w, m, S


def longdouble_work(x, cols, row0, N, center):
    """Per chain the two-pass window mean minus `center` (None: 0) [C][p] and the ddof-1 covariance [C][p][p], longdouble."""
    w, m, S = _moments(x, cols, row0, N)
    return m - (LD(0) if center is None else np.asarray(center).astype(LD)), S


def work_bounds(x, cols, row0, N, center):
    """(bound on xbar [C][p], bound on S [C][p][p]) of the module docstring, longdouble."""
    w, m, S = _moments(x, cols, row0, N)
    ctr = np.zeros(len(cols), dtype=LD) if center is None else np.asarray(center).astype(LD)
    delta = w[:, :, 0] - m
    E = np.einsum("caa->ca", S) + LD(N) / LD(N - 1) * delta * delta
    rE = np.sqrt(E)
    return ((N + 16) * LD(U) * rE + 2 * LD(U) * (np.abs(m) + np.abs(ctr)[None, :]),
            (N + 32) * LD(U) * rE[:, :, None] * rE[:, None, :])


def ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 the distance has to be 0 (ratio 0, else inf)."""
    err = np.abs(np.asarray(got).astype(LD) - ref)
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, LD(0), LD(np.inf)))
    return float(np.max(r)) if r.size else 0.0


def work_ratios(work, x, cols, row0, N, center):
    """(worst ratio of xbar, worst ratio of S) of a device or emulated work [C][p + p p] against the longdouble reference."""
    p = len(cols)
    xb, S = longdouble_work(x, cols, row0, N, center)
    bx, bS = work_bounds(x, cols, row0, N, center)
    Cn = xb.shape[0]
    return ratio(work[:, :p], xb, bx), ratio(work[:, p:].reshape(Cn, p, p), S, bS)


def emulate_work(x, cols, row0, N, center):
    """The float64 restatement of gelman_cov_mfma's order of operations: shift by the first window row, one pass, four
    waves on four contiguous ranges of 16-row groups, a column sum per lane class joined as (0 + 1) + (2 + 3), a product
    accumulator per wave taking rows {4 kk + u} of a group for u = 0 .. 3, the waves joined in order.  work [C][p + p p]."""
    x = np.asarray(x, dtype=np.float64)
    cols = np.asarray(cols)
    Cn, p = x.shape[0], len(cols)
    ctr = np.zeros(p) if center is None else np.asarray(center, dtype=np.float64)
    groups = (N + 15) // 16
    per = (groups + 3) // 4
    out = np.empty((Cn, p + p * p))
    for c in range(Cn):
        w = x[c][cols, row0:row0 + N].T                         # [N][p]
        shift = w[0].copy()
        d = w - shift
        acc_j = sum_j = None
        for wave in range(4):
            acc = np.zeros((p, p))
            cs = np.zeros((4, p))
            for gi in range(wave * per, min(wave * per + per, groups)):
                for u in range(4):
                    for kk in range(4):
                        t = 16 * gi + 4 * kk + u
                        if t < N:
                            cs[kk] += d[t]
                            acc += np.outer(d[t], d[t])
            s = (cs[0] + cs[1]) + (cs[2] + cs[3])
            acc_j = acc if wave == 0 else acc_j + acc
            sum_j = s if wave == 0 else sum_j + s
        out[c, :p] = (shift + sum_j / N) - ctr
        out[c, p:] = ((acc_j - np.outer(sum_j, sum_j) / N) / (N - 1.0)).ravel()
    return out


# ------------------------------------------------------------------------------------------------ the chain sum
def _partial_terms(w, p):
    """[C][1 + 5 p + 2 p p] terms of the partial of include/fmcmc_amd.h from work rows w [C][p + p p] (any float type)."""
    Cn = w.shape[0]
    xb, Sc = w[:, :p], w[:, p:].reshape(Cn, p, p)
    s2 = np.einsum("caa->ca", Sc)
    one = np.ones((Cn, 1), dtype=w.dtype)
    return np.concatenate([one, xb, (xb[:, :, None] * xb[:, None, :]).reshape(Cn, p * p), Sc.reshape(Cn, p * p),
                           s2, s2 * s2, s2 * xb, s2 * xb * xb], axis=1)


def longdouble_partial_from_work(work, p):
    """(partial, bound) in longdouble: the definition of the partial evaluated from `work` rows [C][p + p p] (the DEVICE's own
    when it judges gelman_sum_kernel), and (C + 8) u sum_c |term_c| per element, 0 for element 0."""
    _check_longdouble()
    t = _partial_terms(np.asarray(work).astype(LD), p)
    Cn = t.shape[0]
    bound = (Cn + 8) * LD(U) * np.abs(t).sum(0)
    bound[0] = 0
    return t.sum(0), bound


def partial_ratio(part, work, p):
    ref, bound = longdouble_partial_from_work(work, p)
    return ratio(part, ref, bound)


def emulate_partial(work, p):
    """gelman_sum_kernel in float64: four threads summing every fourth chain in order, joined as ((0 + 1) + 2) + 3."""
    t = _partial_terms(np.asarray(work, dtype=np.float64), p)
    g = []
    for i in range(4):
        s = np.zeros(t.shape[1])
        for c in range(i, t.shape[0], 4):
            s = s + t[c]
        g.append(s)
    out = ((g[0] + g[1]) + g[2]) + g[3]
    out[0] = t.shape[0]
    return out


def longdouble_partial(x, cols, row0, N, center):
    """The partial from the raw chains, all in longdouble."""
    xb, S = longdouble_work(x, cols, row0, N, center)
    Cn, p = xb.shape
    return longdouble_partial_from_work(np.concatenate([xb, S.reshape(Cn, p * p)], axis=1), p)[0]
