"""What tests/test_rank_rhat_host.py and tests/test_gpu_rank_rhat.py share: the literal restatement of the rank-normalised split
R-hat, the constructed cases whose answer follows from the definition alone, and the error bounds of the
device reduction, derived from its documented order of operations (csrc/diag_rank.hpp: split_stats_kernel).
A plain module next to tests/gelman_ref.py."""
import numpy as np

U = 2.0 ** -53                      # unit roundoff of float64
QNORM_REL = 4e-15                   # fmh_qnorm against scipy's ndtri, relative (tests/test_detmath.py holds it to this)


# ------------------------------------------------------------------------------------------------ the definition, written out
def literal_rhat(data):
    """data [C][N][p] -> (bulk [p], tail [p], rhat [p], med [p]), step by step as the definition states it, with plain loops."""
    from scipy.special import ndtri
    data = np.asarray(data, dtype=np.float64)
    Cn, N, p = data.shape
    nh = N // 2
    m, M = 2 * Cn, 2 * Cn * nh

    def one(v):                                       # steps 2-4 on v [m][nh]
        flat = [float(v[s][r]) + 0.0 for s in range(m) for r in range(nh)]
        z = np.empty((m, nh), dtype=np.longdouble)
        for s in range(m):
            for r in range(nh):
                x = flat[s * nh + r]
                less = sum(1 for y in flat if y < x)
                equal = sum(1 for y in flat if y == x)
                rank = (2 * less + equal + 1) / 2.0
                z[s][r] = ndtri((rank - 0.375) / (M + 0.25))
        means = [sum(z[s]) / nh for s in range(m)]
        variances = [sum((z[s][r] - means[s]) ** 2 for r in range(nh)) / (nh - 1) for s in range(m)]
        grand = sum(means) / m
        B = nh * sum((mu - grand) ** 2 for mu in means) / (m - 1)
        W = sum(variances) / m
        return float("nan") if W == 0 else float(np.sqrt((B / W + nh - 1) / nh))

    bulk, tail, med = [], [], []
    for j in range(p):
        v = np.array([list(data[c, :nh, j]) if h == 0 else list(data[c, N - nh:, j]) for c in range(Cn) for h in (0, 1)])
        srt = sorted(float(t) + 0.0 for t in v.ravel())
        med.append((srt[M // 2 - 1] + srt[M // 2]) / 2.0)
        bulk.append(one(v))
        tail.append(one(np.abs(v - med[-1])))
    rhat = [float("nan") if np.isnan(b) or np.isnan(t) else max(b, t) for b, t in zip(bulk, tail)]
    return np.array(bulk), np.array(tail), np.array(rhat), np.array(med)


# ------------------------------------------------------------------------------------------------ constructed cases [C][N][1]
def identical_chains(Cn=4, N=100, seed=11):
    """every chain AND both halves of it hold the same rows: all split chains are equal, B = 0"""
    half = np.random.default_rng(seed).standard_normal(N // 2)
    return np.tile(np.concatenate([half, half])[None, :, None], (Cn, 1, 1))


def shifted_chains(Cn=4, N=200, seed=12):
    """unit-variance chains, every second one shifted by ten standard deviations"""
    x = np.random.default_rng(seed).standard_normal((Cn, N, 1))
    x[1::2] += 10.0
    return x


def scaled_chains(Cn=4, N=400, seed=13):
    """equal location, scales 1 and 10 in turn"""
    x = np.random.default_rng(seed).standard_normal((Cn, N, 1))
    x[1::2] *= 10.0
    return x


# ------------------------------------------------------------------------------------------------ bounds
def depth(nh):
    """additions a value passes through in a sum of split_stats_kernel over nh rows: a thread adds at most 8 values of every
    batch of 2048 rows, then 6 butterfly steps, then the 4 wavefront sums"""
    return 8 * -(-nh // 2048) + 6 + 4


def gamma(n):
    return n * U / (1.0 - n * U)


def moment_bounds(z):
    """z [m][nh] (the exact scores, any float type) -> (E_mean [m], E_var [m]): how far the device's mean and variance of every
    row may be from the exact ones.
      sum:   fl(sum) = sum z_i (1 + t_i), |t_i| <= gamma(D), D = depth(nh); the division by nh adds one rounding:
             E_mean = gamma(D + 1) sum|z_i| / nh.
      var:   with the device's mean mu' = mu + d, |d| <= E_mean: sum (z_i - mu')^2 = S + nh d^2, S = sum (z_i - mu)^2; every term
             carries 3 roundings (difference, product; the product squares the first), the sum D, the division 1:
             E_var = (gamma(D + 4) (S + nh E_mean^2) + nh E_mean^2) / (nh - 1).
    The np.longdouble reference adds at most nh 2^-64 relative to sum|z_i| resp. S; it is included."""
    z = np.asarray(z, dtype=np.longdouble)
    nh = z.shape[1]
    D = depth(nh)
    ref = nh * 2.0 ** -64
    sabs = np.abs(z).sum(axis=1)
    e_mean = (gamma(D + 1) + ref) * sabs / nh
    S = ((z - z.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    e_var = ((gamma(D + 4) + ref) * (S + nh * e_mean ** 2) + nh * e_mean ** 2) / (nh - 1)
    return e_mean.astype(np.float64), e_var.astype(np.float64)


def score_shift_bounds(z):
    """z [m][nh] -> (dmean [m], dvar [m]): how far mean and variance of a row move when every score moves by at most
    a_i = QNORM_REL |z_i| (the host's ndtri against the device's fmh_qnorm): the mean by mean(a); a deviation z_i - mu by at most
    b = max(a) + mean(a), so S by at most 2 b sum|z_i - mu| + nh b^2."""
    z = np.asarray(z, dtype=np.float64)
    nh = z.shape[1]
    a = QNORM_REL * np.abs(z)
    dmean = a.mean(axis=1)
    b = a.max(axis=1) + dmean
    dev = np.abs(z - z.mean(axis=1, keepdims=True)).sum(axis=1)
    return dmean, (2.0 * b * dev + nh * b * b) / (nh - 1)


def rhat_bound(means, variances, e_mean, e_var, nh):
    """The bounds of the moments carried through step 4.  With the means off by at most e = max(e_mean), a deviation from the
    grand mean moves by at most 2 e: B = nh / (m - 1) sum d_s^2 moves by dB <= nh / (m - 1) (4 e sum|d_s| + 4 m e^2); W by
    dW <= max(e_var).  B / W moves by at most (dB + (B / W) dW) / (W - dW), and R = sqrt((B / W + nh - 1) / nh) by that over
    2 nh R_min, R_min = sqrt((nh - 1) / nh); 8 U R covers the roundings of the finish itself."""
    mu = np.asarray(means, dtype=np.float64)
    s2 = np.asarray(variances, dtype=np.float64)
    m = mu.size
    e, dW = float(np.max(e_mean)), float(np.max(e_var))
    d = mu - mu.mean()
    B, W = nh * (d * d).sum() / (m - 1), s2.mean()
    dB = nh / (m - 1) * (4.0 * e * np.abs(d).sum() + 4.0 * m * e * e)
    assert W > 2.0 * dW, "the bound needs W well above its own error"
    ratio = (dB + B / W * dW) / (W - dW)
    R = np.sqrt((B / W + nh - 1) / nh)
    return ratio / (2.0 * nh * np.sqrt((nh - 1.0) / nh)) + 8.0 * U * R
