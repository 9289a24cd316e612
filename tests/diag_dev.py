"""The raw device calls, the inputs and the cases that tests/test_gpu_diag_bits.py shares with the writer of its fixture
(tests/golden/make_diag_bits.py): the four windowed diagnostics (fmcmc_summary_dev, fmcmc_heidel_dev, fmcmc_chain_order_dev,
fmcmc_raftery_dev) at the smallest lengths at which the code they share (csrc/diag_common.hpp: the pair walk, the keys, the
rank pair) can go wrong.  A plain module next to tests/gelman_dev.py; torch is imported where it is used, so collecting needs no
GPU."""
import ctypes as C

import numpy as np

from gelman_dev import GUARD, _bits

CHAINS, K, ROW0, COLS = 3, 4, 5, (2, 0, 3)
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
SERIES = CHAINS * len(COLS)


def make_series(N, seed, non_finite=False):
    """[3][4][S], S odd with a few rows on both sides of the window [5, 5 + N): a moving average of seeded noise around an offset
    per chain and column (values of both signs); column 0 is rounded to two decimals, so it has ties.  `non_finite` plants one
    NaN and one infinity in the window of chain 1, column 2."""
    S = ROW0 + N + 2
    S += 1 - S % 2
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((CHAINS, K, S + 1))
    x = e[:, :, 1:] + 0.5 * e[:, :, :-1] + 0.3 * rng.standard_normal((CHAINS, K, 1))
    x[:, 0, :] = np.round(x[:, 0, :], 2)
    if non_finite:
        x[1, 2, ROW0 + 7], x[1, 2, ROW0 + N - 3] = np.nan, np.inf
    return np.ascontiguousarray(x)


def device_call(name, x, N, mid, lens, run=None):
    """One call L.<name>(samples, C, k, S, ROW0, N, cols, p, *mid, *buffers, stream 0) on x [C][k][S]: a buffer of doubles per
    entry of `lens` (None: a null pointer), NaN-filled and GUARD elements longer than asked, which must stay NaN.  Returns the
    buffers as numpy arrays of their documented lengths.  run: None, or run(inputs, buffers, call) -> code, which makes the
    call as call(hip_stream) on a stream of its choice (tests/test_gpu_streams.py); the device inputs and the buffers are its
    to prepare, and the buffers must be NaN beyond what the call writes when it returns."""
    import torch
    from fmcmc_amd import _abi as abi
    Cn, k, S = x.shape
    assert ROW0 + N <= S and max(COLS) < k
    xd = torch.as_tensor(x).cuda()
    cd = torch.as_tensor(np.asarray(COLS, dtype=np.int32)).cuda()
    bufs = [None if n is None else torch.full((int(n) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for n in lens]
    call = lambda stream: getattr(abi.lib(), name)(xd.data_ptr(), Cn, k, S, ROW0, N, cd.data_ptr(), len(COLS), *mid,
                                                   *[None if b is None else b.data_ptr() for b in bufs], stream)
    rc = call(None) if run is None else run([xd, cd], [b for b in bufs if b is not None], call)
    assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    host = [None if b is None else b.cpu().numpy() for b in bufs]
    assert all(np.isnan(h[int(n):]).all() for h, n in zip(host, lens) if h is not None)   # nothing past the documented lengths
    return [None if h is None else h[:int(n)] for h, n in zip(host, lens)]


def _lib():
    from fmcmc_amd import _abi as abi
    return abi.lib()


def summary_case(N, non_finite=False, run=None):
    """The five default probs, chain_stats asked for: slots 0..67 of every series' 72-double head of `work` (68..71 are never
    written), chain_stats and pooled."""
    L, nprobs = _lib(), len(PROBS)
    probs = np.asarray(PROBS, dtype=np.float64)
    work, stats, pooled = device_call("fmcmc_summary_dev", make_series(N, 1000 + N, non_finite), N,
                                      (probs.ctypes.data_as(C.POINTER(C.c_double)), nprobs),
                                      (L.fmcmc_summary_work_len(CHAINS, len(COLS), nprobs), SERIES * 4,
                                       L.fmcmc_summary_pooled_len(len(COLS), nprobs)), run)
    head = work[:SERIES * 72].reshape(SERIES, 72)
    if non_finite:
        return {"non_finite": _bits(head[:, 67]), "pooled_non_finite": _bits(pooled[:5 * len(COLS)].reshape(-1, 5)[:, 4])}
    return {"work": _bits(head[:, :68]).ravel(), "chain_stats": _bits(stats), "pooled": _bits(pooled)}


def heidel_case(N, non_finite=False, run=None):
    """The windows heidel() takes of the iterations 1 .. N: all of `out`, and the non-finite slot of every series of `work`."""
    from fmcmc_amd.summary import heidel_candidates
    L = _lib()
    _, rows, half = heidel_candidates(np.arange(1, N + 1))
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    work, out = device_call("fmcmc_heidel_dev", make_series(N, 2000 + N, non_finite), N,
                            (int(half), rows.ctypes.data_as(C.POINTER(C.c_int64)), int(rows.size)),
                            (L.fmcmc_heidel_work_len(CHAINS, len(COLS), rows.size), L.fmcmc_heidel_out_len(CHAINS, len(COLS), rows.size)),
                            run)
    nf = {"non_finite": _bits(work.reshape(SERIES, 72)[:, 67])}
    return nf if non_finite else dict(nf, out=_bits(out))


def order_case(N, nprobs, non_finite=False, run=None):
    """nprobs = 0: the one rank of the lower median; else the 2 nprobs ranks of evenly spaced probs from 0 to 1.  `out` and the
    non-finite counts."""
    from fmcmc_amd.summary import type7_order_ranks
    probs = [0.5] if nprobs == 0 else np.linspace(0.0, 1.0, nprobs)
    ranks = np.ascontiguousarray(type7_order_ranks(N, probs).ravel()[:1 if nprobs == 0 else None], dtype=np.int64)
    work, out = device_call("fmcmc_chain_order_dev", make_series(N, 3000 + N + nprobs, non_finite), N,
                            (ranks.ctypes.data_as(C.POINTER(C.c_int64)), int(ranks.size)),
                            (_lib().fmcmc_chain_order_work_len(CHAINS, len(COLS), ranks.size), SERIES * ranks.size), run)
    nf = {"non_finite": _bits(work)}
    return nf if non_finite else dict(nf, out=_bits(out))


def raftery_case(N, q, j0, nj, non_finite=False, run=None):
    """The head (u, x_(lo), x_(hi), non-finite count per series) and the integer counts of the thinnings j0 .. j0 + nj - 1 (they
    cover the indicator words in `work`)."""
    L = _lib()
    _work, out = device_call("fmcmc_raftery_dev", make_series(N, 4000 + N, non_finite), N, (float(q), int(j0), int(nj)),
                             (L.fmcmc_raftery_work_len(CHAINS, len(COLS), N), L.fmcmc_raftery_out_len(CHAINS, len(COLS), nj)),
                             run)
    head = out[:SERIES * 4].reshape(SERIES, 4)
    if non_finite:
        return {"non_finite": _bits(head[:, 3])}
    return {"head": _bits(head).ravel(), "counts": _bits(out[SERIES * 4:])}


# The lengths: the shortest windows; one batch of the pair walk (2 x 8 pairs x 512 threads = 8192 rows in summary_series_kernel,
# 2 x 4 x 512 = 4096 in raftery.hip) with one row less and one more; the 19456 rows that are staged in LDS and one more; two such
# tiles and a row (38913); tails on both sides of the 4608-row scan tile of summary_cvm_kernel; 23553 rows, which the unstaged
# select re-reads through the pair walk on every pass.
CASES = {}
CASES.update({"summary_N%d" % N: (summary_case, (N,)) for N in (3, 4, 17, 1025, 8191, 8192, 8193, 19456, 19457, 38913)})
CASES.update({"heidel_N%d" % N: (heidel_case, (N,)) for N in (30, 4609, 9300, 20000)})
CASES.update({"order_N%d_probs%d" % (N, n): (order_case, (N, n)) for N in (3, 4, 65, 4095, 4096, 4097, 19456, 19457, 23553)
              for n in (0, 16)})
CASES.update({"raftery_N%d_q%g_j%d_%d" % (N, q, j0, nj): (raftery_case, (N, q, j0, nj)) for N in (3, 64, 65, 4097, 19456, 19457)
              for q in (0.025, 0.5) for j0, nj in ((1, 16), (17, 32))})
CASES.update({"summary_non_finite": (summary_case, (1025, True)), "heidel_non_finite": (heidel_case, (1025, True)),
              "order_non_finite": (order_case, (1025, 16, True)), "raftery_non_finite": (raftery_case, (1025, 0.025, 1, 16, True))})


def run_case(key):
    """name -> bit patterns (uint64) of what the case compares."""
    fn, args = CASES[key]
    return fn(*args)
