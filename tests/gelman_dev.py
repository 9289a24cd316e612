"""The device call, the inputs and the bit comparisons that the GPU tests of the Gelman-Rubin window reduction share
(tests/test_gpu_gelman_narrow.py, tests/test_gpu_gelman_wide.py) with the writer of their fixtures (tests/golden/make_gelman_bits.py).
A plain module next to tests/gelman_ref.py; torch is imported where it is used, so collecting needs no GPU."""
import numpy as np

GUARD = 64
FIRST_ROW = "first row of chain 0"


def make_chains(Cn, k, S, seed):
    """[C][k][S]: noise, an offset per chain and column, a slow random walk.  The committed fixtures are bits of these inputs."""
    rng = np.random.default_rng(seed)
    return (0.5 * rng.standard_normal((Cn, k, S)) + 0.2 * rng.standard_normal((Cn, k, 1)) + 3.0
            + 0.01 * np.cumsum(rng.standard_normal((Cn, k, S)), axis=2))


def pick_columns(k, p, seed):
    return (np.arange(k) if p == k else np.sort(np.random.default_rng(seed).choice(k, size=p, replace=False))).astype(np.int32)


def device_partial(x, cols, row0, N, center=FIRST_ROW, run=None):
    """One fmcmc_gelman_partial_dev call on x [C][k][S]: (work [C][p + p p], partial) as numpy; buffers NaN-filled, guards
    checked.  center None passes a null pointer.  run: None, or run(inputs, buffers, call) -> code, which makes the call as
    call(hip_stream) on a stream of its choice (tests/test_gpu_streams.py); the device inputs and the buffers are its to prepare,
    and the buffers must be NaN beyond what the call writes when it returns."""
    import torch
    from fmcmc_amd import _abi as abi
    L = abi.lib()
    Cn, k, S = x.shape
    p = len(cols)
    assert row0 >= 0 and row0 + N <= S and N >= 2 and min(cols) >= 0 and max(cols) < k
    xd = torch.as_tensor(np.ascontiguousarray(x)).cuda()
    cd = torch.as_tensor(np.ascontiguousarray(cols, dtype=np.int32)).cuda()
    if isinstance(center, str):
        center = x[0, cols, row0]
    ctr = None if center is None else torch.as_tensor(np.ascontiguousarray(center, dtype=np.float64)).cuda()
    wlen, plen = int(L.fmcmc_gelman_work_len(Cn, p)), int(L.fmcmc_gelman_partial_len(p))
    assert wlen == Cn * (p + p * p) and plen == 1 + 5 * p + 2 * p * p
    work = torch.full((wlen + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    part = torch.full((plen + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    call = lambda stream: L.fmcmc_gelman_partial_dev(xd.data_ptr(), Cn, k, S, row0, N, cd.data_ptr(), p,
                                                     None if ctr is None else ctr.data_ptr(), work.data_ptr(), part.data_ptr(), stream)
    rc = call(None) if run is None else run([xd, cd] + ([] if ctr is None else [ctr]), [work, part], call)
    assert rc == abi.OK, rc
    torch.cuda.synchronize()
    wh, ph = work.cpu().numpy(), part.cpu().numpy()
    assert np.isnan(wh[wlen:]).all() and np.isnan(ph[plen:]).all()      # nothing written past the documented lengths
    return wh[:wlen].reshape(Cn, p + p * p), ph[:plen]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def bit_checksums(u64):
    """Order-dependent and order-independent 64-bit checksums of a vector of bit patterns, as hex strings."""
    u64 = np.asarray(u64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        weighted = (u64 * (np.arange(u64.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64)
    return {"n": int(u64.size), "xor": "%016x" % int(np.bitwise_xor.reduce(u64)), "weighted_sum": "%016x" % int(weighted),
            "first": "%016x" % int(u64[0]), "last": "%016x" % int(u64[-1])}


def narrow_case(p):
    """The p <= 64 inputs of tests/golden/gelman_narrow_bits.json and the bits of the device result (work, partial)."""
    Cn, k, S, row0, N = 5, 64, 141, 7, 131
    x = make_chains(Cn, k, S, 64000 + p)
    work, part = device_partial(x, pick_columns(k, p, p), row0, N)
    return _bits(work).ravel(), _bits(part)


# (p, N) of tests/golden/gelman_bits.json: each number of column blocks of one super-block at both ends of its range, then 2, 3
# and 4 super-blocks (65 and 129: a last one of one live column); N = 2 leaves three waves idle, N = 333 gives every wave more
# than three row groups (the buffer rotation) and a ragged tail
BITS_SHAPES = ([(p, N) for p in (1, 16, 17, 32, 33, 48, 49) for N in (2, 37, 333)]
               + [(p, N) for p in (65, 129, 200, 256) for N in (17, 333)])


def bits_case(p, N):
    """Inputs of one shape of tests/golden/gelman_bits.json (three chains, an odd row stride, row0 = 5, a shuffled subset of
    k = p + 3 columns, every one of 256 at p = 256) and the bits of the device result (work, partial)."""
    Cn, row0, k = 3, 5, 256 if p == 256 else p + 3
    S = row0 + N + 2
    S += 1 - S % 2
    x = make_chains(Cn, k, S, 9000 * p + N)
    cols = np.random.default_rng(1000 * p + N).permutation(k)[:p].astype(np.int32)
    work, part = device_partial(x, cols, row0, N)
    return _bits(work).ravel(), _bits(part)
