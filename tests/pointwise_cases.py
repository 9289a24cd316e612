"""The "table" callback, the inputs and the raw device calls that tests/test_gpu_pointwise_waic.py,
tests/test_gpu_pointwise_loo.py and tests/test_gpu_pointwise_streams.py share.  A plain module next to tests/waic_cases.py; torch
is imported where it is used, so collecting needs no GPU.

A table callback feeds any matrix L [S][n] to fmcmc_waic_fun_dev / fmcmc_loo_fun_dev: k = 1, the draw in `samples` is its own
index c N + row as a float, and fn returns L[theta[:, 0]] for the device copy of L.  The device and *_host_matrix(L in
longdouble) then see the same l to the bit: no evaluation error lies between them."""

import numpy as np

from fmcmc_amd import _abi as abi
from fmcmc_amd.summary import loo_tail_len

LD = np.longdouble
GUARD = 64
ROW0 = 5                              # odd, so the window starts off every alignment
# one unit; three units (no divisor of a part of 32); 33 units (a part and a unit); 32 units (whole parts at 4 x 1024 rows: what
# the default's rounding gives where the draws do not fit one block); the default (one block at these shapes)
BLOCK_ROWS = (16, 48, 528, 512, 0)


def index_samples(C_, N, row0=ROW0, pad=2):
    """[C][1][S]: the window [row0, row0 + N) of chain c holds c N, c N + 1, ...; the rows around it hold another valid index
    (0), which a call that reads outside its window would fold in.  S = row0 + N + pad."""
    S = row0 + N + pad
    x = np.zeros((C_, 1, S))
    x[:, 0, row0:row0 + N] = np.arange(C_ * N, dtype=np.float64).reshape(C_, N)
    return np.ascontiguousarray(x)


class Table:
    """fn(theta) = L[theta[:, 0]] on the device, with the blocks it was called on (rows per call).  A draw that is not a number
    or lies outside the table reads row 0: the callback itself never leaves the table."""

    def __init__(self, L, fail_at=None, fail_with=None):
        import torch
        self.L = torch.as_tensor(np.ascontiguousarray(L, dtype=np.float64)).cuda()
        self.calls, self.fail_at, self.fail_with = [], fail_at, fail_with

    def __call__(self, theta):
        import torch
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            self.calls.append(-1)
            raise self.fail_with
        self.calls.append(int(theta.shape[0]))
        idx = torch.nan_to_num(theta[:, 0], nan=0.0, posinf=0.0, neginf=0.0).long().clamp_(0, self.L.shape[0] - 1)
        return self.L[idx]


def callback(fn, n, stream=None):
    """fn as a fmcmc_pointwise_fn (the library's own trampoline), and the list that keeps what it raised"""
    import torch
    import fmcmc_amd as F
    from fmcmc_amd.engine import _Views
    from fmcmc_amd.summary import _pointwise_trampoline
    dev = torch.device("cuda", torch.cuda.current_device())
    caught = []
    stream = torch.cuda.current_stream() if stream is None else stream
    return _pointwise_trampoline(F.pointwise_fun(fn, n, 1), dev, stream, _Views(dev), caught), caught


def blocks(units, block_rows, n):
    """the calls of one sweep over `units` units"""
    ub = (block_rows + 15) // 16 if block_rows else max(1, (1 << 25) // (16 * n))
    return -(-units // min(max(ub, 1), max(units, 1)))


def device_fun(what, fn, n, samples, N, block_rows, row0=ROW0, want_tail=True, run=None, cb=None, expect=abi.OK):
    """One fmcmc_waic_fun_dev (what = "waic") or fmcmc_loo_fun_dev ("loo") call on samples [C][k][S] with the window at row0:
    NaN-filled buffers GUARD doubles longer than documented, which must stay NaN.  Returns (point, total) or (point, tail, total,
    state [n][8] int64) as numpy.  run: as in tests/diag_dev.py: device_call (the callback then works on the stream it is given
    by `cb`, made by the caller).  expect: the return code; another one than OK returns (code, message) instead."""
    import torch
    L = abi.lib()
    Cn, k, S = samples.shape
    loo = what == "loo"
    M = loo_tail_len(Cn * N)
    xd = torch.as_tensor(np.ascontiguousarray(samples)).cuda()
    nwork = (L.fmcmc_loo_fun_work_len if loo else L.fmcmc_waic_fun_work_len)(n, Cn, N, block_rows)
    assert nwork > 0, abi.last_error()
    lens = (nwork, n * 6, n * M, 12) if loo else (nwork, n * 4, 10)
    bufs = [torch.full((int(v) + GUARD,), float("nan"), dtype=torch.float64, device="cuda") for v in lens]
    caught = []
    if cb is None:
        cb, caught = callback(fn, n)
    head = (cb, None, n, xd.data_ptr(), Cn, k, S, row0, N, block_rows, bufs[0].data_ptr(), bufs[1].data_ptr())
    if loo:
        call = lambda stream: L.fmcmc_loo_fun_dev(*head, bufs[2].data_ptr() if want_tail else None, bufs[3].data_ptr(), stream)
    else:
        call = lambda stream: L.fmcmc_waic_fun_dev(*head, bufs[2].data_ptr(), stream)
    rc = call(None) if run is None else run([xd], bufs, call)
    torch.cuda.synchronize()
    if caught:
        raise caught[0]
    if expect != abi.OK:
        assert rc == expect, (rc, abi.last_error())
        return rc, abi.last_error()
    assert rc == abi.OK, (rc, abi.last_error())
    host = [b.cpu().numpy() for b in bufs[1:]]
    assert all(np.isnan(h[int(v):]).all() for h, v in zip(host, lens[1:]))      # nothing past the documented lengths
    assert torch.isnan(bufs[0][lens[0]:]).all()
    if not loo:
        return host[0][:lens[1]].reshape(n, 4), host[1][:10]
    off = L.fmcmc_loo_fun_state_offset(n, Cn, N, block_rows)
    assert off >= 0
    state = bufs[0][off:off + 8 * n].cpu().numpy().view(np.int64).reshape(n, 8)
    return host[0][:lens[1]].reshape(n, 6), host[1][:lens[2]].reshape(n, M), host[2][:12], state


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def smooth_matrix(S, n, seed):
    """l of a plausible model: -0.5 z^2 minus an offset per observation, a few observations with heavier tails"""
    rng = np.random.default_rng(seed)
    scale = 1.0 + 0.5 * (np.arange(n) % 3)
    return -0.5 * (scale[None, :] * rng.standard_normal((S, n))) ** 2 - 0.9 + 0.3 * rng.standard_normal(n)[None, :]
