"""fmcmc_waic_fun_dev and fmcmc_loo_fun_dev are held to their caller's stream, with the gate of tests/test_gpu_streams.py
(direction A there): the call goes to a side stream that a timed gate keeps busy; before it every device input holds a decoy;
on the side stream, in this order: the gate, the copy of the true inputs, a NaN fill of every buffer, the call.  A piece of the
call -- a kernel, or the callback's own work -- that ran elsewhere read decoys or had its output overwritten by the fill, and the
bits would differ from the ungated run on the default stream.

fmcmc_waic_fun_dev only enqueues: the gate is still closed when it returns.  fmcmc_loo_fun_dev synchronises once, behind the
collect sweep (include/fmcmc_amd.h): every callback of the sample pass and of the collect sweep is made while the gate is closed,
the call returns after it opened, and with flagged observations the histogram sweeps are called after it opened."""
import time

import numpy as np
import pytest

import pointwise_cases as P
from test_gpu_pointwise_loo import C_, N, S, UNITS, fallback_matrix
from test_gpu_streams import Gate, decoy, quiet_host, side_streams, sptr

pytestmark = pytest.mark.gpu
GATE_MS = 60.0          # the host side of the longest call here (11 sweeps of 8 blocks, a Python callback each) takes a few ms
BR = 528


class Watched(P.Table):
    """a table callback that notes whether the gate was closed at each call"""

    def __init__(self, L):
        super().__init__(L)
        self.gate, self.closed = None, []

    def __call__(self, theta):
        self.closed.append(self.gate.closed() if self.gate is not None else None)
        return super().__call__(theta)


def gated(what, L, n):
    """(reference, gated result, the callback of the gated run, closed at return, host ms, the gate)"""
    import torch
    x = P.index_samples(C_, N)
    ref = P.device_fun(what, P.Table(L), n, x, N, BR)
    side = side_streams()[0]
    tab = Watched(L)
    cb, caught = P.callback(tab, n, stream=side)
    seen = {}

    def run(inputs, bufs, call):
        true = [t.clone() for t in inputs]
        for t in inputs:
            t.copy_(decoy(t))
        torch.cuda.synchronize()
        quiet_host()
        gate = tab.gate = Gate(side, GATE_MS)
        with torch.cuda.stream(side):
            for t, v in zip(inputs, true):
                t.copy_(v, non_blocking=True)
            for b in bufs:
                b.fill_(float("nan"))
            t0 = time.perf_counter()
            rc = call(sptr(side))
            seen["ms"] = 1e3 * (time.perf_counter() - t0)
            seen["closed"] = gate.closed()
        torch.cuda.synchronize()
        seen["gate"] = gate
        return rc

    got = P.device_fun(what, None, n, x, N, BR, run=run, cb=cb)
    assert not caught
    return ref, got, tab, seen


def test_waic_stays_on_its_stream_and_only_enqueues():
    n = 70
    L = P.smooth_matrix(S, n, seed=50)
    ref, got, tab, seen = gated("waic", L, n)
    assert seen["closed"], seen["gate"].too_short(seen["ms"])
    assert all(tab.closed) and len(tab.closed) == P.blocks(UNITS, BR, n)
    for a, b in zip(got, ref):
        assert np.array_equal(P.bits(a), P.bits(b))


@pytest.mark.parametrize("flagged", [False, True], ids=["hit-only", "fallback"])
def test_loo_stays_on_its_stream_and_synchronises_once(flagged):
    n = 70
    L = fallback_matrix(n, (5, 66)) if flagged else P.smooth_matrix(S, n, seed=51)
    ref, got, tab, seen = gated("loo", L, n)
    before = P.blocks(UNITS // 4, BR, n) + P.blocks(UNITS, BR, n)
    assert all(tab.closed[:before]), seen["gate"].too_short(seen["ms"])      # nothing waited before the documented place
    assert not seen["closed"]                                                # the call itself waited for the stream
    assert len(tab.closed) == before + (9 * P.blocks(UNITS, BR, n) if flagged else 0)
    assert not any(tab.closed[before:])
    for a, b in zip(got, ref):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
