"""Time of the kernels behind waic() / loo() of a pointwise_fun (csrc/diag_pointwise.hpp), in one process, at 4 chains x 10^4 rows x
n = 10^4 observations.  The callback costs nothing: it is a C-level function that leaves the [B][n] block as it is (seeded values
that were written into `work` before the call) and records a HIP event on the call's stream, so the gap between the events of two
consecutive callbacks is the device time of one block: the fold (or collect) kernel of block j, the gather kernel of block j + 1
and the two launch boundaries between them.  The rates below are therefore LOWER bounds of the fold (collect) kernel's own rate.
Per block size (0 = the library's choice):
  * fold_ms_per_block / collect_ms_per_block: the median gap; *_bytes_per_s = 8 B n / that; the shares of the 8.0 TB/s of the
    HBM3E specification and of the 6.29 TB/s a copy kernel reaches (MI355X: what the project's own notes measured)
  * torch_ms_per_block: torch.logsumexp(ll, 0) and ll.var(0) on a block of the same shape, best of five between two events
  * waic_call_ms / loo_call_ms: two events around the whole call (host enqueueing included), best of three
Usage: python tools/bench_pointwise.py [--blocks 0,1664,6656,20000] [--chains 4 --rows 10000 --obs 10000] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="0,1664,6656,20000")
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--obs", type=int, default=10000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import loo_plan, loo_tail_len
    L = abi.lib()
    Cn, N, n = a.chains, a.rows, a.obs
    S = Cn * N
    x = torch.zeros((Cn, 1, N), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream()
    plan = loo_plan(Cn, N, n)
    M = loo_tail_len(S)
    lines = []
    pool = [torch.cuda.Event(enable_timing=True) for _ in range(4096)]

    def gaps(evs):
        return [evs[j].elapsed_time(evs[j + 1]) for j in range(len(evs) - 1)]

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = call()
        e1.record()
        e1.synchronize()
        assert rc == abi.OK, abi.last_error()
        return e0.elapsed_time(e1)

    for br in (int(v) for v in a.blocks.split(",")):
        B = int(L.fmcmc_pointwise_block_rows(n, Cn, N, br))
        nwork = int(L.fmcmc_loo_fun_work_len(n, Cn, N, br))
        assert B > 0 and nwork > 0, abi.last_error()
        g = torch.Generator(device="cuda").manual_seed(11)
        work = -torch.randn(nwork, generator=g, dtype=torch.float64, device="cuda").abs_()
        point = torch.empty(n * 6, dtype=torch.float64, device="cuda")
        total = torch.empty(12, dtype=torch.float64, device="cuda")
        evs, rows = [], []

        def cb(theta, Bj, k, n_, ll, st, user):
            e = pool[len(evs)]                                       # (made before the call: the callback only records)
            e.record(stream)
            evs.append(e)
            rows.append(int(Bj))
            return 0

        ccb = abi.POINTWISE_FN(cb)
        sp = stream.cuda_stream
        waic = lambda: L.fmcmc_waic_fun_dev(ccb, None, n, x.data_ptr(), Cn, 1, N, 0, N, br, work.data_ptr(), point.data_ptr(),
                                            total.data_ptr(), sp)
        loo = lambda: L.fmcmc_loo_fun_dev(ccb, None, n, x.data_ptr(), Cn, 1, N, 0, N, br, work.data_ptr(), point.data_ptr(), None,
                                          total.data_ptr(), sp)
        out = dict(block_rows_asked=br, block_rows=B, chains=Cn, rows=N, observations=n, block_bytes=8 * B * n,
                   work_bytes=8 * nwork, plan=vars(plan))
        for name, call in (("waic", waic), ("loo", loo)):
            timed(call)                                              # warm-up
            best, per = None, []
            for _ in range(3):
                del evs[:], rows[:]
                ms = timed(call)
                best = ms if best is None else min(best, ms)
                gp, rw = gaps(evs), list(rows)
                if name == "loo":                                    # the collect sweep: the callbacks behind the sample pass
                    nsub = next(j for j in range(1, len(rw) + 1) if sum(rw[:j]) == plan.sub_rows)
                    assert sum(rw[nsub:]) == S, "an observation took the fallback"
                    gp, rw = gp[nsub:], rw[nsub:]
                full = [t for t, r in zip(gp, rw) if r == B]         # (the gap behind the last callback is not measured)
                per += full
            key = "fold" if name == "waic" else "collect"
            out["%s_call_ms" % name] = round(best, 3)
            out["%s_blocks" % key] = len(rw)
            if per:
                ms = float(np.median(per))
                bps = 8.0 * B * n / (ms * 1e-3)
                out.update({"%s_ms_per_block" % key: round(ms, 4), "%s_bytes_per_s" % key: round(bps, 0),
                            "%s_share_of_hbm_spec" % key: round(bps / HBM_SPEC, 3),
                            "%s_share_of_hbm_copy" % key: round(bps / HBM_COPY, 3)})
            else:                                                    # one block: the call itself, finishing kernels included
                out["%s_ms_per_block" % key] = None
        del work
        torch.cuda.empty_cache()
        ll = -torch.randn((B, n), generator=g, dtype=torch.float64, device="cuda").abs_()

        def torch_block():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep = (torch.logsumexp(ll, 0), ll.var(0))
            e1.record()
            e1.synchronize()
            del keep
            return e0.elapsed_time(e1)

        torch_block()
        out["torch_ms_per_block"] = round(min(torch_block() for _ in range(5)), 4)
        del ll
        torch.cuda.empty_cache()
        lines.append(out)
        print(json.dumps(out), flush=True)
    if a.json:
        props = torch.cuda.get_device_properties(0)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_pointwise.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "a HIP event per callback; a block's time is the median gap between the events of two consecutive "
                                 "callbacks of full blocks over three calls after a warm-up; calls: two events around the call, "
                                 "best of three; torch: best of five", "blocks": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
