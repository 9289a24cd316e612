"""Time of the rank-normalised bulk / tail effective sample size on the device (fmcmc_amd/summary.py: ess -> csrc/diag_ess.hpp)
next to the route a user had before it, on the output of bench.py's headline config (kernel_normal(scale = 0.02)):
  * headline: 1024 chains x 5 parameters x 10^4 kept rows (M = 1.024 x 10^7 pooled values a column)
  * small:    4 chains x 5 parameters x 2000 kept rows
Per shape, one warm-up call and then the best of five of: the enqueued kernels of one fmcmc_rank_ess_dev call between two HIP
events; the wall time of ess() including the copy back and the finish; the wall time of rhat() on the same rows; the wall time
of DeviceChains.to_host() of the same rows.  Once: convergence.ess_host on a bounded sample of the copied rows (one column, at
most --host-chains chains: the longdouble sums of the host restatement take minutes on the whole headline result), and the
largest relative difference between the two results on that sample.
Usage: python tools/bench_ess.py [--shapes headline,small] [--host-chains 64] [--json FILE]   (one JSON line per shape; --json
also writes them, with the device and the date, to FILE: profiles/bench_ess.json holds the run DESIGN.md section 5.10 quotes)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"headline": (None, 10000), "small": (4, 2000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,small")
    ap.add_argument("--host-chains", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import enqueue_rank_ess
    from bench import Config
    dev = torch.device("cuda", 0)
    lines = []
    for shape in a.shapes.split(","):
        chains, nsteps = SHAPES[shape]
        cfg = Config("c2")
        chains = cfg.chains if chains is None else chains
        X, y, init = cfg.workload(chains, 0)
        dc = F.MCMC(init, F.gaussian_linreg(X, y), nsteps, nchains=chains, seed=1215, kernel=F.kernel_normal(scale=0.02),
                    _return_device=True, keep_logpost=False, keep_draws=False)
        C_, k, N = (int(v) for v in dc.samples.shape)

        def kernels():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            keep = enqueue_rank_ess(dc, 0, N, None)
            e1.record()
            e1.synchronize()
            del keep
            return e0.elapsed_time(e1) * 1e-3

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            wall.last = out
            return time.perf_counter() - t0

        best = {}
        for name, fn in (("ess_kernels_ms", kernels), ("ess_wall_ms", lambda: wall(dc.ess)),
                         ("rhat_wall_ms", lambda: wall(dc.rhat)), ("to_host_wall_ms", lambda: wall(dc.to_host))):
            fn()
            best[name] = round(1e3 * min(fn() for _ in range(5)), 3)
        wall(dc.ess)
        d = wall.last
        wall(dc.to_host)
        hc = min(C_, a.host_chains)
        data = np.ascontiguousarray(wall.last.as_array()[:hc, :, :1])
        t0 = time.perf_counter()
        host = F.ess_host(data)
        best["ess_host_sample_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        ml = F.McmcList([F.Mcmc(data[c], start=1, end=N, thin=1) for c in range(hc)])
        same = F.ess(ml)
        rel = max(abs(same.bulk[0] - host.bulk[0]) / host.bulk[0], abs(same.tail[0] - host.tail[0]) / host.tail[0])
        M = 2 * C_ * (N // 2)
        lines.append(dict(shape=shape, chains=C_, columns=k, rows=N, pooled_values=M,
                          work_bytes=8 * int(abi.lib().fmcmc_rank_ess_work_len(C_, k, N)), **best,
                          host_sample_chains=hc, host_sample_columns=1,
                          ess_bulk_min=float(np.nanmin(d.bulk)), ess_tail_min=float(np.nanmin(d.tail)),
                          pairs_kept_max=int(d.lags.max()), max_rel_diff_to_host_on_sample=float(rel)))
        print(json.dumps(lines[-1]), flush=True)
        del dc, data
        torch.cuda.empty_cache()
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_ess.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per shape one warm-up call, then the best of five; kernels: HIP events around the enqueued "
                                 "launches of one fmcmc_rank_ess_dev; wall: perf_counter around the synchronised call; "
                                 "ess_host: once, on one column of at most --host-chains chains", "shapes": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
