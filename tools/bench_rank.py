"""Time of the rank-normalised split R-hat on the device (fmcmc_amd/summary.py: rhat -> csrc/diag_rank.hpp) next to the two
routes a user had before it, on the output of bench.py's headline config (kernel_normal(scale = 0.02)):
  * headline: 1024 chains x 5 parameters x 10^4 kept rows (M = 1.024 x 10^7 pooled values a column)
  * small:    4 chains x 5 parameters x 2000 kept rows
Per shape, one warm-up call and then the best of five of: the enqueued kernels of one fmcmc_rank_rhat_dev call between two HIP
events; the wall time of rhat() including the small copy back and the finish; the wall time of gelman_diag(autoburnin = False)
on the same rows; the wall time of DeviceChains.to_host() of the same rows.  Once: convergence.rhat_host on the copied rows
(scipy's rankdata and ndtri), which with to_host() is the host route, and the largest difference between the two results.
Usage: python tools/bench_rank.py [--shapes headline,small] [--json FILE]   (one JSON line per shape; --json also writes them,
with the device and the date, to FILE: profiles/bench_rank.json holds the run DESIGN.md section 5.10 quotes)"""
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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import enqueue_rank_rhat
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
            keep = enqueue_rank_rhat(dc, 0, N, None)
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
        for name, fn in (("rhat_kernels_ms", kernels), ("rhat_wall_ms", lambda: wall(dc.rhat)),
                         ("gelman_diag_wall_ms", lambda: wall(lambda: dc.gelman_diag(autoburnin=False))),
                         ("to_host_wall_ms", lambda: wall(dc.to_host))):
            fn()
            best[name] = round(1e3 * min(fn() for _ in range(5)), 3)
        wall(dc.rhat)
        d = wall.last
        wall(dc.to_host)
        data = wall.last.as_array()
        t0 = time.perf_counter()
        host = F.rhat_host(data)
        best["rhat_host_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        best["host_route_ms"] = round(best["to_host_wall_ms"] + best["rhat_host_ms"], 1)
        M = 2 * C_ * (N // 2)
        lines.append(dict(shape=shape, chains=C_, columns=k, rows=N, pooled_values=M,
                          work_bytes=8 * int(abi.lib().fmcmc_rank_work_len(C_, k, N)), **best,
                          sorted_pairs_per_s=round(2 * k * M / (best["rhat_kernels_ms"] * 1e-3), 0),
                          rhat_max=float(np.nanmax(d.rhat)), max_abs_diff_to_host=float(np.nanmax(np.abs(d.rhat - host.rhat)))))
        print(json.dumps(lines[-1]), flush=True)
        del dc, data
        torch.cuda.empty_cache()
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_rank.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per shape one warm-up call, then the best of five; kernels: HIP events around the enqueued "
                                 "launches of one fmcmc_rank_rhat_dev; wall: perf_counter around the synchronised call; "
                                 "rhat_host: once", "shapes": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
