"""Time of predict() on the device (fmcmc_amd/summary.py: predict -> csrc/diag_predict.hpp) next to the route a user had before
it, at bench.py's headline config (1024 chains x 10^4 kept rows of the BASELINE regression, k = 5):
  * m = 10^4: the fitted values at the model's own X;  m = 100: its first 100 rows as newdata
  * with the three default probs (six ranks, one batch of the select: eight passes over all draws) and with none (the fold alone)
Per line, one warm-up call and then the best of three of: every enqueued kernel of one call between two HIP events; the wall time
of predict() including the copy back.  fold_kernels_ms is the events time of the call without probs (the draw kernel, the fold
pass, the finish: the fold pass is all but a few microseconds of them); select_kernels_ms is the events time of the call with
probs less that: the eight histogram passes and their scans.  Once: the wall time of DeviceChains.to_host(), and of predict_host
on a SLICE of the copied rows that the host can finish -- at most --host-chains chains and --host-points points: the full matrix
at m = 10^4 has 10^11 entries -- with the largest difference between device and host on that slice in the metric
|a - b| / max(1, |b|).
Usage: python tools/bench_predict.py [--points 10000,100] [--host-chains 16] [--host-points 64] [--json FILE]
(one JSON line per (m, probs); --json also writes them, with the device and the date, to FILE)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_of(fn, n=3):
    fn()
    return round(1e3 * min(fn() for _ in range(n)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="10000,100")
    ap.add_argument("--host-chains", type=int, default=16)
    ap.add_argument("--host-points", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import ctypes as C
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.engine import DeviceModel
    from fmcmc_amd.summary import enqueue_predict, waic_parts
    from bench import Config
    dev = torch.device("cuda", 0)
    lines = []

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wall.last = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        keep = fn()
        e1.record()
        e1.synchronize()
        del keep
        return e0.elapsed_time(e1) * 1e-3

    cfg = Config("c2")
    chains, nsteps = cfg.chains, 10000
    X, y, init = cfg.workload(chains, 0)
    model = F.gaussian_linreg(X, y)
    dc = F.MCMC(init, model, nsteps, nchains=chains, seed=1215, kernel=F.kernel_normal(scale=0.02), _return_device=True,
                keep_logpost=False, keep_draws=False)
    C_, k, N = (int(v) for v in dc.samples.shape)
    to_host_ms = round(1e3 * wall(dc.to_host), 1)
    hc = min(C_, a.host_chains)
    draws = np.ascontiguousarray(wall.last.as_array()[:hc].reshape(hc * N, k))
    sl = F.DeviceChains(dc._samples[:hc], None, None, dc.iters, dc.thin, None, 0, hc, nrows=N)
    for m in (int(v) for v in a.points.split(",")):
        new = model.X[:m]
        dm = DeviceModel(model.family, new, np.zeros(m), model.intercept, model.guard, model.prior_div, device=dev)
        fold_ms = best_of(lambda: events(lambda: enqueue_predict(dc, dm, 0, N, "epred", ())))
        for probs in ((0.025, 0.5, 0.975), ()):
            best = dict(kernels_ms=best_of(lambda: events(lambda: enqueue_predict(dc, dm, 0, N, "epred", probs))),
                        fold_kernels_ms=fold_ms)
            best["select_kernels_ms"] = round(best["kernels_ms"] - fold_ms, 3) if probs else 0.0
            best["predict_wall_ms"] = best_of(lambda: wall(lambda: F.predict(dc, model, new, probs)))
            r = F.predict(dc, model, new, probs)
            ho = min(m, a.host_points)
            t0 = time.perf_counter()
            host = F.predict_host(model, draws, new[:ho], probs)
            host_ms = round(1e3 * (time.perf_counter() - t0), 1)
            same = F.predict(sl, model, new[:ho], probs)
            rel = np.max(np.abs(same.point_dev.cpu().numpy() - host.point) / np.maximum(1.0, np.abs(host.point)))
            cm = dm.c()
            lines.append(dict(points=m, nprobs=len(probs), chains=C_, rows=N, k=k, elements=C_ * N * m,
                              parts=waic_parts(C_, N, m)[1],
                              work_bytes=8 * int(abi.lib().fmcmc_predict_work_len(C.byref(cm), C_, N, len(probs))), **best,
                              to_host_wall_ms=to_host_ms, predict_host_slice_ms=host_ms, host_slice_chains=hc,
                              host_slice_points=ho, host_slice_share_of_the_elements=hc * ho / (C_ * m),
                              mean_sd=float(r.sd.mean()), mean_sd_pred=float(r.sd_pred.mean()),
                              max_diff_to_host_on_slice=float(rel)))
            print(json.dumps(lines[-1]), flush=True)
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_predict.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per line one warm-up call, then the best of three; kernels: HIP events around every enqueued "
                                 "launch of one call; fold: the call without probs; select: the difference; wall: perf_counter "
                                 "around the synchronised call; to_host and predict_host: once, predict_host on the slice named "
                                 "in the line", "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
