"""Time of predictive() on the device (fmcmc_amd/summary.py: predictive -> csrc/diag_predictive.hpp) at bench.py's headline config
(1024 chains x 10^4 kept rows of the BASELINE regression, k = 5), in the style of tools/bench_predict.py:
  * m = 10^4: the model's own points and y;  m = 100: its first 100 rows as newdata with their y
  * the PIT-only call (no probs: the draw pass, the fold, one evaluation pass with one slot) and the call with the three default
    probs (the same, then evaluation passes with three slots in rounds until every quantile has finished)
Per line, one warm-up call and then the best of --reps of the wall time of predictive() including the copies back and the
synchronisation after every round; pass_kernels_ms is one evaluation pass of the three probs between two HIP events (a resumed call
of one pass on a fresh state, so that nothing has finished), passes the number of passes that were run and finished_by the largest
pass at which a quantile finished.  In the same process, once per m: the wall time of predict() with the same probs, of waic()
(m = the model's own points only) and of DeviceChains.to_host().
Usage: python tools/bench_predictive.py [--points 10000,100] [--reps 3] [--json FILE]
(one JSON line per (m, probs); --json also writes them, with the device and the date, to FILE)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="10000,100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import ctypes as C
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.engine import DeviceModel
    from fmcmc_amd.summary import enqueue_predictive, waic_parts
    from bench import Config
    dev = torch.device("cuda", 0)
    lines = []

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wall.last = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def best_of(fn):
        fn()
        return round(1e3 * min(fn() for _ in range(a.reps)), 3)

    cfg = Config("c2")
    chains, nsteps = cfg.chains, 10000
    X, y, init = cfg.workload(chains, 0)
    model = F.gaussian_linreg(X, y)
    dc = F.MCMC(init, model, nsteps, nchains=chains, seed=1215, kernel=F.kernel_normal(scale=0.02), _return_device=True,
                keep_logpost=False, keep_draws=False)
    C_, k, N = (int(v) for v in dc.samples.shape)
    to_host_ms = round(1e3 * wall(dc.to_host), 1)
    wall.last = None
    probs3 = (0.025, 0.5, 0.975)
    for m in (int(v) for v in a.points.split(",")):
        new, yn = model.X[:m], model.y[:m]
        dm = DeviceModel(model.family, new, yn, model.intercept, model.guard, model.prior_div, device=dev)
        predict_ms = best_of(lambda: wall(lambda: F.predict(dc, model, new, probs3)))
        waic_ms = best_of(lambda: wall(lambda: F.waic(dc, model))) if m == model.y.shape[0] else None

        def one_pass():
            state = enqueue_predictive(dc, dm, 0, N, probs3, 1)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            enqueue_predictive(dc, dm, 0, N, probs3, 1, True, state)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        pass_ms = best_of(one_pass)
        for probs in ((), probs3):
            ms = best_of(lambda: wall(lambda: F.predictive(dc, model, new, yn, probs)))
            r = wall.last
            cm = dm.c()
            lines.append(dict(points=m, nprobs=len(probs), chains=C_, rows=N, k=k, elements=C_ * N * m,
                              parts=waic_parts(C_, N, m)[1],
                              work_bytes=8 * int(abi.lib().fmcmc_predictive_work_len(C.byref(cm), C_, N, len(probs))),
                              predictive_wall_ms=ms, pass_kernels_ms=pass_ms, passes=r.total_passes,
                              finished_by=int(r.passes.max()) if probs else 0, converged=bool(r.converged.all()),
                              predict_wall_ms=predict_ms, waic_wall_ms=waic_ms, to_host_wall_ms=to_host_ms,
                              mean_sd_pred=float(r.sd_pred.mean()), mean_pit=float(r.pit.mean()),
                              coverage_95=r.coverage(0.025, 0.975) if probs else None))
            print(json.dumps(lines[-1]), flush=True)
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_predictive.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per line one warm-up call, then the best of --reps (%d); wall: perf_counter around the "
                                 "synchronised call; pass_kernels_ms: HIP events around one resumed call of one pass with three "
                                 "probs on a state in which nothing has finished; to_host: once" % a.reps, "lines": lines}, f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
