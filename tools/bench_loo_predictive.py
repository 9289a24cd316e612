"""Time of loo_predictive() on the device (fmcmc_amd/summary.py: loo_predictive -> csrc/diag_loo_predictive.hpp) at bench.py's
headline config (1024 chains x 10^4 kept rows of the BASELINE regression, k = 5), in the style of tools/bench_predictive.py:
  * n = 10^4: the model itself;  n = 100: the model of its first 100 observations
Per line, one warm-up call and then the best of --reps of the wall time, including the copies back, of loo_predictive(), of
loo() and of predictive() with no probs (the PIT alone: the in-sample counterpart of the LOO-PIT), all from the same process and
the same draws; extra_kernels_ms is what the call enqueues behind the kernels of loo() (the run means, the expectation sweep, the
finish), between two HIP events: the whole raw call minus a raw fmcmc_loo_dev call.
Usage: python tools/bench_loo_predictive.py [--obs 10000,100] [--reps 3] [--json FILE]
(one JSON line per n; --json also writes them, with the device and the date, to FILE)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", default="10000,100")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import ctypes as C
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import enqueue_loo_groups, enqueue_loo_predictive, waic_parts
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
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def best_of(fn):
        fn()
        return round(1e3 * min(fn() for _ in range(a.reps)), 3)

    cfg = Config("c2")
    chains, nsteps = cfg.chains, 10000
    X, y, init = cfg.workload(chains, 0)
    full = F.gaussian_linreg(X, y)
    dc = F.MCMC(init, full, nsteps, nchains=chains, seed=1215, kernel=F.kernel_normal(scale=0.02), _return_device=True,
                keep_logpost=False, keep_draws=False)
    C_, k, N = (int(v) for v in dc.samples.shape)
    for n in (int(v) for v in a.obs.split(",")):
        model = full if n == full.y.shape[0] else F.gaussian_linreg(full.X[:n], full.y[:n])
        dm = model.device_model(dev)
        lp_ms = best_of(lambda: wall(lambda: F.loo_predictive(dc, model)))
        r = wall.last
        loo_ms = best_of(lambda: wall(lambda: F.loo(dc, model)))
        pit_ms = best_of(lambda: wall(lambda: F.predictive(dc, model, probs=())))
        insample = wall.last
        raw_lp = best_of(lambda: events(lambda: enqueue_loo_predictive(dc, dm, 0, N)))
        raw_loo = best_of(lambda: events(lambda: enqueue_loo_groups(dc, dm, 1, C_, 0, N)))
        cm = dm.c()
        m = r.metrics()
        lines.append(dict(obs=n, chains=C_, rows=N, k=k, elements=C_ * N * n, tail=r.loo.tail_len, parts=waic_parts(C_, N, n)[1],
                          work_bytes=8 * int(abi.lib().fmcmc_loo_predictive_work_len(C.byref(cm), C_, N)),
                          loo_work_bytes=8 * int(abi.lib().fmcmc_loo_work_len(C.byref(cm), 1, C_, N)),
                          loo_predictive_wall_ms=lp_ms, loo_wall_ms=loo_ms, predictive_pit_wall_ms=pit_ms,
                          call_kernels_ms=raw_lp, loo_kernels_ms=raw_loo, extra_kernels_ms=round(raw_lp - raw_loo, 3),
                          bad_points=r.bad_points, max_k=r.loo.max_k, r2=m["r2"], rmse=m["rmse"], coverage_90=r.coverage(0.9),
                          mean_abs_pit_shift=float(abs(r.pit - insample.pit).mean())))
        print(json.dumps(lines[-1]), flush=True)
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_loo_predictive.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per line one warm-up call, then the best of --reps (%d); wall: perf_counter around the "
                                 "synchronised call; *_kernels_ms: HIP events around the raw entry (allocation of its buffers "
                                 "included)" % a.reps, "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
