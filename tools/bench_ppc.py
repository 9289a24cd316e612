"""Time of ppc() on the device (fmcmc_amd/summary.py: ppc -> csrc/diag_ppc.hpp), in the style of tools/bench_predictive.py, in one
run at two shapes:
  * headline: bench.py's headline config (1024 chains x 10^4 kept rows of the BASELINE regression, k = 5, n = 10^4 observations):
    10^11 replicated observations
  * small: 4 chains x 2000 rows x the first 1000 observations
Per shape, one warm-up call and then the best of --reps of the wall time of ppc() including the copy back of `total` and the
synchronisation; kernels_ms is the whole fmcmc_ppc_dev call between two HIP events.  In the same process: the wall time of waic()
and of DeviceChains.to_host(), and eval_pass_kernels_ms, one evaluation pass of predictive() with three probs between two HIP
events (the nearest yardstick: the same tiles, one Phi per element where ppc() has half a Philox block and one qnorm).
Usage: python tools/bench_ppc.py [--shapes headline,small] [--reps 3] [--json FILE]
(one JSON line per shape; --json also writes them, with the device and the date, to FILE)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,small")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import fmcmc_amd as F
    from fmcmc_amd.summary import enqueue_ppc, enqueue_predictive, ppc_observed
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

    def events(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    cfg = Config("c2")
    shapes = {"headline": (cfg.chains, 10000, None), "small": (4, 2000, 1000)}
    for name in a.shapes.split(","):
        chains, nsteps, nobs = shapes[name]
        X, y, init = cfg.workload(chains, 0)
        if nobs is not None:
            X, y = X[:nobs], y[:nobs]
        model = F.gaussian_linreg(X, y)
        dc = F.MCMC(init, model, nsteps, nchains=chains, seed=1215, kernel=F.kernel_normal(scale=0.02), _return_device=True,
                    keep_logpost=False, keep_draws=False)
        C_, k, N = (int(v) for v in dc.samples.shape)
        n = int(model.y.shape[0])
        dm = model.device_model(dev)
        tobs = ppc_observed(model)
        to_host_ms = round(1e3 * wall(dc.to_host), 1)
        wall.last = None
        ppc_ms = best_of(lambda: wall(lambda: F.ppc(dc, model)))
        r = wall.last
        kernels_ms = best_of(lambda: events(lambda: enqueue_ppc(dc, dm, 0, N, 1, tobs)))
        waic_ms = best_of(lambda: wall(lambda: F.waic(dc, model)))
        probs3 = (0.025, 0.5, 0.975)

        def one_pass():
            state = enqueue_predictive(dc, dm, 0, N, probs3, 1)
            return events(lambda: enqueue_predictive(dc, dm, 0, N, probs3, 1, True, state))

        pass_ms = best_of(one_pass)
        lines.append(dict(shape=name, chains=C_, rows=N, k=k, observations=n, elements=C_ * N * n, ppc_wall_ms=ppc_ms,
                          kernels_ms=kernels_ms, ns_per_element=round(1e6 * kernels_ms / (C_ * N * n), 6),
                          eval_pass_kernels_ms=pass_ms, waic_wall_ms=waic_ms, to_host_wall_ms=to_host_ms,
                          pvalue={s: round(v, 4) for s, v in r.pvalue.items()}))
        print(json.dumps(lines[-1]), flush=True)
        del dc, r
        wall.last = None
        torch.cuda.empty_cache()
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_ppc.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per line one warm-up call, then the best of --reps (%d); wall: perf_counter around the "
                                 "synchronised call; kernels_ms and eval_pass_kernels_ms: HIP events around the enqueued call; "
                                 "to_host: once" % a.reps, "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
