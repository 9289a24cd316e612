"""Time of waic() on the device (fmcmc_amd/summary.py: waic -> csrc/diag_waic.hpp) next to the route a user had before it:
  * headline: bench.py's headline config (1024 chains x 10^4 kept rows of the BASELINE regression, n = 10^4, k = 5)
  * logistic: a logistic model of the vignette's size (n = 100, three columns, prior_div = 8), 1024 chains x 10^4 rows
  * batch:    256 datasets x 4 chains x 2000 rows of a regression with n = 1000 (k = 4), seeded draws around the truth in an
              McmcBatch built by hand: the grouped call against the Python loop of single calls in the same process
Per shape, one warm-up call and then the best of five of: the four enqueued kernels of one call between two HIP events (the
tile kernel is all but a few microseconds of them); the wall time of waic() including the copy back.  Once: the
wall time of DeviceChains.to_host(), and of waic_host on a SLICE of the copied rows that the host can finish -- at most
--host-chains chains and --host-obs observations: the full matrix of the headline has 10^11 entries -- with the largest
difference between device and host on that slice in the metric |a - b| / max(1, |b|).
Usage: python tools/bench_waic.py [--shapes headline,logistic,batch] [--host-chains 64] [--host-obs 64] [--json FILE]
(one JSON line per shape; --json also writes them, with the device and the date, to FILE)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_of(fn, n=5):
    fn()
    return round(1e3 * min(fn() for _ in range(n)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,logistic,batch")
    ap.add_argument("--host-chains", type=int, default=64)
    ap.add_argument("--host-obs", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import ctypes as C
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import enqueue_waic_groups, waic_parts
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

    for shape in a.shapes.split(","):
        if shape == "batch":
            D, Cm, rows, n, p = 256, 4, 2000, 1000, 2
            rng = np.random.default_rng(7)
            Xs = rng.uniform(-2, 2, (D, n, p))
            beta = np.array([0.5, 1.0, -1.0])
            ys = beta[0] + Xs @ beta[1:] + rng.standard_normal((D, n))
            models = F.model_batch(F.gaussian_linreg(Xs[d], ys[d]) for d in range(D))
            g = torch.Generator(device="cpu").manual_seed(3)
            x = torch.as_tensor(np.concatenate([beta, [1.0]]))[None, :, None] + 0.05 * torch.randn((D * Cm, p + 2, rows), generator=g,
                                                                                                   dtype=torch.float64)
            dc = F.DeviceChains(x.cuda(), None, None, np.arange(1, rows + 1), 1, None, 0, D * Cm)
            ans = F.McmcBatch(dc, D, Cm)
            dm = models.device_model(dev)
            best = dict(kernels_ms=best_of(lambda: events(lambda: enqueue_waic_groups(dc, dm, D, Cm, 0, rows))),
                        waic_wall_ms=best_of(lambda: wall(lambda: ans.waic(models))),
                        loop_wall_ms=best_of(lambda: wall(lambda: [F.waic(ans[d], models[d]) for d in range(D)]), 2))
            got, loop = ans.waic(models), [F.waic(ans[d], models[d]) for d in range(D)]
            same = all(np.array_equal(got[d].pointwise.view(np.uint64), loop[d].pointwise.view(np.uint64)) for d in range(D))
            cm = dm.c()
            lines.append(dict(shape=shape, datasets=D, chains=Cm, rows=rows, observations=n, k=p + 2,
                              parts=waic_parts(Cm, rows, n)[1], work_bytes=8 * int(abi.lib().fmcmc_waic_work_len(C.byref(cm), D, Cm, rows)),
                              **best, same_bits_as_the_loop=bool(same)))
            print(json.dumps(lines[-1]), flush=True)
            continue
        cfg = Config("c2")
        chains, nsteps = cfg.chains, 10000
        if shape == "headline":
            X, y, init = cfg.workload(chains, 0)
            model, kern = F.gaussian_linreg(X, y), F.kernel_normal(scale=0.02)
        else:
            rng = np.random.default_rng(11)
            n = 100
            X = np.column_stack([np.ones(n), rng.standard_normal((n, 2))])
            y = (rng.uniform(size=n) < 1 / (1 + np.exp(-(X @ np.array([0.5, 1.0, -1.0]))))).astype(np.float64)
            model, kern = F.logistic(X, y, prior_div=8.0), F.kernel_normal(scale=0.1)
            init = np.zeros(3)
        dc = F.MCMC(init, model, nsteps, nchains=chains, seed=1215, kernel=kern, _return_device=True, keep_logpost=False,
                    keep_draws=False)
        C_, k, N = (int(v) for v in dc.samples.shape)
        dm = model.device_model(dc._samples.device)
        n = dm.n
        best = dict(kernels_ms=best_of(lambda: events(lambda: enqueue_waic_groups(dc, dm, 1, C_, 0, N))),
                    waic_wall_ms=best_of(lambda: wall(lambda: dc.waic(model))))
        w = dc.waic(model)
        best["to_host_wall_ms"] = round(1e3 * wall(dc.to_host), 1)
        hc, ho = min(C_, a.host_chains), min(n, a.host_obs)
        draws = np.ascontiguousarray(wall.last.as_array()[:hc].reshape(hc * N, k))
        sub = (F.gaussian_linreg(model.X[:ho], model.y[:ho]) if shape == "headline" else F.logistic(model.X[:ho], model.y[:ho]))
        t0 = time.perf_counter()
        host = F.waic_host(sub, draws)
        best["waic_host_slice_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        sl = F.DeviceChains(dc._samples[:hc], None, None, dc.iters, dc.thin, None, 0, hc, nrows=N)
        same = F.waic(sl, sub)
        rel = np.max(np.abs(same.pointwise - host.pointwise) / np.maximum(1.0, np.abs(host.pointwise)))
        cm = dm.c()
        lines.append(dict(shape=shape, chains=C_, rows=N, observations=n, k=k, elements=C_ * N * n, parts=waic_parts(C_, N, n)[1],
                          work_bytes=8 * int(abi.lib().fmcmc_waic_work_len(C.byref(cm), 1, C_, N)), **best,
                          host_slice_chains=hc, host_slice_observations=ho,
                          host_slice_share_of_the_elements=hc * ho / (C_ * n), elpd_waic=w.elpd_waic, p_waic=w.p_waic,
                          n_high=w.n_high, max_diff_to_host_on_slice=float(rel)))
        print(json.dumps(lines[-1]), flush=True)
        del dc, draws, sl
        torch.cuda.empty_cache()
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_waic.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per shape one warm-up call, then the best of five (the loop: of two); kernels: HIP events around "
                                 "the four enqueued launches of one call; wall: perf_counter around the synchronised call; "
                                 "to_host and waic_host: once, waic_host on the slice named in the line", "shapes": lines}, f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
