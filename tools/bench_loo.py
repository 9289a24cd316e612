"""Time of loo() on the device (fmcmc_amd/summary.py: loo -> csrc/diag_loo.hpp) next to waic() in the same process:
  * headline: bench.py's headline config (1024 chains x 10^4 kept rows of the BASELINE regression, n = 10^4, k = 5)
  * batch:    256 datasets x 4 chains x 2000 rows of a regression with n = 1000 (k = 4), seeded draws around the truth in an
              McmcBatch built by hand: the grouped call against the Python loop of single calls
Per shape, one warm-up call and then the best of three of: the enqueued kernels of one call between two HIP events, for loo
and for waic; the wall time of loo() and waic() including the copy back; once: the wall time of DeviceChains.to_host() (the
headline), the number of observations the exact fallback served, and the plan.
Usage: python tools/bench_loo.py [--shapes headline,batch] [--json FILE]   (one JSON line per shape)"""
import argparse
import ctypes as C
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
    ap.add_argument("--shapes", default="headline,batch")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import enqueue_loo_groups, enqueue_waic_groups, loo_plan
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

    def fallbacks(dm, G, Cm, N, work):
        cm = dm.c()
        off = int(abi.lib().fmcmc_loo_state_offset(C.byref(cm), G, Cm, N))
        st = work[off:off + 8 * G * dm.n].cpu().numpy().view(np.int64).reshape(-1, 8)
        return int(st[:, 3].sum())

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
            best = dict(loo_kernels_ms=best_of(lambda: events(lambda: enqueue_loo_groups(dc, dm, D, Cm, 0, rows))),
                        waic_kernels_ms=best_of(lambda: events(lambda: enqueue_waic_groups(dc, dm, D, Cm, 0, rows))),
                        loo_wall_ms=best_of(lambda: wall(lambda: ans.loo(models))),
                        waic_wall_ms=best_of(lambda: wall(lambda: ans.waic(models))),
                        loo_loop_wall_ms=best_of(lambda: wall(lambda: [F.loo(ans[d], models[d]) for d in range(D)]), 1))
            got, loop = ans.loo(models), [F.loo(ans[d], models[d]) for d in range(D)]
            same = all(np.array_equal(got[d].pointwise.view(np.uint64), loop[d].pointwise.view(np.uint64)) for d in range(D))
            work = enqueue_loo_groups(dc, dm, D, Cm, 0, rows)[2]
            lines.append(dict(shape=shape, datasets=D, chains=Cm, rows=rows, observations=n, k=p + 2, plan=vars(loo_plan(Cm, rows, n)),
                              work_bytes=8 * int(work.numel()), fallbacks=fallbacks(dm, D, Cm, rows, work), **best,
                              same_bits_as_the_loop=bool(same), max_k=float(got.max_k.max())))
            print(json.dumps(lines[-1]), flush=True)
            del work
            continue
        cfg = Config("c2")
        chains, nsteps = cfg.chains, 10000
        X, y, init = cfg.workload(chains, 0)
        model, kern = F.gaussian_linreg(X, y), F.kernel_normal(scale=0.02)
        dc = F.MCMC(init, model, nsteps, nchains=chains, seed=1215, kernel=kern, _return_device=True, keep_logpost=False,
                    keep_draws=False)
        C_, k, N = (int(v) for v in dc.samples.shape)
        dm = model.device_model(dc._samples.device)
        best = dict(loo_kernels_ms=best_of(lambda: events(lambda: enqueue_loo_groups(dc, dm, 1, C_, 0, N))),
                    waic_kernels_ms=best_of(lambda: events(lambda: enqueue_waic_groups(dc, dm, 1, C_, 0, N))),
                    loo_wall_ms=best_of(lambda: wall(lambda: dc.loo(model))),
                    waic_wall_ms=best_of(lambda: wall(lambda: dc.waic(model))))
        r, w = dc.loo(model), dc.waic(model)
        work = enqueue_loo_groups(dc, dm, 1, C_, 0, N)[2]
        torch.cuda.synchronize()
        nfall, wbytes = fallbacks(dm, 1, C_, N, work), 8 * int(work.numel())
        del work
        torch.cuda.empty_cache()
        best["to_host_wall_ms"] = round(1e3 * wall(dc.to_host), 1)
        lines.append(dict(shape=shape, chains=C_, rows=N, observations=dm.n, k=k, elements=C_ * N * dm.n, plan=vars(loo_plan(C_, N, dm.n)),
                          work_bytes=wbytes, fallbacks=nfall, **best, elpd_loo=r.elpd_loo, p_loo=r.p_loo, elpd_waic=w.elpd_waic,
                          p_waic=w.p_waic, max_k=r.max_k, n_k_bad=r.n_k_bad))
        print(json.dumps(lines[-1]), flush=True)
        del dc
        torch.cuda.empty_cache()
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_loo.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per shape one warm-up call, then the best of three (the loop: of one); kernels: HIP events around "
                                 "the enqueued launches of one call; wall: perf_counter around the synchronised call; to_host: once",
                       "shapes": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
