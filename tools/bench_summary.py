"""Time of the device-side summary (fmcmc_amd/summary.py -> csrc/summary.hip) next to the copy it makes unnecessary, on the
output of two of bench.py's configs:
  * headline (c2): 1024 chains x 5 parameters x 10^4 kept rows, kernel_normal(scale = 0.02)
  * c4:            512 chains x 50 parameters x 5000 kept rows, kernel_ram()
Per shape, one warm-up call and then the best of five of: the enqueued kernels of summary() between two HIP events; the wall
time of summary() including the small copy back; the wall time of DeviceChains.to_host() of the same rows in the same process.
At the headline shape also heidel(): its enqueued kernels between two HIP events, its wall time, and the only other route to
the same table: to_host() plus convergence.heidel_diag chain by chain, timed on --heidel-host-chains chains and scaled to all.
And raftery_diag() (the `raftery` leg): the one kernel of fmcmc_raftery_dev for the first batch of thinnings between two HIP
events, the wall time of the whole call with its copy back and numpy finish, the number of launches it took, the kernel and wall
of chain_quantiles() at the default five probs, and convergence.raftery_diag on the host for --heidel-host-chains chains.
And the posterior leg: the kernel and the wall time of hpd_interval() at prob 0.95, of autocorr_diag() at coda's five default
lags and of crosscorr() (the Gelman reduction over all rows), beside the same to_host().
Usage: python tools/bench_summary.py [--shapes headline,c4] [--json FILE]   (one JSON line per shape; --json also writes them, with
the device and the date, to FILE: profiles/bench_summary.json holds the run DESIGN.md section 5.10 quotes, and
profiles/bench_summary_heidel.json the headline run with heidel(), profiles/bench_summary_raftery.json the one with the
raftery leg, profiles/bench_summary_posterior.json the one with the posterior leg)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"headline": ("c2", 10000), "c4": ("c4", 5000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,c4")
    ap.add_argument("--json", default=None)
    ap.add_argument("--heidel-host-chains", type=int, default=4)
    a = ap.parse_args()
    import torch
    import fmcmc_amd as F
    import importlib
    S = importlib.import_module("fmcmc_amd.summary")     # (fmcmc_amd.summary is the function)
    from fmcmc_amd.summary import DEFAULT_QUANTILES, enqueue_heidel, enqueue_window, heidel_candidates
    from bench import Config
    dev = torch.device("cuda", 0)
    lines = []
    for shape in a.shapes.split(","):
        cname, nsteps = SHAPES[shape]
        cfg = Config(cname)
        X, y, init = cfg.workload(cfg.chains, 0)
        kern = F.kernel_normal(scale=0.02) if cname == "c2" else F.kernel_ram()
        dc = F.MCMC(init, F.gaussian_linreg(X, y), nsteps, nchains=cfg.chains, seed=1215, kernel=kern, _return_device=True,
                    keep_logpost=False, keep_draws=False)
        C_, k, N = (int(v) for v in dc.samples.shape)

        def between_events(enqueue):
            """seconds between two HIP events around what `enqueue` launches (its tensors live until the second has passed)"""
            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                keep = enqueue()
                e1.record()
                e1.synchronize()
                del keep
                return e0.elapsed_time(e1) * 1e-3
            return run

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        best = {}
        for name, fn in (("summary_kernels_ms", between_events(lambda: enqueue_window(dc, 0, N, None, DEFAULT_QUANTILES))),
                         ("summary_wall_ms", lambda: wall(dc.summary)),
                         ("to_host_wall_ms", lambda: wall(dc.to_host))):
            fn()
            best[name] = round(1e3 * min(fn() for _ in range(5)), 3)
        if shape == "headline":
            _, rows, half = heidel_candidates(dc.iters)
            for name, fn in (("heidel_kernels_ms", between_events(lambda: enqueue_heidel(dc, half, rows, None))),
                             ("heidel_wall_ms", lambda: wall(dc.heidel))):
                fn()
                best[name] = round(1e3 * min(fn() for _ in range(5)), 3)
            host = dc.samples[:a.heidel_host_chains].cpu().numpy()
            t0 = time.perf_counter()
            for c in range(host.shape[0]):
                F.heidel_diag(host[c].T, dc.iters)
            per_chain = (time.perf_counter() - t0) / host.shape[0]
            best.update(heidel_candidates=int(rows.size), heidel_diag_host_ms_per_chain=round(1e3 * per_chain, 3),
                        heidel_host_route_ms=round(best["to_host_wall_ms"] + 1e3 * per_chain * C_, 1))
            # the raftery leg
            ranks = S.type7_order_ranks(N, DEFAULT_QUANTILES).ravel()
            launches = []
            real = S.enqueue_raftery
            S.enqueue_raftery = lambda *args: launches.append(args[2]) or real(*args)
            try:
                rd = dc.raftery_diag()
            finally:
                S.enqueue_raftery = real
            for name, fn in (("raftery_kernel_ms", between_events(lambda: S.enqueue_raftery(dc, 0.025, 1, S.RAFTERY_BATCH, None))),
                             ("raftery_wall_ms", lambda: wall(dc.raftery_diag)),
                             ("chain_order_kernel_ms", between_events(lambda: S.enqueue_chain_order(dc, ranks, None))),
                             ("chain_quantiles_wall_ms", lambda: wall(dc.chain_quantiles))):
                fn()
                best[name] = round(1e3 * min(fn() for _ in range(5)), 3)
            t0 = time.perf_counter()
            for c in range(host.shape[0]):
                F.raftery_diag(host[c].T, dc.iters)
            per_chain = (time.perf_counter() - t0) / host.shape[0]
            best.update(raftery_launches=len(launches), raftery_thinnings_per_launch=S.RAFTERY_BATCH,
                        raftery_kthin_max=float(np.nanmax(rd.kthin)), raftery_I_median=round(float(np.nanmedian(rd.I)), 3),
                        raftery_diag_host_ms_per_chain=round(1e3 * per_chain, 3),
                        raftery_host_route_ms=round(best["to_host_wall_ms"] + 1e3 * per_chain * C_, 1))
            # the posterior leg: hpd_interval(), autocorr_diag() and crosscorr(), kernels between two HIP events and the calls' wall
            for name, fn in (("hpd_kernel_ms", between_events(lambda: S.enqueue_hpd(dc, S.hpd_gap(N, 0.95), None))),
                             ("hpd_wall_ms", lambda: wall(dc.hpd_interval)),
                             ("autocov_kernel_ms", between_events(lambda: S.enqueue_autocov(dc, S.DEFAULT_LAGS, None))),
                             ("autocorr_wall_ms", lambda: wall(dc.autocorr_diag)),
                             ("crosscorr_kernels_ms", between_events(lambda: S.enqueue_gelman(dc, 0, N, None))),
                             ("crosscorr_wall_ms", lambda: wall(dc.crosscorr))):
                fn()
                best[name] = round(1e3 * min(fn() for _ in range(5)), 3)
            del host
        nbytes = C_ * k * N * 8
        lines.append(dict(shape=shape, chains=C_, columns=k, rows=N, sample_bytes=nbytes, quantiles=len(DEFAULT_QUANTILES), **best,
                          read_gbs_of_9_passes=round(9 * nbytes / best["summary_kernels_ms"] * 1e-6, 1)))
        print(json.dumps(lines[-1]), flush=True)
        del dc
        torch.cuda.empty_cache()
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_summary.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "per shape one warm-up call, then the best of five; kernels: HIP events around the enqueued "
                                 "launches of one summary(); wall: perf_counter around the synchronised call",
                       "shapes": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
