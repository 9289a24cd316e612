"""Step time of one model on many datasets (engine.sweep_batch -> fmcmc_mcmc_run_batch_dev, mh_batch.hpp) against the job as
it is done without it: D datasets x C chains of the README's regression (linreg, n observations, p covariates), microseconds
per MH step of ALL D x C chains
  * batch:  one sweep_batch call, under kernel_normal and kernel_ram, the dataset in LDS ("batch-lds") and streamed
            ("batch-stream"); device events around the call and the wall clock to its synchronise
  * loop:   D engine.sweep calls, one per dataset's DeviceModel (C chains each: the latency form), enqueued back to back on one
            stream, wall clock to the synchronise behind the last
Both after a 50-step warm-up of every shape and every dataset.  The loop runs code that mh_batch.hpp does not touch:
--loop-only times it alone (FMCMC_AMD_LIB selects another build of the library, e.g. the parent commit's), and --parent-loop
FILE merges the figures of such a run into this one's JSON.
Usage: python tools/bench_batch.py [--datasets D] [--chains C] [--n N] [--p P] [--nsteps S] [--loop-only] [--parent-loop FILE]
                                   [--json FILE]   (profiles/bench_batch.json holds the run DESIGN.md section 5.11 quotes)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", type=int, default=256)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--parent-loop", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from fmcmc_amd import _abi as abi
    from fmcmc_amd import engine as E
    D, Cm, n, p, k = a.datasets, a.chains, a.n, a.p, a.p + 2
    rng = np.random.default_rng(1)
    beta = np.linspace(1.0, -1.0, p + 1)
    Xs = rng.standard_normal((D, n, p))
    ys = beta[0] + Xs @ beta[1:] + 2.0 * rng.standard_normal((D, n))
    init = np.array(list(beta) + [2.0])[None, :] + 0.05 * rng.standard_normal((D * Cm, k))
    init[:, -1] = np.abs(init[:, -1]) + 0.5
    unb, free = np.full(k, 1e308), np.zeros(k, np.uint8)
    kernels = {"kernel_normal": lambda: E.KernelSpec(abi.KERNEL_NORMAL, k, np.zeros(k), np.full(k, 0.05), -unb, unb, free),
               "kernel_ram": lambda: E.KernelSpec(abi.KERNEL_RAM, k, np.zeros(k), np.ones(k), -unb, unb, free)}
    kw = dict(seed=7, want_logpost=False, want_draws=False, want_bits=False, check=False)
    lines = []

    def record(**line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    models = [E.DeviceModel(abi.FAM_GAUSSIAN_LINREG, Xs[d], ys[d]) for d in range(D)]
    batch = None if a.loop_only else E.DeviceModelBatch(abi.FAM_GAUSSIAN_LINREG, Xs, ys)
    for name, spec in kernels.items():
        gk = spec()

        def loop(ns):
            sts = [E.ChainState(init[d * Cm:(d + 1) * Cm], gk.kf) for d in range(D)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for d in range(D):
                E.sweep(models[d], gk, sts[d], ns, chain_base=d * Cm, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        loop(50)
        dt = loop(a.nsteps)
        loop_us = dt / a.nsteps * 1e6
        record(case="loop", kernel=name, form=abi.last_kernel(), datasets=D, chains_per_dataset=Cm, n=n, p=p, nsteps=a.nsteps,
               us_per_step=round(loop_us, 2))
        if a.loop_only:
            continue
        for stream_data in (False, True):
            def one(ns):
                st = E.ChainState(init, gk.kf)
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev0.record()
                E.sweep_batch(batch, gk, st, ns, stream_data=stream_data, **kw)
                ev1.record()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, ev0.elapsed_time(ev1) * 1e-3

            one(50)
            wall, dev_s = one(a.nsteps)
            us = wall / a.nsteps * 1e6
            record(case="batch", kernel=name, form=abi.last_kernel(), datasets=D, chains_per_dataset=Cm, n=n, p=p, nsteps=a.nsteps,
                   us_per_step=round(us, 2), us_per_step_device_events=round(dev_s / a.nsteps * 1e6, 2),
                   loop_over_batch=round(loop_us / us, 2))
    if a.json:
        props = torch.cuda.get_device_properties(0)
        doc = {"tool": "tools/bench_batch.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": props.name,
               "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
               "timing": "us per MH step of all datasets x chains: one call of nsteps steps (loop: one call per dataset, back to back) "
                         "after a 50-step warm-up of the same calls, wall clock to the synchronise; device events around the batch call",
               "cases": lines}
        if a.parent_loop:
            with open(a.parent_loop) as f:
                doc["loop_at_parent_commit"] = [c for c in json.load(f)["cases"] if c["case"] == "loop"]
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
