"""Step time of the callback path (batched_fun -> fmcmc_mcmc_run_fun_dev, mh_fun.hpp) for 1024 chains: microseconds per MH step
  * trivial: fn(theta) = -sum(theta^2) at k = 3 under kernel_normal -- the engine's own floor (one launch + one torch op per step)
  * mvn100:  the multivariate-normal mean of the reference's benchmark (playground/benchmarks.Rmd: k = 100, n = 500) under
             kernel_ram, fn in torch through the sufficient statistics of the data
Usage: python tools/bench_fun.py [--nsteps N] [--chains C] [--json FILE]   (one JSON line per case; --json also writes them, with
the device and the date, to FILE: profiles/bench_fun.json holds the run DESIGN.md section 5.9 quotes)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    Y = torch.tensor(rng.standard_normal((500, 100)) + np.linspace(-1, 1, 100)[None, :], dtype=torch.float64, device=dev)
    n, sy, syy = Y.shape[0], Y.sum(0), (Y * Y).sum()

    def mvn(th):   # sum_i log N(y_i | mu, I) up to a constant
        return -0.5 * (syy - 2.0 * (th @ sy) + n * (th * th).sum(1))

    cases = {"trivial": (lambda th: -(th * th).sum(1), 3, lambda: F.kernel_normal(scale=0.1)),
             "mvn100": (mvn, 100, lambda: F.kernel_ram(warmup=100))}
    lines = []
    for name, (fn, k, kern) in cases.items():
        init = (Y.mean(0)[:k].cpu().numpy()[None, :] if k == 100 else np.zeros((1, k))) + 0.01 * rng.standard_normal((a.chains, k))
        run = lambda ns: F.MCMC(init, F.batched_fun(fn, k), ns, nchains=a.chains, seed=7, kernel=kern(), _return_device=True,
                                keep_logpost=False, keep_draws=False)
        run(50)   # (warm-up: code objects, the caching allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(a.nsteps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines.append({"case": name, "k": k, "chains": a.chains, "nsteps": a.nsteps, "kernel": abi.last_kernel(),
                      "us_per_step": round(dt / a.nsteps * 1e6, 2)})
        print(json.dumps(lines[-1]), flush=True)
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_fun.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "wall clock of one call of nsteps steps after a 50-step warm-up call, synchronised",
                       "cases": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
