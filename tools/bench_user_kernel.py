"""Step time of a user-defined transition kernel (kernel_new -> fmcmc_mcmc_run_user_dev, mh_user.hpp) for 1024 chains:
microseconds per MH step
  * fun_builtin:   fn(theta) = -sum(theta^2) at k = 3 under the built-in kernel_normal through batched_fun -- the existing
                   callback path (tools/bench_fun.py, "trivial"), the comparison
  * fun_user:      the same fn under a kernel_new restatement of kernel_normal with env.rnorm
  * linreg_user:   the same user kernel on gaussian_linreg at the headline data (n = 10^4, k = 5), evaluated by the engine
  * logpost_call:  one DeviceModel.logpost call on those data, 1024 parameter vectors (microseconds per call)
Usage: python tools/bench_user_kernel.py [--nsteps N] [--chains C] [--json FILE]   (one JSON line per case; --json also writes
them, with the device and the date, to FILE: profiles/bench_user_kernel.json holds the run DESIGN.md section 5.9 quotes)"""
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
    rng = np.random.default_rng(20260102)
    n, beta = 10000, np.array([3.0, 2.0, -1.0, 0.5])
    X = rng.standard_normal((n, 3))
    y = beta[0] + X @ beta[1:] + 4.0 * rng.standard_normal(n)
    trivial = F.batched_fun(lambda th: -(th * th).sum(1), 3)
    linreg = F.gaussian_linreg(X, y)

    def user_normal(scale):
        return F.kernel_new(lambda env: env.theta0 + scale * env.rnorm(env.k))
    init3 = 0.01 * rng.standard_normal((a.chains, 3))
    init5 = np.array([0.0, 0.0, 0.0, 0.0, float(np.std(y, ddof=1))])[None, :] + 0.1 * rng.standard_normal((a.chains, 5))
    init5[:, -1] = np.abs(init5[:, -1])
    cases = {"fun_builtin": (trivial, init3, lambda: F.kernel_normal(scale=0.1)),
             "fun_user": (trivial, init3, lambda: user_normal(0.1)),
             "linreg_user": (linreg, init5, lambda: user_normal(0.02))}
    lines = []
    for name, (fun, init, kern) in cases.items():
        run = lambda ns: F.MCMC(init, fun, ns, nchains=a.chains, seed=7, kernel=kern(), _return_device=True,
                                keep_logpost=False, keep_draws=False)
        run(50)   # (warm-up: code objects, the caching allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(a.nsteps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines.append({"case": name, "k": init.shape[1], "chains": a.chains, "nsteps": a.nsteps, "kernel": abi.last_kernel(),
                      "us_per_step": round(dt / a.nsteps * 1e6, 2)})
        print(json.dumps(lines[-1]), flush=True)
    gm = linreg.device_model(dev)
    th = torch.as_tensor(init5).to(dev)
    out = torch.empty(a.chains, dtype=torch.float64, device=dev)
    for reps in (50, 1000):   # (the first round warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            gm.logpost(th, out=out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    lines.append({"case": "logpost_call", "k": 5, "chains": a.chains, "calls": reps, "kernel": "logpost_eval_kernel",
                  "us_per_call": round(dt / reps * 1e6, 2)})
    print(json.dumps(lines[-1]), flush=True)
    if a.json:
        props = torch.cuda.get_device_properties(dev)
        with open(a.json, "w") as f:
            json.dump({"tool": "tools/bench_user_kernel.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                       "device": props.name, "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
                       "timing": "wall clock of one call of nsteps steps after a 50-step warm-up call, synchronised; "
                                 "logpost_call: 1000 back-to-back calls after 50, synchronised once",
                       "cases": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
