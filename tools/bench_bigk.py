"""Step time of mh_sweep_bigk (more parameters than a wavefront has lanes) in its two forms: matrices in LDS ("big-k") and in
the chain's Sigma square in HBM ("big-k-hbm").  Gaussian linreg, n = 1000, k = 100 (LDS form, and the HBM form forced with
FMCMC_AMD_DEBUG=bigkhbm=1), 150, 200, 256; kernel_ram, kernel_adapt (warm-up 5, so that every timed step adapts) and
kernel_normal; 1, 256 and 1024 chains.  One warm-up call per shape, then the best of `reps` timed calls of `nsteps` steps
(host clock around a call that ends in a device synchronise).  Prints one line per shape; --json FILE writes the rows."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fmcmc_amd import engine as E, _abi as abi

ap = argparse.ArgumentParser()
ap.add_argument("--nsteps", type=int, default=20)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--chains", default="1,256,1024")
ap.add_argument("--json", default=None)
a = ap.parse_args()
n = 1000
KINDS = {"ram": abi.KERNEL_RAM, "adapt": abi.KERNEL_ADAPT, "normal": abi.KERNEL_NORMAL}
rows = []
for k, forced in ((100, False), (100, True), (150, False), (200, False), (256, False)):
    rng = np.random.default_rng(k)
    p = k - 2
    beta = np.linspace(1.0, -1.0, p + 1)
    X = rng.standard_normal((n, p)); y = beta[0] + X @ beta[1:] + 2.0 * rng.standard_normal(n)
    gm = E.DeviceModel(abi.FAM_GAUSSIAN_LINREG, X, y)
    for kname, kind in KINDS.items():
        gk = E.KernelSpec(kind, k, np.zeros(k), np.full(k, 0.01), np.full(k, -E.DBL_MAX), np.full(k, E.DBL_MAX), np.zeros(k, np.uint8),
                          warmup=5 if kind == abi.KERNEL_ADAPT else 0)
        for C in [int(c) for c in a.chains.split(",")]:
            if forced:
                os.environ["FMCMC_AMD_DEBUG"] = "bigkhbm=1"
            else:
                os.environ.pop("FMCMC_AMD_DEBUG", None)
            init = np.r_[beta, 2.0][None, :] + 0.02 * rng.standard_normal((C, k))
            st = E.ChainState(init, k)
            E.sweep(gm, gk, st, a.nsteps, want_draws=False, want_logpost=False, want_bits=False)   # warm-up (and past warm-up)
            torch.cuda.synchronize()
            form = abi.last_kernel()
            best = float("inf")
            for _ in range(a.reps):
                t = time.time()
                E.sweep(gm, gk, st, a.nsteps, want_draws=False, want_logpost=False, want_bits=False)
                torch.cuda.synchronize()
                best = min(best, (time.time() - t) / (a.nsteps - 1))
            row = dict(k=k, kernel=kname, chains=C, form=form, us_per_step=best * 1e6)
            rows.append(row)
            print("k=%3d %-6s C=%4d %-9s %10.1f us per step" % (k, kname, C, form, best * 1e6), flush=True)
os.environ.pop("FMCMC_AMD_DEBUG", None)
if a.json:
    with open(a.json, "w") as f:
        json.dump(rows, f, indent=1)
