"""What MCMC_batch(stop_each = ...) costs and saves, at the shape tools/bench_batch.py publishes: D datasets x C chains of the
README's regression (linreg, n observations, p covariates).  Three measurements, each in fresh child processes:

  (a) check   one grouped Gelman-Rubin check of a 2000-row window of all D datasets (summary.enqueue_gelman_groups, one copy
              back, D host finishes) against the loop it replaces: D convergence_gelman.check_device calls, one per dataset.
              The loop runs code this change does not touch; with --parent-lib it is timed on that build as well.
  (b) sweep   us per MH step of "batch-lds" through fmcmc_mcmc_run_batch_sel_dev with active = NULL and with an all-ones mask,
              against fmcmc_mcmc_run_batch_dev of --parent-lib (the build of the parent commit): processes alternate parent,
              head, parent, head; every figure is one call of --nsteps steps between device events, after a warm-up call.
  (c) stop    one MCMC_batch(stop_each = convergence_gelman(freq, threshold)) call under kernel_ram: us per step of every
              bulk beside the number of datasets still running, and the whole call against the same call without a stop.

Usage: python tools/bench_batch_stop.py [--datasets D] [--chains C] [--n N] [--p P] [--nsteps S] [--parent-lib FILE] [--json FILE]
(profiles/bench_batch_stop.json holds the run DESIGN.md section 5.11 quotes).  Without --parent-lib the parent's figures are
"not measured"."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bind_parent(path):
    """The library of the parent commit behind _abi.lib(): it lacks the entries this package binds, so the few functions the
    parent's measurements call are bound here."""
    from fmcmc_amd import _abi as abi
    L = C.CDLL(path)
    L.fmcmc_last_error.restype = L.fmcmc_last_kernel.restype = C.c_char_p
    L.fmcmc_gelman_partial_len.restype = L.fmcmc_gelman_work_len.restype = C.c_int64
    L.fmcmc_gelman_partial_len.argtypes = [C.c_int32]
    L.fmcmc_gelman_work_len.argtypes = [C.c_int64, C.c_int32]
    L.fmcmc_gelman_partial_dev.restype = C.c_int
    L.fmcmc_gelman_partial_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    dp = C.POINTER(C.c_double)
    L.fmcmc_gelman_finish.restype = C.c_int
    L.fmcmc_gelman_finish.argtypes = [dp, C.c_int32, C.c_int64, dp, dp]
    L.fmcmc_mcmc_run_batch_dev.restype = C.c_int
    L.fmcmc_mcmc_run_batch_dev.argtypes = [C.POINTER(abi.Model), C.c_int64, C.c_int64, C.c_int64, C.POINTER(abi.Kernel),
                                           C.POINTER(abi.Run), C.POINTER(abi.State), C.POINTER(abi.Out), C.c_uint32, C.c_void_p]
    abi._lib = L
    return L


def data(a):
    D, Cm, n, p, k = a.datasets, a.chains, a.n, a.p, a.p + 2
    rng = np.random.default_rng(1)
    beta = np.linspace(1.0, -1.0, p + 1)
    Xs = rng.standard_normal((D, n, p))
    ys = beta[0] + Xs @ beta[1:] + 2.0 * rng.standard_normal((D, n))
    base = np.array(list(beta) + [2.0])
    return Xs, ys, base, k


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def part_check(a, parent):
    """(a): a seeded random history [D C][k][4000]; the window is coda's second half, 2000 rows"""
    import torch
    import fmcmc_amd as F
    from fmcmc_amd.convergence import _window
    from fmcmc_amd.summary import enqueue_gelman_groups
    D, Cm, k, rows = a.datasets, a.chains, a.p + 2, 4000
    g = torch.Generator(device="cpu").manual_seed(3)
    x = (torch.randn((D * Cm, k, rows), generator=g, dtype=torch.float64) + 0.1 * torch.randn((D * Cm, k, 1), generator=g, dtype=torch.float64)).cuda()
    iters = np.arange(1, rows + 1)
    free = np.arange(k)
    row0, N = _window(iters)
    out = dict(part="check", build="parent" if parent else "head", datasets=D, chains_per_dataset=Cm, columns=k, window_rows=N)

    def loop():
        chk = F.convergence_gelman(1000, threshold=1.1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verdicts = []
        for d in range(D):
            dc = F.DeviceChains(x[d * Cm:(d + 1) * Cm], None, None, iters, 1, None, 0, Cm)
            verdicts.append(chk.check_device(dc, free))
        return (time.perf_counter() - t0) * 1e3, verdicts, [h[1] for h in chk.history]

    loop()
    runs = [loop() for _ in range(a.repeats)]
    out["loop_ms"] = [round(r[0], 3) for r in runs]
    out["loop_ms_median"] = round(median(out["loop_ms"]), 3)
    if not parent:
        full = F.DeviceChains(x, None, None, iters, 1, None, 0, D * Cm)

        def grouped():
            chk = F.convergence_gelman(1000, threshold=1.1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            partials, _work, _cols = enqueue_gelman_groups(full, D, Cm, row0, N, free)
            ph = partials.cpu().numpy()
            verdicts = [chk._finish(ph[d], k, N, rows, ph.shape[1] - 2, Cm) for d in range(D)]
            return (time.perf_counter() - t0) * 1e3, verdicts, [h[1] for h in chk.history]

        grouped()
        gr = [grouped() for _ in range(a.repeats)]
        assert gr[0][1] == runs[0][1] and gr[0][2] == runs[0][2], "the grouped check and the loop disagree"
        out["grouped_ms"] = [round(r[0], 3) for r in gr]
        out["grouped_ms_median"] = round(median(out["grouped_ms"]), 3)
        out["loop_over_grouped"] = round(out["loop_ms_median"] / out["grouped_ms_median"], 1)
        out["same_verdicts_and_statistics_to_the_bit"] = True
    return out


def part_sweep(a, parent):
    """(b): kernel_normal, the dataset in LDS, nothing but the samples written"""
    import torch
    from fmcmc_amd import _abi as abi
    from fmcmc_amd import engine as E
    Xs, ys, base, k = data(a)
    D, Cm = a.datasets, a.chains
    init = base[None, :] + 0.05 * np.random.default_rng(2).standard_normal((D * Cm, k))
    init[:, -1] = np.abs(init[:, -1]) + 0.5
    unb, free = np.full(k, 1e308), np.zeros(k, np.uint8)
    gk = E.KernelSpec(abi.KERNEL_NORMAL, k, np.zeros(k), np.full(k, 0.05), -unb, unb, free)
    batch = E.DeviceModelBatch(abi.FAM_GAUSSIAN_LINREG, Xs, ys)
    L = abi.lib()
    ones = torch.ones(D, dtype=torch.int32, device="cuda")

    def one(ns, mask):
        st = E.ChainState(init, gk.kf)
        out, crun, cout = E._call_buffers(st, ns, 0, 1, 7, 0, False, False, False, None, None, None, 0)
        cm, ck, cs = batch.c(), gk.c(), st.c(ns)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        if parent:
            rc = L.fmcmc_mcmc_run_batch_dev(C.byref(cm), D, batch.x_stride, batch.y_stride, C.byref(ck), C.byref(crun), C.byref(cs),
                                            C.byref(cout), 0, stream)
        else:
            rc = L.fmcmc_mcmc_run_batch_sel_dev(C.byref(cm), D, batch.x_stride, batch.y_stride, C.byref(ck), C.byref(crun),
                                                C.byref(cs), C.byref(cout), mask.data_ptr() if mask is not None else None, 0, stream)
        ev1.record()
        torch.cuda.synchronize()
        assert rc == 0 and int(out.status.abs().sum()) == 0
        return ev0.elapsed_time(ev1) * 1e3 / ns, float(out.samples[:, :, -1].sum())

    out = dict(part="sweep", build="parent" if parent else "head", datasets=D, chains_per_dataset=Cm, n=a.n, p=a.p, nsteps=a.nsteps)
    one(50, None)
    variants = [("entry", None)] if parent else [("null", None), ("ones", ones)]
    for _ in range(a.repeats):
        for name, mask in variants:
            us, checksum = one(a.nsteps, mask)
            out.setdefault("us_per_step_" + name, []).append(round(us, 3))
            out["checksum"] = checksum
    out["form"] = L.fmcmc_last_kernel().decode()
    return out


def part_stop(a, parent):
    """(c): kernel_ram from scattered starts; engine.sweep_batch is wrapped to time every bulk to its synchronise"""
    import torch
    import fmcmc_amd as F
    from fmcmc_amd import engine as E
    Xs, ys, base, k = data(a)
    D, Cm = a.datasets, a.chains
    init = base[None, :] + 0.5 * np.random.default_rng(4).standard_normal((D * Cm, k))
    init[:, -1] = np.abs(init[:, -1]) + 0.5
    batch = F.model_batch(F.gaussian_linreg(Xs[d], ys[d]) for d in range(D))
    bulks, inner = [], E.sweep_batch

    def timed(b, kernel, state, nsteps, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = inner(b, kernel, state, nsteps, **kw)
        torch.cuda.synchronize()
        act = kw.get("active")
        bulks.append(dict(nsteps=nsteps, active_datasets=D if act is None else int(act.sum()),
                          us_per_step=round((time.perf_counter() - t0) / nsteps * 1e6, 2)))
        return r

    def call(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ans = F.MCMC_batch(init.reshape(D, Cm, k), batch, a.stop_nsteps, nchains=Cm, seed=11, kernel=F.kernel_ram(), **kw)
        torch.cuda.synchronize()
        return ans, (time.perf_counter() - t0) * 1e3

    call(stop_each=F.convergence_gelman(a.stop_freq, threshold=a.stop_threshold))      # warm-up of every shape
    E.sweep_batch = timed
    try:
        ans, ms = call(stop_each=F.convergence_gelman(a.stop_freq, threshold=a.stop_threshold))
    finally:
        E.sweep_batch = inner
    stop_bulks = list(bulks)
    call()
    _full, ms_full = call()
    steps, counts = np.unique(ans.steps, return_counts=True)
    return dict(part="stop", build="head", datasets=D, chains_per_dataset=Cm, n=a.n, p=a.p, kernel="kernel_ram", nsteps=a.stop_nsteps,
                freq=a.stop_freq, threshold=a.stop_threshold, bulks=stop_bulks, call_ms=round(ms, 2),
                call_ms_note="with a synchronise around every bulk", converged=int(ans.converged.sum()),
                datasets_by_steps_run={int(s): int(c) for s, c in zip(steps, counts)},
                steps_run_over_steps_without_stop=round(float(ans.steps.sum()) / (D * a.stop_nsteps), 3),
                call_without_stop_ms=round(ms_full, 2))


PARTS = {"check": part_check, "sweep": part_sweep, "stop": part_stop}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", type=int, default=256)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--nsteps", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stop-nsteps", type=int, default=4000)
    ap.add_argument("--stop-freq", type=int, default=500)
    ap.add_argument("--stop-threshold", type=float, default=1.1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)      # PART:head or PART:parent
    a = ap.parse_args()
    if a.child:
        part, build = a.child.split(":")
        if build == "parent":
            bind_parent(a.parent_lib)
        print("RESULT " + json.dumps(PARTS[part](a, build == "parent")), flush=True)
        return
    lines = []

    def child(part, build):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "%s:%s" % (part, build)]
        for name in ("datasets", "chains", "n", "p", "nsteps", "repeats", "stop_nsteps", "stop_freq", "stop_threshold"):
            cmd += ["--" + name.replace("_", "-"), str(getattr(a, name))]
        if a.parent_lib:
            cmd += ["--parent-lib", a.parent_lib]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
        if res.returncode != 0:
            raise SystemExit("the %s measurement on the %s build ended with %d" % (part, build, res.returncode))
        line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        lines.append(line)
        print(json.dumps(line), flush=True)
        return line

    builds = ["parent", "head", "parent", "head"] if a.parent_lib else ["head", "head"]
    sweeps = [child("sweep", b) for b in builds]
    checks = [child("check", b) for b in (["parent", "head"] if a.parent_lib else ["head"])]
    child("stop", "head")
    summary = {}
    head = [v for s in sweeps if s["build"] == "head" for v in s["us_per_step_null"]]
    ones = [v for s in sweeps if s["build"] == "head" for v in s["us_per_step_ones"]]
    par = [v for s in sweeps if s["build"] == "parent" for v in s["us_per_step_entry"]]
    summary["sweep_us_per_step"] = {"head_null": [min(head), max(head)], "head_all_ones": [min(ones), max(ones)],
                                    "parent": [min(par), max(par)] if par else "not measured"}
    summary["sweep_same_checksum"] = len({s["checksum"] for s in sweeps}) == 1
    hc = [c for c in checks if c["build"] == "head"][0]
    pc = [c for c in checks if c["build"] == "parent"]
    summary["check_ms"] = {"grouped": hc["grouped_ms_median"], "loop_head": hc["loop_ms_median"],
                           "loop_parent": pc[0]["loop_ms_median"] if pc else "not measured", "loop_over_grouped": hc["loop_over_grouped"]}
    print(json.dumps(summary), flush=True)
    if a.json:
        import torch
        props = torch.cuda.get_device_properties(0)
        doc = {"tool": "tools/bench_batch_stop.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": props.name,
               "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
               "timing": "sweep: device events around one call of nsteps steps after a 50-step warm-up, `repeats` calls per process, "
                         "processes in the order of `cases`; check: wall clock from the first enqueue to the last host finish, after "
                         "one warm-up round, `repeats` rounds; stop: wall clock to a synchronise behind every bulk",
               "summary": summary, "cases": lines}
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
