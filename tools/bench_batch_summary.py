"""What summary(ans) of an McmcBatch costs against the loop it replaces, [summary(ans[d]) for d in range(D)], at the shape
tools/bench_batch.py publishes: D datasets x C chains x `rows` kept rows of k parameters, five quantiles.  The results are seeded
series in an McmcBatch built by hand (the summary does not care where the rows came from).  Every measurement runs in a fresh child
process, after one warm-up call, as wall clock from the call to a synchronise behind the returned host object; `repeats` runs,
the best and all of them reported; the grouped call's kernels are also timed between two device events.

  batch   the loop and the grouped call at D x C x rows.  The loop runs code this change does not touch; with --parent-lib it is
          timed on that build as well, the processes alternating parent, head, parent, head.  The head's process also checks
          that both give the same bits.
  ragged  the grouped call on a result with four distinct row counts (rows, 3/4, 1/2 and 1/4 of them): four masked calls.
  large   one large-group shape (16 datasets x 64 chains x 5000 rows): one select workgroup per (dataset, column) walks 320000
          values eight times or more; the loop's select spreads each column over many workgroups.

Usage: python tools/bench_batch_summary.py [--datasets D] [--chains C] [--rows R] [--k K] [--parent-lib FILE] [--json FILE]
(profiles/bench_batch_summary.json holds the run DESIGN.md section 5.11 quotes).  Without --parent-lib the parent's figures are
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

QUANTILES = (0.025, 0.25, 0.5, 0.75, 0.975)


def bind_parent(path):
    """The library of the parent commit behind _abi.lib(): it lacks the entries this package binds, so the few functions the
    loop calls are bound here."""
    from fmcmc_amd import _abi as abi
    L = C.CDLL(path)
    L.fmcmc_last_error.restype = C.c_char_p
    L.fmcmc_summary_work_len.restype = L.fmcmc_summary_pooled_len.restype = C.c_int64
    L.fmcmc_summary_work_len.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.fmcmc_summary_pooled_len.argtypes = [C.c_int32, C.c_int32]
    L.fmcmc_summary_dev.restype = C.c_int
    L.fmcmc_summary_dev.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                    C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    abi._lib = L
    return L


def result(D, Cm, k, rows, nrows=None):
    """an McmcBatch over seeded series: an MA(1) series per (chain, column) around a level of its dataset and column"""
    import torch
    import fmcmc_amd as F
    g = torch.Generator(device="cpu").manual_seed(3)
    e = torch.randn((D * Cm, k, rows + 1), generator=g, dtype=torch.float64)
    x = e[:, :, 1:] + 0.6 * e[:, :, :-1]
    x += torch.arange(D, dtype=torch.float64).repeat_interleave(Cm)[:, None, None] + 10.0 * torch.arange(k, dtype=torch.float64)[None, :, None]
    kw = {}
    if nrows is not None:
        for d, nr in enumerate(nrows):
            x[d * Cm:(d + 1) * Cm, :, nr:] = float("nan")
        kw = dict(nrows=np.asarray(nrows), steps=np.asarray(nrows), converged=[True] * D)
    dc = F.DeviceChains(x.contiguous().cuda(), None, None, np.arange(1, rows + 1), 1, None, 0, D * Cm)
    return F.McmcBatch(dc, D, Cm, **kw)


def timed(f, repeats):
    """f() once to warm up, then `repeats` runs: (wall ms of each, the last value)"""
    import torch
    f()
    ms, val = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        val = f()
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return ms, val


def kernels_ms(ans, repeats):
    """the enqueued kernels of one grouped call between two device events, ms"""
    import torch
    from fmcmc_amd.summary import enqueue_summary_groups
    out = []
    for _ in range(repeats + 1):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        enqueue_summary_groups(ans.history, ans.nmodels, ans.nchains, 0, int(ans.nrows[0]), None, QUANTILES)
        ev1.record()
        torch.cuda.synchronize()
        out.append(round(ev0.elapsed_time(ev1), 3))
    return out[1:]


def same_bits(batch, loop):
    u = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return all(np.array_equal(u(getattr(batch[d], f)), u(getattr(loop[d], f))) for d in range(len(loop))
               for f in ("statistics", "quantiles", "ess")) and all(str(batch[d]) == str(loop[d]) for d in range(len(loop)))


def part_batch(a, parent):
    import fmcmc_amd as F
    ans = result(a.datasets, a.chains, a.k, a.rows)
    out = dict(part="batch", build="parent" if parent else "head", datasets=a.datasets, chains_per_dataset=a.chains, columns=a.k,
               rows=a.rows, quantiles=len(QUANTILES))
    out["loop_ms"], loop = timed(lambda: [F.summary(ans[d], QUANTILES) for d in range(len(ans))], a.repeats)
    out["loop_ms_best"] = min(out["loop_ms"])
    if not parent:
        out["grouped_ms"], batch = timed(lambda: F.summary(ans, QUANTILES), a.repeats)
        out["grouped_ms_best"] = min(out["grouped_ms"])
        out["grouped_kernels_ms"] = kernels_ms(ans, a.repeats)
        out["same_bits_and_text_as_the_loop"] = same_bits(batch, loop)
        assert out["same_bits_and_text_as_the_loop"], "the grouped call and the loop disagree"
        out["loop_over_grouped"] = round(out["loop_ms_best"] / out["grouped_ms_best"], 1)
    return out


def part_ragged(a, parent):
    import fmcmc_amd as F
    counts = [a.rows, 3 * a.rows // 4, a.rows // 2, a.rows // 4]
    nrows = [counts[d % 4] for d in range(a.datasets)]
    ans = result(a.datasets, a.chains, a.k, a.rows, nrows)
    out = dict(part="ragged", build="head", datasets=a.datasets, chains_per_dataset=a.chains, columns=a.k, row_counts=counts)
    out["grouped_ms"], batch = timed(lambda: F.summary(ans, QUANTILES), a.repeats)
    out["grouped_ms_best"] = min(out["grouped_ms"])
    out["loop_ms"], loop = timed(lambda: [F.summary(ans[d], QUANTILES) for d in range(len(ans))], a.repeats)
    out["loop_ms_best"] = min(out["loop_ms"])
    out["same_bits_and_text_as_the_loop"] = same_bits(batch, loop)
    assert out["same_bits_and_text_as_the_loop"], "the grouped calls and the loop disagree"
    return out


def part_large(a, parent):
    import fmcmc_amd as F
    D, Cm, rows = 16, 64, 5000
    ans = result(D, Cm, a.k, rows)
    out = dict(part="large", build="head", datasets=D, chains_per_dataset=Cm, columns=a.k, rows=rows, values_per_group=Cm * rows)
    out["grouped_ms"], batch = timed(lambda: F.summary(ans, QUANTILES), a.repeats)
    out["grouped_ms_best"] = min(out["grouped_ms"])
    out["grouped_kernels_ms"] = kernels_ms(ans, a.repeats)
    out["loop_ms"], loop = timed(lambda: [F.summary(ans[d], QUANTILES) for d in range(D)], a.repeats)
    out["loop_ms_best"] = min(out["loop_ms"])
    out["same_bits_and_text_as_the_loop"] = same_bits(batch, loop)
    assert out["same_bits_and_text_as_the_loop"], "the grouped call and the loop disagree"
    out["grouped_over_loop"] = round(out["grouped_ms_best"] / out["loop_ms_best"], 2)
    return out


PARTS = {"batch": part_batch, "ragged": part_ragged, "large": part_large}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", type=int, default=256)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
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
        for name in ("datasets", "chains", "rows", "k", "repeats"):
            cmd += ["--" + name, str(getattr(a, name))]
        if a.parent_lib:
            cmd += ["--parent-lib", a.parent_lib]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
        if res.returncode != 0:
            raise SystemExit("the %s measurement on the %s build ended with %d" % (part, build, res.returncode))
        line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        lines.append(line)
        print(json.dumps(line), flush=True)
        return line

    runs = [child("batch", b) for b in (["parent", "head", "parent", "head"] if a.parent_lib else ["head", "head"])]
    ragged, large = child("ragged", "head"), child("large", "head")
    grouped = [v for r in runs if r["build"] == "head" for v in r["grouped_ms"]]
    kernels = [v for r in runs if r["build"] == "head" for v in r["grouped_kernels_ms"]]
    loop_head = [v for r in runs if r["build"] == "head" for v in r["loop_ms"]]
    loop_parent = [v for r in runs if r["build"] == "parent" for v in r["loop_ms"]]
    rng = lambda v: [min(v), max(v)]
    summary = {"batch_ms": {"grouped": rng(grouped), "grouped_kernels": rng(kernels), "loop_head": rng(loop_head),
                            "loop_parent": rng(loop_parent) if loop_parent else "not measured"},
               "grouped_beats_the_parents_loop_in_every_run": (max(grouped) < min(loop_parent)) if loop_parent else "not measured",
               "loop_over_grouped_best": round(min(loop_parent or loop_head) / min(grouped), 1),
               "ragged_ms": {"grouped_four_calls": rng(ragged["grouped_ms"]), "loop": rng(ragged["loop_ms"])},
               "large_group_ms": {"grouped": rng(large["grouped_ms"]), "grouped_kernels": rng(large["grouped_kernels_ms"]),
                                  "loop": rng(large["loop_ms"]), "grouped_over_loop": large["grouped_over_loop"]}}
    print(json.dumps(summary), flush=True)
    if a.json:
        import torch
        props = torch.cuda.get_device_properties(0)
        doc = {"tool": "tools/bench_batch_summary.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": props.name,
               "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
               "timing": "wall clock from the call to a synchronise behind the returned host object, after one warm-up call, "
                         "`repeats` runs per process, processes in the order of `cases`; *_kernels_ms: device events around the "
                         "kernels one grouped call enqueues",
               "summary": summary, "cases": lines}
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
