"""What rhat(ans) of an McmcBatch costs against the loop it replaces, [rhat(ans[d]) for d in range(D)], at the shape of a
simulation study: D datasets x C chains x `rows` kept rows of k parameters (256 x 4 x 2000, k = 4).  The results are seeded series
in an McmcBatch built by hand (the diagnostic does not care where the rows came from).  Every measurement runs in a fresh child
process, after one warm-up call, as wall clock from the call to a synchronise behind the returned host object; `repeats` runs, all
of them reported.

  batch    the grouped rhat(ans), the grouped call alone (enqueue_rank_rhat_groups and the copy back; also between two device
           events) and the loop, in the same process.  The loop runs code this change does not touch: it is the parent commit's
           path.  The process also checks that both give the same bits.
  ragged   rhat(ans) on a result with four distinct row counts (rows, 3/4, 1/2 and 1/4 of them): four masked calls.
  kernels  the grouped call's kernel alone, from `rocprofv3 --kernel-trace --stats` in a run of its own (the program directly
           behind `--`); skipped with a note when rocprofv3 is not on the PATH.

Usage: python tools/bench_batch_rhat.py [--datasets D] [--chains C] [--rows R] [--k K] [--repeats N] [--loop-repeats N]
       [--json FILE] [--no-trace]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_batch_summary import result, timed  # noqa: E402  (the hand-built McmcBatch and the clock of that tool)


def same_bits(batch, loop):
    u = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return all(np.array_equal(u(getattr(batch[d], f)), u(getattr(loop[d], f))) for d in range(len(loop))
               for f in ("bulk", "tail", "rhat", "median")) and all(str(batch[d]) == str(loop[d]) for d in range(len(loop)))


def grouped_call(ans):
    from fmcmc_amd.summary import enqueue_rank_rhat_groups
    out, _scores, _work, _cols = enqueue_rank_rhat_groups(ans.history, ans.nmodels, ans.nchains, 0, int(ans.nrows[0]), None)
    return out


def device_ms(ans, repeats):
    """the one kernel a grouped call enqueues between two device events, ms"""
    import torch
    got = []
    for _ in range(repeats + 1):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        grouped_call(ans)
        ev1.record()
        torch.cuda.synchronize()
        got.append(round(ev0.elapsed_time(ev1), 3))
    return got[1:]


def part_batch(a):
    import fmcmc_amd as F
    ans = result(a.datasets, a.chains, a.k, a.rows)
    out = dict(part="batch", datasets=a.datasets, chains_per_dataset=a.chains, columns=a.k, rows=a.rows,
               values_per_group=2 * a.chains * (a.rows // 2))
    out["grouped_rhat_ms"], batch = timed(lambda: F.rhat(ans), a.repeats)
    out["grouped_call_ms"], _ = timed(lambda: grouped_call(ans).cpu(), a.repeats)
    out["grouped_device_ms"] = device_ms(ans, a.repeats)
    out["loop_ms"], loop = timed(lambda: [F.rhat(ans[d]) for d in range(len(ans))], a.loop_repeats)
    out["same_bits_and_text_as_the_loop"] = same_bits(batch, loop)
    assert out["same_bits_and_text_as_the_loop"], "the grouped call and the loop disagree"
    out["loop_over_grouped"] = round(min(out["loop_ms"]) / min(out["grouped_rhat_ms"]), 1)
    return out


def part_ragged(a):
    import fmcmc_amd as F
    counts = [a.rows, 3 * a.rows // 4, a.rows // 2, a.rows // 4]
    ans = result(a.datasets, a.chains, a.k, a.rows, [counts[d % 4] for d in range(a.datasets)])
    out = dict(part="ragged", datasets=a.datasets, chains_per_dataset=a.chains, columns=a.k, row_counts=counts)
    out["grouped_rhat_ms"], batch = timed(lambda: F.rhat(ans), a.repeats)
    out["loop_ms"], loop = timed(lambda: [F.rhat(ans[d]) for d in range(len(ans))], 1)
    out["same_bits_and_text_as_the_loop"] = same_bits(batch, loop)
    assert out["same_bits_and_text_as_the_loop"], "the grouped calls and the loop disagree"
    return out


def part_kernels(a):
    """what the traced run executes: the grouped call, a warm-up and `repeats` more"""
    import torch
    ans = result(a.datasets, a.chains, a.k, a.rows)
    for _ in range(a.repeats + 1):
        grouped_call(ans)
    torch.cuda.synchronize()
    return dict(part="kernels", calls=a.repeats + 1)


PARTS = {"batch": part_batch, "ragged": part_ragged, "kernels": part_kernels}


def child_cmd(a, part):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", part]
    for name in ("datasets", "chains", "rows", "k", "repeats", "loop_repeats"):
        cmd += ["--" + name.replace("_", "-"), str(getattr(a, name))]
    return cmd


def traced_kernels(a):
    """the rows of rocprofv3's kernel statistics of one `kernels` run: the grouped kernel and whatever else ran"""
    if shutil.which("rocprofv3") is None:
        return "not measured: rocprofv3 is not on the PATH"
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + child_cmd(a, "kernels")
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=200)
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if res.returncode != 0 or len(files) != 1:
            return "not measured: rocprofv3 ended with %d and left %d statistics files" % (res.returncode, len(files))
        rows = list(csv.DictReader(open(files[0])))
    keep = ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage")
    rows = [{k: r[k] for k in keep if k in r} for r in rows]
    ours = [r for r in rows if "rank_groups_kernel" in r["Name"]]
    return {"rank_groups_kernel": ours[0] if ours else None, "kernels_in_the_run": len(rows),
            "every_kernel": [(r["Name"][:60], r["Calls"], r["AverageNs"]) for r in rows[:6]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", type=int, default=256)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-repeats", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(PARTS[a.child](a)), flush=True)
        return
    lines = []
    for part in ("batch", "ragged"):
        res = subprocess.run(child_cmd(a, part), stdout=subprocess.PIPE, text=True, timeout=300)
        if res.returncode != 0:
            raise SystemExit("the %s measurement ended with %d" % (part, res.returncode))
        lines.append(json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(json.dumps(lines[-1]), flush=True)
    batch, ragged = lines
    rng = lambda v: [min(v), max(v)]
    summary = {"batch_ms": {"grouped_rhat": rng(batch["grouped_rhat_ms"]), "grouped_call": rng(batch["grouped_call_ms"]),
                            "grouped_device_events": rng(batch["grouped_device_ms"]), "loop": rng(batch["loop_ms"])},
               "loop_over_grouped_best": batch["loop_over_grouped"],
               "grouped_beats_the_loop_in_every_run": max(batch["grouped_rhat_ms"]) < min(batch["loop_ms"]),
               "ragged_ms": {"grouped_four_calls": rng(ragged["grouped_rhat_ms"]), "loop": rng(ragged["loop_ms"])},
               "kernel_trace": "not measured: --no-trace" if a.no_trace else traced_kernels(a)}
    print(json.dumps(summary), flush=True)
    if a.json:
        import torch
        props = torch.cuda.get_device_properties(0)
        doc = {"tool": "tools/bench_batch_rhat.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": props.name,
               "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
               "timing": "wall clock from the call to a synchronise behind the returned host object, after one warm-up call; "
                         "grouped_device_events: device events around the kernel one grouped call enqueues; kernel_trace: "
                         "rocprofv3 --kernel-trace --stats of a run of its own",
               "summary": summary, "cases": lines}
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
