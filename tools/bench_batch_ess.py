"""What ess(ans) of an McmcBatch costs against the loop it replaces, [ess(ans[d]) for d in range(D)], at the shape of a simulation
study: D datasets x C chains x `rows` kept rows of k parameters (256 x 4 x 2000, k = 4).  The results are seeded series in an
McmcBatch built by hand (tools/bench_batch_summary.py: result; the diagnostic does not care where the rows came from).  Every
measurement runs in a fresh child process under a time limit of its own, after one warm-up call, as wall clock from the call to a
synchronise behind the returned host object; `repeats` runs, all of them reported.  A child that fails or runs out of time ends
the tool: nothing more is started.

  batch    the grouped ess(ans); its two halves, the grouped call with its copy back (enqueue_rank_ess_groups, `out` to the host)
           and the host finish (ess_groups_finish on that copy); the NaN prefill and the kernel between two device events; and
           the loop, in the same process.  The loop runs the single form, which this tool's subject does not replace: it is the
           path ess(ans) took before.  The process also checks that both give the same bits and the same text.
  ragged   ess(ans) on a result with four distinct row counts (rows, 3/4, 1/2 and 1/4 of them): four masked calls.

Usage: python tools/bench_batch_ess.py [--datasets D] [--chains C] [--rows R] [--k K] [--repeats N] [--loop-repeats N]
       [--json FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_batch_summary import result, timed  # noqa: E402  (the hand-built McmcBatch and the clock of that tool)

FIELDS = ("bulk", "tail", "tail_q05", "tail_q95", "mean", "mcse_mean", "tau_bulk", "q05", "q95")
CHILD_SECONDS = {"batch": 240, "ragged": 240}


def same_bits(batch, loop):
    u = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return all(np.array_equal(u(getattr(batch[d], f)), u(getattr(loop[d], f))) for d in range(len(loop)) for f in FIELDS) \
        and all(np.array_equal(batch[d].lags, loop[d].lags) and str(batch[d]) == str(loop[d]) for d in range(len(loop)))


def grouped_call(ans):
    from fmcmc_amd.summary import enqueue_rank_ess_groups
    out, _work, _cols = enqueue_rank_ess_groups(ans.history, ans.nmodels, ans.nchains, 0, int(ans.nrows[0]), None)
    return out


def device_ms(ans, repeats):
    """the NaN prefill of `out` and the one kernel a grouped call enqueues, between two device events, ms"""
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


def host_ms(f, repeats):
    """a host-only step: wall ms of `repeats` runs after one warm-up"""
    f()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return ms


def part_batch(a):
    import fmcmc_amd as F
    from fmcmc_amd.summary import ess_groups_finish
    ans = result(a.datasets, a.chains, a.k, a.rows)
    out = dict(part="batch", datasets=a.datasets, chains_per_dataset=a.chains, columns=a.k, rows=a.rows,
               values_per_group=2 * a.chains * (a.rows // 2))
    out["grouped_ess_ms"], batch = timed(lambda: F.ess(ans), a.repeats)
    out["grouped_call_and_copy_ms"], host = timed(lambda: grouped_call(ans).cpu().numpy(), a.repeats)
    out["out_megabytes"] = round(host.nbytes / 1e6, 1)
    out["host_finish_ms"] = host_ms(lambda: ess_groups_finish(host, a.chains, a.rows), a.repeats)
    out["grouped_device_ms"] = device_ms(ans, a.repeats)
    out["lags_computed_max"] = int(ess_groups_finish(host, a.chains, a.rows).computed.max())
    out["loop_ms"], loop = timed(lambda: [F.ess(ans[d]) for d in range(len(ans))], a.loop_repeats)
    out["same_bits_and_text_as_the_loop"] = same_bits(batch, loop)
    assert out["same_bits_and_text_as_the_loop"], "the grouped call and the loop disagree"
    out["loop_over_grouped"] = round(min(out["loop_ms"]) / min(out["grouped_ess_ms"]), 1)
    return out


def part_ragged(a):
    import fmcmc_amd as F
    counts = [a.rows, 3 * a.rows // 4, a.rows // 2, a.rows // 4]
    ans = result(a.datasets, a.chains, a.k, a.rows, [counts[d % 4] for d in range(a.datasets)])
    out = dict(part="ragged", datasets=a.datasets, chains_per_dataset=a.chains, columns=a.k, row_counts=counts)
    out["grouped_ess_ms"], batch = timed(lambda: F.ess(ans), a.repeats)
    out["loop_ms"], loop = timed(lambda: [F.ess(ans[d]) for d in range(len(ans))], 1)
    out["same_bits_and_text_as_the_loop"] = same_bits(batch, loop)
    assert out["same_bits_and_text_as_the_loop"], "the grouped calls and the loop disagree"
    return out


PARTS = {"batch": part_batch, "ragged": part_ragged}


def child_cmd(a, part):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", part]
    for name in ("datasets", "chains", "rows", "k", "repeats", "loop_repeats"):
        cmd += ["--" + name.replace("_", "-"), str(getattr(a, name))]
    return cmd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", type=int, default=256)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-repeats", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(PARTS[a.child](a)), flush=True)
        return
    lines = []
    for part in ("batch", "ragged"):                 # one after the other; the first that fails ends the tool
        try:
            res = subprocess.run(child_cmd(a, part), stdout=subprocess.PIPE, text=True, timeout=CHILD_SECONDS[part])
        except subprocess.TimeoutExpired:
            raise SystemExit("the %s measurement did not end within %d s" % (part, CHILD_SECONDS[part]))
        if res.returncode != 0:
            raise SystemExit("the %s measurement ended with %d" % (part, res.returncode))
        lines.append(json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(json.dumps(lines[-1]), flush=True)
    batch, ragged = lines
    rng = lambda v: [min(v), max(v)]
    summary = {"batch_ms": {"grouped_ess": rng(batch["grouped_ess_ms"]),
                            "grouped_call_and_copy_back": rng(batch["grouped_call_and_copy_ms"]),
                            "host_finish": rng(batch["host_finish_ms"]),
                            "prefill_and_kernel_device_events": rng(batch["grouped_device_ms"]), "loop": rng(batch["loop_ms"])},
               "out_megabytes": batch["out_megabytes"],
               "loop_over_grouped_best": batch["loop_over_grouped"],
               "grouped_beats_the_loop_in_every_run": max(batch["grouped_ess_ms"]) < min(batch["loop_ms"]),
               "ragged_ms": {"grouped_four_calls": rng(ragged["grouped_ess_ms"]), "loop": rng(ragged["loop_ms"])}}
    print(json.dumps(summary), flush=True)
    if a.json:
        import torch
        props = torch.cuda.get_device_properties(0)
        doc = {"tool": "tools/bench_batch_ess.py", "date_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "device": props.name,
               "arch": getattr(props, "gcnArchName", ""), "torch": torch.__version__,
               "timing": "wall clock from the call to a synchronise behind the returned host object, after one warm-up call; "
                         "host_finish: wall clock of ess_groups_finish on the copied `out`; prefill_and_kernel_device_events: "
                         "device events around the NaN prefill and the kernel one grouped call enqueues",
               "summary": summary, "cases": lines}
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
