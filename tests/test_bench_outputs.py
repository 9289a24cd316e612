"""bench.py --dump-outputs and the plain (lean) run.

CPU: dump_outputs writes every array as float64 .npy, whole where the outputs fit the size limit, otherwise a fixed, seeded
     sample of chains (and of kept rows where even the fewest chains are too long), recorded in chain_index / row_index.
GPU: a plain run of the headline config times exactly --steps steps, carries none of what --full measures, and writes the
     outputs of its last timed step; a second run with the same arguments writes the same bits."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _outputs(torch, C, k, S, draws=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(C, k, S, dtype=torch.float64, generator=g)
    outs = {"samples": s, "logpost": torch.randn(C, S, dtype=torch.float64, generator=g),
            "accept_count": torch.randint(0, S, (C,), generator=g)}
    if draws:
        outs["draws"] = torch.randn(C, k, S, dtype=torch.float64, generator=g)
    outs["final_state"] = s[:, :, -1]
    return outs


def _size(d):
    return sum(os.path.getsize(f) for f in glob.glob(os.path.join(d, "*.npy")))


def test_dump_outputs_writes_small_outputs_whole(tmp_path):
    import torch
    import bench
    outs = _outputs(torch, 7, 3, 20)
    r = bench.dump_outputs(str(tmp_path), outs, 0, 1, torch)
    assert r["chains"] == "7 of 7" and r["rows"] == "all"
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in outs)
    for n, a in outs.items():
        got = np.load(str(tmp_path / (n + ".npy")))
        assert got.dtype == np.float64
        assert np.array_equal(got, a.double().numpy())


@pytest.mark.parametrize("C,k,S,draws", [(1024, 5, 10000, True),     # C2's outputs: a sample of the chains
                                         (512, 50, 10000, False)])   # C4's: a sample of the chains and of their rows
def test_dump_outputs_samples_large_outputs_within_the_limit(tmp_path, C, k, S, draws):
    import torch
    import bench
    outs = _outputs(torch, C, k, S, draws)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), outs, 0, 1, torch)
    bench.dump_outputs(str(b), outs, 0, 1, torch)
    assert _size(str(a)) <= 64 * 10 ** 6
    ci = np.load(str(a / "chain_index.npy")).astype(np.int64)
    assert 0 < ci.size < C and np.all(np.diff(ci) > 0)
    src = outs["samples"].numpy()[ci]
    if os.path.exists(str(a / "row_index.npy")):
        ri = np.load(str(a / "row_index.npy")).astype(np.int64)
        assert 0 < ri.size < S and np.all(np.diff(ri) > 0)
        src = src[:, :, ri]
    assert np.array_equal(np.load(str(a / "samples.npy")), src)
    assert np.array_equal(np.load(str(a / "final_state.npy")), outs["samples"].numpy()[ci, :, -1])
    for f in sorted(os.listdir(str(a))):                              # the sample is fixed: the same files every time
        assert np.array_equal(np.load(str(a / f)), np.load(str(b / f)))


def test_dump_outputs_divides_the_limit_over_the_ranks(tmp_path):
    import torch
    import bench
    outs = _outputs(torch, 1024, 5, 10000)
    bench.dump_outputs(str(tmp_path), outs, 0, 2, torch)
    bench.dump_outputs(str(tmp_path), _outputs(torch, 1024, 5, 10000, seed=1), 1, 2, torch)
    assert os.path.exists(str(tmp_path / "samples.npy")) and os.path.exists(str(tmp_path / "samples_rank1.npy"))
    assert _size(str(tmp_path)) <= 64 * 10 ** 6


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out_dir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_its_dumped_outputs_repeat(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _plain_run(a)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] > 0 and line["unit"] == "MH samples/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    for key in ("cpu_baseline", "configs", "strong_scaling_projection", "scalings"):
        assert key not in line
    assert "default_path_ms_per_step" not in line["roofline"]
    names = sorted(os.listdir(a))
    assert {"samples.npy", "logpost.npy", "draws.npy", "accept_count.npy", "final_state.npy"} <= set(names)
    assert _size(a) <= 64 * 10 ** 6
    s = np.load(os.path.join(a, "samples.npy"))
    assert s.dtype == np.float64 and s.shape[1:] == (5, 10000) and np.isfinite(s).all()
    _plain_run(b)
    assert sorted(os.listdir(b)) == names
    for f in names:
        assert np.array_equal(np.load(os.path.join(a, f)).view(np.uint64), np.load(os.path.join(b, f)).view(np.uint64)), f
