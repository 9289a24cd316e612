"""examples/c_abi_fun.c: a user-defined log-posterior through fmcmc_mcmc_run_fun_host from plain C (gcc, host pointers, a CPU
callback).  CPU: it compiles against include/fmcmc_amd.h, links the library and fails loudly without a GPU.  GPU: over two calls
with carried kernel state its output equals the oracle's bit for bit -- samples, logpost, draws, acceptance and the state
(theta0, f0, abs_iter, Sigma, mean_prev, have_mean, nerrors)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fmcmc_amd", "lib")


def _build(tmp_path):
    if not os.path.exists(os.path.join(LIBDIR, "libfmcmc_amd.so")):
        pytest.skip("libfmcmc_amd.so is not built (python -m fmcmc_amd.build)")
    exe = str(tmp_path / "c_abi_fun")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-mfma", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "c_abi_fun.c"), "-o", exe,
                    "-L" + LIBDIR, "-lfmcmc_amd", "-lm", "-Wl,-rpath," + LIBDIR], check=True)
    return exe


def _case(kind):
    from conftest import synth_linreg
    X, y = synth_linreg(700, 2, 654)
    rng = np.random.default_rng(6)
    init = np.array([3.0, 2.0, -1.0, float(np.std(y))])[None, :] + 0.1 * rng.standard_normal((5, 4))
    init[:, -1] = np.abs(init[:, -1])
    bounded = kind in (2, 4, 6)
    lb = np.array([-10.0, -10.0, -10.0, 0.5]) if bounded else np.full(4, -np.finfo(np.float64).max)
    ub = np.full(4, 20.0) if bounded else np.full(4, np.finfo(np.float64).max)
    return X, y, init, np.full(4, 0.05), lb, ub


def _write_input(path, X, y, init, scale, lb, ub, nsteps, burnin, thin, seed, kind, calls):
    n, p = X.shape
    C, k = init.shape
    with open(path, "wb") as f:
        f.write(np.array([n, p, C, k, nsteps, burnin, thin, seed, kind, calls], np.int64).tobytes())
        for a in (X.T, y, init, scale, lb, ub):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())


def _run(exe, fin, fout):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=300)


def test_c_fun_example_builds_and_fails_loudly_without_a_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: covered by the gpu test")
    exe = _build(tmp_path)
    X, y, init, scale, lb, ub = _case(1)
    _write_input(str(tmp_path / "in.bin"), X, y, init, scale, lb, ub, 100, 0, 1, 5, 1, 1)
    r = _run(exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"))
    assert r.returncode == 3 and "no CPU fallback" in r.stderr
    assert not os.path.exists(str(tmp_path / "out.bin"))


class _Reader:
    def __init__(self, raw):
        self.raw, self.off = raw, 0

    def take(self, dtype, shape):
        a = np.frombuffer(self.raw, dtype, int(np.prod(shape)), offset=self.off).reshape(shape)
        self.off += a.nbytes
        return a


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_c_fun_example_equals_the_oracle(tmp_path, kind):
    sys.path.insert(0, ROOT)
    from oracle import oracle as O
    exe = _build(tmp_path)
    X, y, init, scale, lb, ub = _case(kind)
    nsteps, burnin, thin, seed, calls = 150, 10, 2, 4321, 2
    _write_input(str(tmp_path / "in.bin"), X, y, init, scale, lb, ub, nsteps, burnin, thin, seed, kind, calls)
    r = _run(exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"))
    assert r.returncode == 0, r.stderr
    assert "kernel fun," in r.stdout
    om = O.Model(O.FAM_LINREG, X, y)
    ok = O.Kernel(kind, 4, scale=scale, lb=lb, ub=ub, warmup=20 if kind == O.K_ADAPT else 0)
    ost = O.ChainState(init, 4)
    C, k, S, W = 5, 4, (nsteps - burnin) // thin, (nsteps + 31) // 32
    rd = _Reader(open(str(tmp_path / "out.bin"), "rb").read())
    for call in range(calls):
        ro = O.run(om, ok, nsteps=nsteps, burnin=burnin, thin=thin, seed=seed, state=ost)
        assert (ro.status == 0).all()
        assert np.array_equal(_bits(rd.take(np.float64, (C, k, S))), _bits(ro.samples_cks)), ("samples", call)
        assert np.array_equal(_bits(rd.take(np.float64, (C, S))), _bits(ro.logpost)), ("logpost", call)
        assert np.array_equal(_bits(rd.take(np.float64, (C, k, S))), _bits(ro.draws_cks)), ("draws", call)
        assert np.array_equal(rd.take(np.int64, (C,)), ro.accept_count), ("accept_count", call)
        assert np.array_equal(rd.take(np.uint32, (C, W)), ro.accept_bits), ("accept_bits", call)
    assert np.array_equal(_bits(rd.take(np.float64, (C, k))), _bits(ost.theta0))
    assert np.array_equal(_bits(rd.take(np.float64, (C,))), _bits(ost.f0))
    abs_iter, Sigma, mean_prev = rd.take(np.int64, (C,)), rd.take(np.float64, (C, k, k)), rd.take(np.float64, (C, k))
    have_mean, nerrors = rd.take(np.int32, (C,)), rd.take(np.int32, (C,))
    if kind in (O.K_ADAPT, O.K_RAM):
        assert np.array_equal(abs_iter, ost.abs_iter)
        assert np.array_equal(_bits(Sigma), _bits(ost.Sigma))
        assert np.array_equal(nerrors, ost.nerrors)
    if kind == O.K_ADAPT:
        assert np.array_equal(have_mean, ost.have_mean) and have_mean.all()
        assert np.array_equal(_bits(mean_prev), _bits(ost.mean_prev))
