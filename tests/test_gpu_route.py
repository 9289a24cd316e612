"""The plan fmcmc_plan_route prints is the plan launch_sweep runs: for one small shape per launcher and register form (shapes
tests/test_gpu_parity.py runs too), fmcmc_last_kernel() after the run is the `form` planned for the device's own compute
units.  No fed logistic shape: there the shadow form, chosen at run time, legitimately differs from the plan."""
import numpy as np
import pytest

from conftest import set_knob

pytestmark = pytest.mark.gpu

LINREG, LOGISTIC = 1, 2
NORMAL, ADAPT, RAM = 1, 3, 4
# (family, p, n, kind, chains, kernel options, knobs, the form on a device of 256 compute units)
SHAPES = [
    (LINREG, 64, 200, NORMAL, 8, {}, {}, "big-k"),
    (LINREG, 1, 1000, NORMAL, 16, {}, {"pipe": 0}, "resident"),
    (LINREG, 3, 700, ADAPT, 8, {"bw": 5, "warmup": 5}, {}, "streamed"),
    (LINREG, 3, 5000, NORMAL, 16, {}, {"lat": 0}, "mfma"),
    (LINREG, 12, 5000, NORMAL, 16, {}, {"lat": 0}, "mfma-streamed"),
    (LINREG, 12, 5000, RAM, 8, {}, {}, "mfma-adaptive"),
    (LINREG, 3, 5000, NORMAL, 8, {}, {}, "lat1"),
    (LINREG, 3, 5000, NORMAL, 300, {"scheme": 1}, {}, "lat2"),
    (LINREG, 3, 5000, ADAPT, 8, {}, {}, "spec-lat1"),
    (LINREG, 3, 5000, ADAPT, 8, {}, {"lat": 0}, "spec"),
    (LOGISTIC, 4, 100, NORMAL, 300, {}, {}, "lat-logit2"),
    (LOGISTIC, 4, 100, ADAPT, 8, {}, {}, "spec-logit-lat1"),
    (LOGISTIC, 5, 3000, NORMAL, 8, {}, {"speclogit": 0}, "streamed-logistic"),
    (LOGISTIC, 5, 1573, NORMAL, 64, {}, {"shard": 1, "shadow": 0}, "logistic-sharded"),
    (LINREG, 20, 1500, NORMAL, 8, {}, {}, "streamed-wide"),
    (LINREG, 20, 1500, NORMAL, 512, {}, {"cw": 2, "shard": 1, "wide2": 0}, "streamed-wide-sharded-mfma"),
    (LINREG, 20, 3000, RAM, 37, {}, {}, "wide-dataflow"),
    (LINREG, 3, 4096, NORMAL, 1, {}, {"shard": 1}, "long-sharded"),
]


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fmcmc_amd import engine, _abi
    _abi.lib()
    return engine


@pytest.mark.parametrize("fam,p,n,kind,chains,opts,knobs,form256", SHAPES, ids=[s[-1] for s in SHAPES])
def test_the_planned_form_is_the_form_that_runs(E, monkeypatch, fam, p, n, kind, chains, opts, knobs, form256):
    import torch
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.kernels import DBL_MAX
    for key, value in knobs.items():
        set_knob(monkeypatch, key, value)
    rng = np.random.default_rng(1000 * p + chains)
    X = rng.standard_normal((n, p))
    beta = rng.uniform(-1.0, 1.0, p + 1)
    eta = beta[0] + X @ beta[1:]
    y = eta + 2.0 * rng.standard_normal(n) if fam == LINREG else (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    k = p + 1 + (1 if fam == LINREG else 0)
    init = np.concatenate([beta, [2.0]] if fam == LINREG else [beta])[None, :] + 0.01 * rng.standard_normal((chains, k))
    gm = E.DeviceModel(fam, X, y)
    gk = E.KernelSpec(kind, k, np.zeros(k), np.full(k, 0.01), np.full(k, -DBL_MAX), np.full(k, DBL_MAX), np.zeros(k, np.uint8), **opts)
    nsteps = 32
    # the same call with the kernel's host arrays, planned for this device's compute units
    hk = gk.c()
    hk.fixed, hk.lb, hk.ub, hk.scale = (a.ctypes.data for a in (gk.h_fixed, gk.h_lb, gk.h_ub, gk.h_scale))
    run = abi.Run(chains, nsteps, 0, 1, 7, 0, 0, abi.RNG_PHILOX, 0, None, None)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rc, line = abi.plan_route(gm.c(), hk, run, 0, ncu)
    assert rc == abi.OK, abi.last_error()
    plan = dict(kv.split("=", 1) for kv in line.split(" "))
    # (the long-data form is planned as a handle the launcher tries first; it reports itself once its launch ran)
    want = "long-sharded" if plan["kfn_long"] == "1" else plan["form"]
    if ncu == 256:
        assert want == form256, line
    E.sweep(gm, gk, E.ChainState(init, gk.kf), nsteps, seed=7, check=False)
    torch.cuda.synchronize()
    assert abi.last_kernel() == want, line
