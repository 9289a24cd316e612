"""fmcmc_ppc_dev, fmcmc_ppc_yrep_dev, ppc() and posterior_predict() on the GPU (csrc/diag_ppc.hpp): the exact cases bit for bit
against ppc_host(float64), every shape edge against ppc_host(longdouble) within the a-priori tolerances of tests/ppc_cases.py, the
bit-for-bit properties of the keys and of the fold, the contract of the entries, and MCMC() end to end.

Measured on an MI355X over all cases of this file: mean, sd and the chisq pair within 1.4e-15 (cap 1e-12), the largest min / max
error / dmax 0.59, every count equal to the host's."""
import ctypes as C
import time

import numpy as np
import pytest

import ppc_cases as Q

pytestmark = pytest.mark.gpu
LD = np.longdouble


def some_draws(case, rng, nsel):
    S = case.C * case.N
    flat = np.sort(rng.choice(S, size=min(nsel, S), replace=False))
    return flat, flat // case.N, flat % case.N


@pytest.mark.parametrize("spec", Q.EXACT, ids=lambda s: "%s-m%d-p%d-C%d-N%d" % s)
def test_exact_cases_bit_for_bit(spec):
    """integer X, theta and sigma: min and max bit for bit ppc_host(float64), all fifteen counts equal, the y_rep of selected draws
    bit for bit the host's, mean, sd and the two chisq within the cap; fmcmc_ppc_elem_host on the exact eta of one draw is the
    device's y_rep row"""
    from fmcmc_amd import _abi as abi
    case, kw = Q.exact_shape_case(spec)
    stats, total = Q.device_ppc(case, **kw)
    want = Q.host(case, np.float64, **kw)
    got = Q.flat(stats)
    assert total[0] == case.C * case.N and total[1] == 0
    assert np.array_equal(Q.bits(got[:, 2:4]), Q.bits(want.stats[:, 2:4]))
    assert np.array_equal(Q.counts_of(total), want.counts), (Q.counts_of(total).tolist(), want.counts.tolist())
    cols = [0, 4, 5] + ([1] if case.m > 1 else [])
    em = Q.metric(got[:, cols], Q.host(case, LD, **kw).stats[:, cols])
    print("%s: mean / sd / chisq %.3g (cap %.3g)" % (case.name, float(em.max()), Q.CAP))
    assert (em <= Q.CAP).all()
    if case.m == 1:
        assert np.isnan(got[:, 1]).all()
    flat, sc, sr = some_draws(case, np.random.default_rng(1), 21)
    yrep = Q.device_yrep(case, sc, sr, **kw)
    assert np.array_equal(Q.bits(yrep), Q.bits(want.yrep[flat]))
    s = int(flat[-1])
    chain_ids, ids = Q.keys(case, **kw)
    eta = np.ascontiguousarray(want.eta[s])
    out, var = np.empty(case.m), np.empty(case.m)
    sigma = float(case.draws[s, -1]) if case.family != "logistic" else 1.0
    rc = abi.lib().fmcmc_ppc_elem_host(int(case.model.family), Q.SEED, int(chain_ids[s]), int(ids[s]), case.m, eta.ctypes.data,
                                       sigma, out.ctypes.data, var.ctypes.data)
    assert rc == abi.OK and np.array_equal(Q.bits(out), Q.bits(yrep[-1]))


@pytest.mark.parametrize("spec", Q.SHAPES, ids=lambda s: "%s-m%d-p%d-ic%d-C%d-N%d" % s)
def test_shape_edges_within_the_tolerances(spec):
    case, kw = Q.shape_case(spec)
    stats, total = Q.device_ppc(case, **kw)
    Q.assert_general(case, stats, total, Q.host(case, LD, **kw))
    if case.family == "logistic":                        # no element can flip: the host's 0 / 1 values, folded alike
        want = Q.host(case, np.float64, **kw)
        assert np.array_equal(Q.bits(Q.flat(stats)[:, :4]), Q.bits(want.stats[:, :4]))
        assert np.array_equal(Q.counts_of(total)[:4], want.counts[:4])


@pytest.fixture(scope="module")
def wide():
    """three chains of 50 rows, n = 33, five operand columns"""
    case = Q.general_case(("linreg", 33, 4, 1, 3, 50), seed=77)
    return case, Q.device_ppc(case)


def test_two_calls_give_the_same_bits(wide):
    case, (stats, total) = wide
    again = Q.device_ppc(case)
    assert np.array_equal(Q.bits(stats), Q.bits(again[0])) and np.array_equal(Q.bits(total), Q.bits(again[1]))


def test_a_draws_numbers_do_not_depend_on_the_call(wide):
    """(C = 1, N = 16) of the same buffer: the six numbers of the draws it shares with (C = 3, N = 50)"""
    case, (stats, _total) = wide
    one, total = Q.device_ppc(case, chains=1, N=16)
    assert total[0] == 16 and np.array_equal(Q.bits(one[0]), Q.bits(stats[0][:, :16]))


def test_the_window_may_sit_anywhere_and_the_ids_follow_the_draws(wide):
    """the window moved inside another buffer; a later window of the same buffer with id0 moved along, and the chains taken as
    chains 7 .. 9 with chain_base lowered by 7 ... the draws keep their ids, so they keep their numbers"""
    case, (stats, total) = wide
    rng = np.random.default_rng(5)
    S2, row2 = case.S + 40, 22
    moved = rng.standard_normal((case.C, case.k, S2)) + 3.0
    moved[:, -1] = np.abs(moved[:, -1]) + 0.5
    moved[:, :, row2:row2 + case.N] = case.samples[:, :, case.row0:case.row0 + case.N]
    got = Q.device_ppc(case, samples=moved, row0=row2)
    assert np.array_equal(Q.bits(stats), Q.bits(got[0])) and np.array_equal(Q.bits(total), Q.bits(got[1]))
    late, _ = Q.device_ppc(case, row0=case.row0 + 10, N=case.N - 10, id0=Q.ID0 + 10)
    assert np.array_equal(Q.bits(late), Q.bits(stats[:, :, 10:]))
    shifted, _ = Q.device_ppc(case, samples=np.ascontiguousarray(case.samples[1:]), chain_base=1)
    assert np.array_equal(Q.bits(shifted), Q.bits(stats[1:]))


def test_another_seed_or_other_ids_change_the_result(wide):
    case, (stats, _total) = wide
    for kw in (dict(seed=Q.SEED + 1), dict(id0=Q.ID0 + 1), dict(chain_base=1), dict(id_step=2)):
        other, _ = Q.device_ppc(case, **kw)
        assert not np.array_equal(Q.bits(other[:, :, 1:]), Q.bits(stats[:, :, 1:])), kw
    step2, _ = Q.device_ppc(case, id_step=2)                        # (row 0 keeps its id; chisq_obs has no variate in it)
    assert np.array_equal(Q.bits(step2[:, :, 0]), Q.bits(stats[:, :, 0]))
    assert np.array_equal(Q.bits(step2[:, 5]), Q.bits(stats[:, 5]))


@pytest.mark.parametrize("family", ("linreg", "logistic"))
def test_the_stats_are_the_fold_of_the_devices_own_yrep(family):
    """every draw's y_rep through fmcmc_ppc_yrep_dev (more than one launch of selections), folded on the host: the device's min
    and max exactly, and with ppc_fold in float64 its mean and sd too (the same operations in the same order)"""
    from fmcmc_amd.summary import ppc_fold
    case = Q.general_case((family, 33, 4, 1, 3, 50), seed=78)
    stats, _total = Q.device_ppc(case)
    S = case.C * case.N
    flat = np.arange(S)
    yrep = Q.device_yrep(case, flat // case.N, flat % case.N)
    got = Q.flat(stats)
    assert np.array_equal(Q.bits(got[:, 2]), Q.bits(yrep.min(axis=1))) and np.array_equal(Q.bits(got[:, 3]), Q.bits(yrep.max(axis=1)))
    fold = ppc_fold(yrep, np.zeros_like(yrep), np.zeros_like(yrep))
    assert np.array_equal(Q.bits(got[:, :4]), Q.bits(fold[:, :4]))
    if family == "logistic":
        assert set(np.unique(yrep)) <= {0.0, 1.0}


def test_bad_draws_are_counted_and_refused():
    import torch
    import fmcmc_amd as F
    for family, bad in (("linreg", 2), ("logistic", 1)):
        case = Q.general_case((family, 17, 2, 1, 2, 33), seed=3)
        x = case.samples.copy()
        x[1, 1, case.row0 + 20] = np.nan
        if family == "linreg":
            x[0, case.k - 1, case.row0 + 4] = 0.0
        x[0, 0, 0] = np.nan                                 # outside the window: not a draw
        stats, total = Q.device_ppc(case, samples=x)
        assert total[1] == bad and total[0] == 66
        assert total[2 + 14] >= 1 and np.isnan(stats[1, 5, 20])     # (the chisq_obs of that draw is not finite)
        window = np.ascontiguousarray(x[:, :, case.row0:case.row0 + case.N])
        dc = F.DeviceChains(torch.as_tensor(window).cuda(), None, None, np.arange(1, case.N + 1), 1, None, 0, case.C)
        with pytest.raises(ValueError, match="%d draw" % bad):
            F.ppc(dc, case.model)


def test_the_refusals_come_before_any_device_call():
    import torch
    from fmcmc_amd import _abi as abi
    case = Q.general_case(("linreg", 17, 2, 1, 1, 33), seed=4)
    L_, cm = abi.lib(), case.model.device_model("cuda").c()
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda")
    tobs = np.zeros(4).ctypes.data_as(C.POINTER(C.c_double))
    args = lambda k=case.k, S=40, row0=0, N=33, base=0, id0=1, step=1, Cn=1, m=cm: (
        C.byref(m), buf.data_ptr(), Cn, k, S, row0, N, 1, base, id0, step, tobs, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None)
    assert L_.fmcmc_ppc_dev(*args(k=case.k - 1)) == abi.ERR_ARG and "family has 4" in abi.last_error()
    assert L_.fmcmc_ppc_dev(*args(N=1)) == abi.ERR_ARG and "at least 2" in abi.last_error()
    assert L_.fmcmc_ppc_dev(*args(row0=8)) == abi.ERR_ARG and "outside" in abi.last_error()
    assert L_.fmcmc_ppc_dev(*args(id0=2 ** 32 - 32)) == abi.ERR_UNSUPPORTED and "32 bits" in abi.last_error()
    assert L_.fmcmc_ppc_dev(*args(id0=2 ** 32 - 33)) == abi.OK
    assert L_.fmcmc_ppc_dev(*args(step=2 ** 27)) == abi.ERR_UNSUPPORTED and "32 bits" in abi.last_error()
    assert L_.fmcmc_ppc_dev(*args(base=2 ** 32)) == abi.ERR_UNSUPPORTED and "chain ids" in abi.last_error()
    assert L_.fmcmc_ppc_dev(*args(base=-1)) == abi.ERR_ARG and L_.fmcmc_ppc_dev(*args(step=0)) == abi.ERR_ARG
    iid = abi.Model(abi.FAM_IID_NORMAL, 0, 17, None, cm.y, 1, 0, 0.0)
    assert L_.fmcmc_ppc_dev(*args(k=2, m=iid)) == abi.ERR_UNSUPPORTED and "iid_normal" in abi.last_error()
    assert L_.fmcmc_ppc_work_len(C.byref(iid), 1, 33) == 0 and L_.fmcmc_ppc_work_len(C.byref(cm), 1, 1) == 0
    assert L_.fmcmc_ppc_work_len(C.byref(cm), 1, 33) == 2 + 16

    i64 = lambda *v: np.asarray(v, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    many = np.zeros(65536, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    yargs = lambda sc=i64(0), sr=i64(5), nsel=1, id0=1, m=cm: (
        C.byref(m), buf.data_ptr(), 1, case.k, 40, 1, 0, id0, 1, sc, sr, nsel, buf.data_ptr(), None)
    assert L_.fmcmc_ppc_yrep_dev(*yargs(sc=many, sr=many, nsel=65536)) == abi.ERR_UNSUPPORTED and "65535" in abi.last_error()
    assert L_.fmcmc_ppc_yrep_dev(*yargs(nsel=0)) == abi.ERR_ARG
    assert L_.fmcmc_ppc_yrep_dev(*yargs(sr=i64(40))) == abi.ERR_ARG and "outside" in abi.last_error()
    assert L_.fmcmc_ppc_yrep_dev(*yargs(sc=i64(1))) == abi.ERR_ARG and "outside" in abi.last_error()
    assert L_.fmcmc_ppc_yrep_dev(*yargs(sr=i64(-1))) == abi.ERR_ARG
    assert L_.fmcmc_ppc_yrep_dev(*yargs(id0=2 ** 32 - 5)) == abi.ERR_UNSUPPORTED and "32 bits" in abi.last_error()
    assert L_.fmcmc_ppc_yrep_dev(*yargs(m=iid)) == abi.ERR_UNSUPPORTED
    assert L_.fmcmc_ppc_yrep_dev(*yargs()) == abi.OK
    torch.cuda.synchronize()


def test_the_call_stays_on_the_callers_stream(wide):
    """behind a gate on a side stream, with the draws written on that stream after the gate: the bits of the ungated call, and
    the call returns while the gate is closed"""
    import torch
    from test_gpu_streams import Gate, decoy, quiet_host, side_streams
    case, (stats, total) = wide
    side = side_streams()[0]
    seen = {}

    def run(inputs, bufs, call):
        xd = inputs[0]
        true = xd.clone()
        xd.copy_(decoy(xd))
        quiet_host()
        gate = Gate(side)
        with torch.cuda.stream(side):
            xd.copy_(true)
            for b in bufs:
                b.fill_(float("nan"))
            t0 = time.perf_counter()
            rc = call(C.c_void_p(side.cuda_stream))
            seen["closed"], seen["ms"] = gate.closed(), 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        seen["gate"] = gate
        return rc

    got = Q.device_ppc(case, run=run)
    assert seen["closed"], seen["gate"].too_short(seen["ms"])
    assert np.array_equal(Q.bits(stats), Q.bits(got[0])) and np.array_equal(Q.bits(total), Q.bits(got[1]))


def test_ppc_through_the_public_api():
    """MCMC() of a 100 x 3 regression, 4 chains x 400 steps: ans.ppc(model) against ppc_host of the copied draws with the keys
    of the result; the derived chain under summary() and hpd_interval() against numpy on its copy; posterior_predict's shape,
    selection and bits; the logistic family the same way; what is refused"""
    import torch
    from types import SimpleNamespace
    import fmcmc_amd as F
    from fmcmc_amd.summary import PPC_NAMES
    rng = np.random.default_rng(12)
    n = 100
    X = rng.uniform(-2, 2, (n, 3))
    lin = 0.5 + X @ [1.5, -1.0, 0.25]
    fits = (("linreg", F.gaussian_linreg(X, lin + rng.standard_normal(n)), [0.5, 1.5, -1.0, 0.25, 1.0], 0.05),
            ("logistic", F.logistic(X, (rng.uniform(size=n) < 1 / (1 + np.exp(-lin))).astype(float), intercept=True),
             [0.5, 1.5, -1.0, 0.25], 0.15))
    for family, model, start, scale in fits:
        init = np.asarray(start) + 0.01 * np.arange(4)[:, None]
        dc = F.MCMC(init, model, 400, seed=8, nchains=4, burnin=40, thin=2, kernel=F.kernel_normal(scale=scale), _return_device=True)
        res = dc.ppc(model, seed=3)
        assert isinstance(res, F.PpcResult) and res.bad_draws == 0
        smp = dc.samples.cpu().numpy()
        Cn, _k, N = smp.shape
        assert res.ndraws == Cn * N and res.stats.samples.shape == (Cn, 6, N)
        assert res.stats.names == list(PPC_NAMES) and res.stats.logpost is None and res.stats.draws is None
        assert np.array_equal(res.stats.iters, dc.iters) and res.stats.thin == dc.thin and res.stats.chain_base == dc.chain_base
        case = SimpleNamespace(family=family, m=n, p=3, ic=1, C=Cn, N=N, model=model, name="MCMC " + family,
                               draws=np.ascontiguousarray(smp.transpose(0, 2, 1).reshape(Cn * N, -1)))
        c, r = np.divmod(np.arange(Cn * N), N)
        truth = F.ppc_host(model, case.draws, dc.chain_base + c, np.asarray(dc.iters)[r], seed=3, dtype=LD)
        host_stats = np.ascontiguousarray(res.stats.to_host().as_array().transpose(0, 2, 1))    # [C][6][N]
        assert np.array_equal(Q.bits(host_stats), Q.bits(res.stats.samples.cpu().numpy()))
        cols = [0, 1, 4, 5]
        em = Q.metric(Q.flat(host_stats)[:, cols], truth.stats[:, cols])
        ext = np.abs(Q.flat(host_stats)[:, 2:4].astype(LD) - truth.stats[:, 2:4])
        diff = np.abs(res.counts - truth.counts).max(axis=1)
        print("%s: mean / sd / chisq %.3g, counts differ by %s, near %s, p %s" % (case.name, float(em.max()), diff.tolist(),
                                                                                 truth.near.tolist(), res.pvalue))
        assert (em <= Q.CAP).all() and (ext <= truth.dmax[:, None]).all() and len(truth.flips) == 0
        if family == "linreg":                              # (the logistic mean ties with T(y) for many draws: see ppc_cases.py)
            assert (diff <= truth.near).all()
            assert all(0.0 < res.pvalue[s] < 1.0 for s in ("mean", "sd", "chisq"))
        else:                                               # no flip: the counts of the host's float64 fold of the same 0 / 1 values
            same = F.ppc_host(model, case.draws, dc.chain_base + c, np.asarray(dc.iters)[r], seed=3)
            assert np.array_equal(res.counts[:4], same.counts[:4]) and diff[4] <= truth.near[4]
        assert all(abs(res.pvalue[s] - (res.counts[j, 0] + res.counts[j, 1]) / res.ndraws) < 1e-15 for j, s in enumerate(abi_stats()))
        text = str(res)
        assert "Posterior predictive check from %d draws" % res.ndraws in text and "chisq" in text and "T(y)" in text
        # the derived chain under the existing diagnostics
        flat = Q.flat(host_stats)
        sm = F.summary(res.stats)
        assert np.allclose(sm.statistics[:, 0], flat.mean(axis=0), rtol=1e-12, atol=1e-12)
        assert np.allclose(sm.statistics[:, 1], flat.std(axis=0, ddof=1), rtol=1e-10, atol=1e-12)
        assert np.allclose(sm.quantiles, np.quantile(flat, sm.probs, axis=0).T, rtol=1e-12, atol=1e-12)
        hp = F.hpd_interval(res.stats, 0.9)
        for ch in range(Cn):
            for j in range(6):
                srt = np.sort(host_stats[ch, j])
                width = srt[hp.gap:] - srt[:N - hp.gap]
                assert hp.lower[ch, j] == srt[hp.index[ch, j]] and hp.upper[ch, j] == srt[hp.index[ch, j] + hp.gap]
                assert hp.upper[ch, j] - hp.lower[ch, j] == width.min()
        # posterior_predict
        yr = dc.posterior_predict(model, ndraws=7, seed=3)
        assert tuple(yr.shape) == (7, n) and yr.is_cuda
        sc, sr = F.posterior_predict_selection(Cn, N, 7)
        sel = sc * N + sr
        yh = yr.cpu().numpy()
        assert np.array_equal(Q.bits(yh.min(axis=1)), Q.bits(flat[sel, 2])) and np.array_equal(Q.bits(yh.max(axis=1)), Q.bits(flat[sel, 3]))
        half = F.ppc(dc, model, seed=3, autoburnin=True)
        assert half.ndraws < res.ndraws
        keep = N - half.ndraws // Cn
        assert np.array_equal(Q.bits(half.stats.samples.cpu().numpy()), Q.bits(host_stats[:, :, keep:]))
    with pytest.raises(ValueError, match="iid_normal"):
        F.ppc(dc, F.iid_normal(np.zeros(5)))
    with pytest.raises(TypeError, match="regression families"):
        F.ppc(dc, F.pointwise_fun(lambda th: th, 5, 2))
    torch.cuda.synchronize()


def abi_stats():
    from fmcmc_amd import _abi as abi
    return abi.PPC_STATS


def test_a_dataset_of_a_batch_is_its_chains_alone():
    import fmcmc_amd as F
    rng = np.random.default_rng(21)
    n, D = 40, 2
    X = rng.uniform(-2, 2, (D, n, 2))
    models = F.model_batch([F.gaussian_linreg(X[d], 0.5 + X[d] @ [1.0, -0.5] + rng.standard_normal(n)) for d in range(D)])
    init = np.array([0.5, 1.0, -0.5, 1.0]) + 0.01 * np.arange(2)[:, None]
    ans = F.MCMC_batch(init, models, 200, seed=5, nchains=2, burnin=20, kernel=F.kernel_normal(scale=0.05))
    with pytest.raises(TypeError, match=r"ppc\(ans\[d\], models\[d\]\)"):
        F.ppc(ans, models)
    with pytest.raises(TypeError, match=r"posterior_predict\(ans\[d\], models\[d\]\)"):
        F.posterior_predict(ans, models)
    got = F.ppc(ans[1], models[1])
    alone = F.DeviceChains(ans[1].samples.clone().contiguous(), None, None, ans[1].iters, ans[1].thin, None, ans[1].chain_base, 2)
    ref = F.ppc(alone, models[1])
    assert np.array_equal(Q.bits(got.stats.samples.cpu().numpy()), Q.bits(ref.stats.samples.cpu().numpy()))
    assert np.array_equal(got.counts, ref.counts) and got.ndraws == 2 * 180
