"""fmcmc_waic_groups_dev and waic() of an McmcBatch on the GPU: row d of the grouped call is the single call on dataset d's chains
to the bit (a Gaussian and a logistic family, 3 datasets x {1, 2, 5} chains), an `active` mask leaves the rows of the
switched-off groups as they were, McmcBatch.waic(models) is the list of waic(ans[d], models[d]), and a ragged result takes one
call per distinct row count."""
import ctypes as C
import importlib

import numpy as np
import pytest

import waic_cases as W

pytestmark = pytest.mark.gpu

D = 3
FIELDS = ("elpd_waic", "p_waic", "lppd", "waic", "se_elpd", "se_p", "se_lppd", "se_waic", "n_high")


def batch(family, Cm, N, seed):
    """D datasets of one shape with Cm chains each: the cases, the model batch, and all chains [D Cm][k][S]"""
    import fmcmc_amd as F
    cases = [W.make_case(family, 70, 3, 1, Cm, N, seed=seed + d) for d in range(D)]
    return cases, F.model_batch(c.model for c in cases), np.ascontiguousarray(np.concatenate([c.samples for c in cases]))


def grouped_call(cases, models, x, active=None, prefill=float("nan")):
    import torch
    from fmcmc_amd import _abi as abi
    c0, L = cases[0], abi.lib()
    dm = models.device_model("cuda")
    cm = dm.c()
    xd = torch.as_tensor(x).cuda()
    lens = (L.fmcmc_waic_work_len(C.byref(cm), D, c0.C, c0.N), D * c0.n * 4, D * 10)
    assert lens[0] > 0, abi.last_error()
    bufs = [torch.full((int(v) + W.GUARD,), prefill, dtype=torch.float64, device="cuda") for v in lens]
    ad = None if active is None else torch.as_tensor(np.asarray(active, dtype=np.int32)).cuda()
    rc = L.fmcmc_waic_groups_dev(C.byref(cm), dm.x_stride, dm.y_stride, xd.data_ptr(), D, c0.C, c0.k, c0.S, c0.row0, c0.N,
                                 None if ad is None else ad.data_ptr(), *[b.data_ptr() for b in bufs], None)
    assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for h, v in zip(host, lens):
        tail = h[int(v):]
        assert np.isnan(tail).all() if np.isnan(prefill) else (tail == prefill).all()
    return host[1][:lens[1]].reshape(D, c0.n, 4), host[2][:lens[2]].reshape(D, 10)


@pytest.mark.parametrize("family", ["linreg", "logistic"])
@pytest.mark.parametrize("Cm", [1, 2, 5])
def test_a_row_of_the_grouped_call_is_the_single_call(family, Cm):
    cases, models, x = batch(family, Cm, 523 if Cm == 2 else 37, seed=40 + Cm)
    point, total = grouped_call(cases, models, x)
    for d, c in enumerate(cases):
        one = W.device_waic(c)
        assert np.array_equal(W.bits(point[d]), W.bits(one[0])) and np.array_equal(W.bits(total[d]), W.bits(one[1])), d


def test_an_active_mask_leaves_the_other_rows_alone():
    cases, models, x = batch("linreg", 2, 37, seed=60)
    full = grouped_call(cases, models, x)
    point, total = grouped_call(cases, models, x, active=[1, 0, 1], prefill=-7.0)
    assert (point[1] == -7.0).all() and (total[1] == -7.0).all()
    for d in (0, 2):
        assert np.array_equal(W.bits(point[d]), W.bits(full[0][d])) and np.array_equal(W.bits(total[d]), W.bits(full[1][d]))


def hand_built(F, cases, x, nrows=None):
    import torch
    c0 = cases[0]
    kw = {} if nrows is None else dict(nrows=np.asarray(nrows), steps=np.asarray(nrows), converged=[True] * D)
    dc = F.DeviceChains(torch.as_tensor(x).cuda(), None, None, np.arange(1, c0.S + 1), 1, None, 0, D * c0.C)
    return F.McmcBatch(dc, D, c0.C, **kw)


def assert_equals_the_loop(F, ans, models, got, **kw):
    assert isinstance(got, F.WaicBatch) and isinstance(got, list) and len(got) == D
    for d in range(D):
        one = F.waic(ans[d], models[d], **kw)
        assert np.array_equal(W.bits(got[d].pointwise), W.bits(one.pointwise)), d
        assert np.array_equal(W.bits(got.pointwise[d]), W.bits(one.pointwise)), d
        for f in FIELDS:
            assert np.array_equal(W.bits(getattr(got[d], f)), W.bits(getattr(one, f))), (d, f)
            assert np.array_equal(W.bits(getattr(got, f)[d]), W.bits(getattr(one, f))), (d, f)
        assert got[d].ndraws == one.ndraws and str(got[d]) == str(one)
        assert np.array_equal(got[d].pointwise_dev.cpu().numpy(), got[d].pointwise)


@pytest.mark.parametrize("family", ["linreg", "logistic"])
def test_waic_of_a_batch_is_waic_of_every_dataset(family):
    import fmcmc_amd as F
    cases, models, x = batch(family, 2, 37, seed=70)
    ans = hand_built(F, cases, x)
    assert_equals_the_loop(F, ans, models, ans.waic(models))
    assert_equals_the_loop(F, ans, models, F.waic(ans, models, autoburnin=True), autoburnin=True)
    cmp_ = F.waic_compare(ans.waic(models), ans.waic(models))
    assert cmp_.elpd_diff.shape == (D,) and (cmp_.elpd_diff == 0).all() and (cmp_.se_diff == 0).all()
    with pytest.raises(TypeError):
        ans.waic(models[0])


def test_a_ragged_batch_takes_one_call_per_distinct_row_count(monkeypatch):
    import fmcmc_amd as F
    S = importlib.import_module("fmcmc_amd.summary")       # (fmcmc_amd.summary is the function)
    cases, models, x = batch("linreg", 2, 37, seed=80)
    nrows = [30, 12, 30]
    for d, nr in enumerate(nrows):
        x[2 * d:2 * d + 2, :, nr:] = np.nan
    ans = hand_built(F, cases, x, nrows=nrows)
    assert ans.ragged
    calls, real = [], S.enqueue_waic_groups

    def counted(dc, dm, ngroups, cpg, row0, N, active=None):
        calls.append((int(N), None if active is None else active.cpu().numpy().tolist()))
        return real(dc, dm, ngroups, cpg, row0, N, active)

    monkeypatch.setattr(S, "enqueue_waic_groups", counted)
    got = ans.waic(models)
    assert calls == [(12, [0, 1, 0]), (30, [1, 0, 1])]
    monkeypatch.setattr(S, "enqueue_waic_groups", real)
    assert_equals_the_loop(F, ans, models, got)
