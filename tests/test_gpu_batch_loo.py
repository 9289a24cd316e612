"""fmcmc_loo_groups_dev and loo() of an McmcBatch on the GPU: row d of the grouped call is the single call on dataset d's chains
to the bit (a Gaussian and a logistic family, 3 datasets x {1, 2, 5} chains, and a shape whose observations take the exact
fallback), an `active` mask leaves the rows of the switched-off groups as they were, McmcBatch.loo(models) is the list of
loo(ans[d], models[d]), and a ragged result takes one call per distinct row count."""
import ctypes as C
import importlib

import numpy as np
import pytest

import loo_cases as Lc
import waic_cases as W

pytestmark = pytest.mark.gpu

D = 3
FIELDS = ("elpd_loo", "p_loo", "lppd", "looic", "se_elpd", "se_p", "se_lppd", "se_looic", "n_k_bad", "n_k_very_bad", "max_k")


def batch(family, Cm, N, seed):
    """D datasets of one shape with Cm chains each: the cases, the model batch, and all chains [D Cm][k][S]"""
    import fmcmc_amd as F
    cases = [W.make_case(family, 70, 3, 1, Cm, N, seed=seed + d) for d in range(D)]
    return cases, F.model_batch(c.model for c in cases), np.ascontiguousarray(np.concatenate([c.samples for c in cases]))


def grouped_call(cases, models, x, active=None, prefill=float("nan")):
    import torch
    from fmcmc_amd import _abi as abi
    from fmcmc_amd.summary import loo_tail_len
    c0, L = cases[0], abi.lib()
    dm = models.device_model("cuda")
    cm = dm.c()
    M = loo_tail_len(c0.C * c0.N)
    xd = torch.as_tensor(x).cuda()
    lens = (L.fmcmc_loo_work_len(C.byref(cm), D, c0.C, c0.N), D * c0.n * 6, D * c0.n * M, D * 12)
    assert lens[0] > 0, abi.last_error()
    bufs = [torch.full((int(v) + W.GUARD,), prefill, dtype=torch.float64, device="cuda") for v in lens]
    ad = None if active is None else torch.as_tensor(np.asarray(active, dtype=np.int32)).cuda()
    rc = L.fmcmc_loo_groups_dev(C.byref(cm), dm.x_stride, dm.y_stride, xd.data_ptr(), D, c0.C, c0.k, x.shape[2], c0.row0, c0.N,
                                None if ad is None else ad.data_ptr(), *[b.data_ptr() for b in bufs], None)
    assert rc == abi.OK, (rc, abi.last_error())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs[1:]]
    for h, v in zip(host, lens[1:]):
        rest = h[int(v):]
        assert np.isnan(rest).all() if np.isnan(prefill) else (rest == prefill).all()
    return host[0][:lens[1]].reshape(D, c0.n, 6), host[1][:lens[2]].reshape(D, c0.n, M), host[2][:lens[3]].reshape(D, 12)


@pytest.mark.parametrize("family", ["linreg", "logistic"])
@pytest.mark.parametrize("Cm", [1, 2, 5])
def test_a_row_of_the_grouped_call_is_the_single_call(family, Cm):
    cases, models, x = batch(family, Cm, 523 if Cm == 2 else 37, seed=40 + Cm)
    got = grouped_call(cases, models, x)
    for d, c in enumerate(cases):
        one = Lc.device_loo(c)
        assert all(np.array_equal(Lc.bits(g[d]), Lc.bits(o)) for g, o in zip(got, one)), d


def test_a_group_that_takes_the_fallback_is_its_single_call():
    """S = 3 x 1200 = 3600 draws (M = 180): dataset 1 has 900 far-off draws outside the subsample, more than the capacity of
    an observation's buffer together with the ordinary ones above the threshold"""
    import fmcmc_amd as F
    Cm, N, n = 3, 1200, 20
    P = Lc.plan(Cm, N, n)
    assert P.ustride > 1 and P.cap < 900 + P.M
    cases = [Lc.big_case("linreg", n, 2, Cm, N, seed=90 + d, row0=5) for d in range(D)]
    win = cases[1].samples[:, :, 5:5 + N]
    insub = Lc.sub_rows_mask(P, Cm, N)
    for c in range(Cm):
        pick = np.flatnonzero(~insub[c])[:300]
        win[c, 0, pick] += 25.0 + 0.01 * np.arange(pick.size)
    for c_ in cases:
        Lc.finish_case(c_)
    models = F.model_batch(c.model for c in cases)
    x = np.ascontiguousarray(np.concatenate([c.samples for c in cases]))
    got = grouped_call(cases, models, x)
    for d, c in enumerate(cases):
        one = Lc.device_loo(c, want_state=True)
        assert all(np.array_equal(Lc.bits(g[d]), Lc.bits(o)) for g, o in zip(got, one[:3])), d
        assert (one[3][:, 3] == (1 if d == 1 else 0)).all(), d
    truth = F.loo_host(cases[1].model, cases[1].draws, Lc.LD)
    Lc.assert_matches(got[0][1], got[1][1], got[2][1], truth, Lc.emax_of(cases[1]), "fallback in a group")


def test_an_active_mask_leaves_the_other_rows_alone():
    cases, models, x = batch("linreg", 2, 37, seed=60)
    full = grouped_call(cases, models, x)
    got = grouped_call(cases, models, x, active=[1, 0, 1], prefill=-7.0)
    assert all((g[1] == -7.0).all() for g in got)
    for d in (0, 2):
        assert all(np.array_equal(Lc.bits(g[d]), Lc.bits(f[d])) for g, f in zip(got, full))


def hand_built(F, cases, x, nrows=None):
    import torch
    c0 = cases[0]
    kw = {} if nrows is None else dict(nrows=np.asarray(nrows), steps=np.asarray(nrows), converged=[True] * D)
    dc = F.DeviceChains(torch.as_tensor(x).cuda(), None, None, np.arange(1, c0.S + 1), 1, None, 0, D * c0.C)
    return F.McmcBatch(dc, D, c0.C, **kw)


def assert_equals_the_loop(F, ans, models, got, **kw):
    assert isinstance(got, F.LooBatch) and isinstance(got, list) and len(got) == D
    for d in range(D):
        one = F.loo(ans[d], models[d], **kw)
        assert np.array_equal(Lc.bits(got[d].pointwise), Lc.bits(one.pointwise)), d
        assert np.array_equal(Lc.bits(got.pointwise[d]), Lc.bits(one.pointwise)), d
        assert np.array_equal(Lc.bits(got.pareto_k[d]), Lc.bits(one.pareto_k)), d
        for f in FIELDS:
            assert np.array_equal(Lc.bits(getattr(got[d], f)), Lc.bits(getattr(one, f))), (d, f)
            assert np.array_equal(Lc.bits(getattr(got, f)[d]), Lc.bits(getattr(one, f))), (d, f)
        assert got[d].ndraws == one.ndraws and str(got[d]) == str(one)
        assert np.array_equal(got[d].pointwise_dev.cpu().numpy(), got[d].pointwise)


@pytest.mark.parametrize("family", ["linreg", "logistic"])
def test_loo_of_a_batch_is_loo_of_every_dataset(family):
    import fmcmc_amd as F
    cases, models, x = batch(family, 2, 37, seed=70)
    ans = hand_built(F, cases, x)
    assert_equals_the_loop(F, ans, models, ans.loo(models))
    assert_equals_the_loop(F, ans, models, F.loo(ans, models, autoburnin=True), autoburnin=True)
    cmp_ = F.loo_compare(ans.loo(models), ans.loo(models))
    assert cmp_.elpd_diff.shape == (D,) and (cmp_.elpd_diff == 0).all() and (cmp_.se_diff == 0).all()
    with pytest.raises(TypeError):
        ans.loo(models[0])


def test_a_ragged_batch_takes_one_call_per_distinct_row_count(monkeypatch):
    import fmcmc_amd as F
    S = importlib.import_module("fmcmc_amd.summary")       # (fmcmc_amd.summary is the function)
    cases, models, x = batch("linreg", 2, 37, seed=80)
    nrows = [30, 12, 30]
    for d, nr in enumerate(nrows):
        x[2 * d:2 * d + 2, :, nr:] = np.nan
    ans = hand_built(F, cases, x, nrows=nrows)
    assert ans.ragged
    calls, real = [], S.enqueue_loo_groups

    def counted(dc, dm, ngroups, cpg, row0, N, active=None, want_tail=False):
        calls.append((int(N), None if active is None else active.cpu().numpy().tolist()))
        return real(dc, dm, ngroups, cpg, row0, N, active, want_tail)

    monkeypatch.setattr(S, "enqueue_loo_groups", counted)
    got = ans.loo(models)
    assert calls == [(12, [0, 1, 0]), (30, [1, 0, 1])]
    monkeypatch.setattr(S, "enqueue_loo_groups", real)
    assert_equals_the_loop(F, ans, models, got)
