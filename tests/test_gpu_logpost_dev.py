"""DeviceModel.logpost(theta) (fmcmc_logpost_dev, logpost_eval_kernel of mh_user.hpp) == the oracle's canonical log-posterior,
bit for bit: the three families at the edges of the 512 canonical lanes, with and without covariates, intercept and guard, at
one, three and 64 parameter vectors a call, and at the thetas where the closed forms branch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [1, 2, 511, 512, 513, 1025, 2049]
PS = [0, 1, 3, 15]
CS = [1, 3, 64]


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fmcmc_amd import engine
    return engine


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def data(fam, n, p, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) if p else None
    if fam == 2:
        y = (rng.uniform(size=n) < 0.4).astype(np.float64)
    else:
        y = 1.5 + (X @ np.linspace(1.0, -1.0, p) if p else 0.0) + 2.0 * rng.standard_normal(n)
    return X, y


def thetas(fam, k, X, seed):
    """64 parameter vectors: random ones, then the rows where the closed form branches"""
    rng = np.random.default_rng(seed)
    th = rng.standard_normal((64, k))
    if fam in (1, 3):   # Gaussian: sigma is the last parameter
        th[:, -1] = np.abs(th[:, -1]) + 0.3
        for r, s in enumerate([-1.0, 0.0, np.nan, 1e-300, -0.0, np.inf, 1e300]):
            th[r, -1] = s
    else:               # logistic: |eta| = 0, about 700, beyond the table's last row (|eta| >= 37.5), just inside it
        big = 1.0 if X is None else 1.0 / max(np.abs(X).max(), 1.0)
        th[0] = 0.0
        th[1] = 0.0; th[1, 0] = 700.0
        th[2] = 1000.0
        th[3] = 0.0; th[3, -1] = 37.5 * big
        th[4] = 0.0; th[4, 0] = -37.49
        th[5] = 1e-9 * th[5]
        th[6] = 1e5 * th[6]
    return th


def check(E, O, fam, X, y, intercept, guard, prior_div, seed):
    import torch
    om = O.Model(fam, X, y, intercept=intercept, guard=guard, prior_div=prior_div)
    gm = E.DeviceModel(fam, X, y, intercept=intercept, guard=guard, prior_div=prior_div)
    assert gm.k == om.k
    th = thetas(fam, om.k, X, seed)
    want = np.array([om.logpost(r) for r in th])
    dth = torch.as_tensor(th).cuda()
    for C in CS:
        for r0 in range(0, 9 if C < 64 else 1, C):   # (the branch rows 0 .. 6 are in the calls of every C)
            got = gm.logpost(dth[r0:r0 + C])
            assert got.dtype == torch.float64 and tuple(got.shape) == (C,)
            g = got.cpu().numpy()
            assert np.array_equal(bits(g), bits(want[r0:r0 + C])), (fam, len(y), intercept, guard, prior_div, C, r0, g, want[r0:r0 + C])


@pytest.mark.parametrize("n", NS)
def test_gaussian_linreg(E, O, n):
    for p in PS:
        X, y = data(1, n, p, 10 * n + p)
        for intercept in (True, False):
            for guard in (True, False):
                check(E, O, 1, X, y, intercept, guard, 0.0, n + p)


@pytest.mark.parametrize("n", NS)
def test_logistic(E, O, n):
    for p in PS:
        X, y = data(2, n, p, 20 * n + p)
        for intercept in (True, False):
            if p == 0 and not intercept:
                continue   # (no parameter at all)
            for guard in (True, False):
                for prior_div in (0.0, 8.0):
                    check(E, O, 2, X, y, intercept, guard, prior_div, n + p)


@pytest.mark.parametrize("n", NS)
def test_iid_normal(E, O, n):
    _, y = data(3, n, 0, 30 * n)
    for guard in (True, False):
        check(E, O, 3, None, y, True, guard, 0.0, n)


@pytest.mark.parametrize("fam,p", [(1, 3), (2, 3), (3, 0)])
def test_two_calls_on_one_model_equal_fresh_models(E, O, fam, p):
    """the logistic sums are formed once per call of the entry point: nothing of an earlier call is left behind"""
    import torch
    X, y = data(fam, 1025, p, 77 + fam)
    kw = dict(intercept=True, guard=False, prior_div=8.0 if fam == 2 else 0.0)
    om = O.Model(fam, X, y, **kw)
    gm = E.DeviceModel(fam, X, y, **kw)
    a, b = thetas(fam, om.k, X, 1)[7:20], thetas(fam, om.k, X, 2)[30:33]
    ga, gb = gm.logpost(torch.as_tensor(a).cuda()), gm.logpost(torch.as_tensor(b).cuda())
    fa = E.DeviceModel(fam, X, y, **kw).logpost(torch.as_tensor(a).cuda())
    fb = E.DeviceModel(fam, X, y, **kw).logpost(torch.as_tensor(b).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(bits(ga.cpu().numpy()), bits(fa.cpu().numpy()))
    assert np.array_equal(bits(gb.cpu().numpy()), bits(fb.cpu().numpy()))
    assert np.array_equal(bits(ga.cpu().numpy()), bits([om.logpost(r) for r in a]))
    assert np.array_equal(bits(gb.cpu().numpy()), bits([om.logpost(r) for r in b]))


def test_wide_models_up_to_the_parameter_ceiling(E, O):
    """k = 256 (FMCMC_MAX_K) in both regression families: the evaluator has no table or register bound below it"""
    import torch
    for fam, p in ((1, 254), (2, 255)):
        X, y = data(fam, 600, p, 5 + fam)
        om = O.Model(fam, X, y, intercept=True, guard=False, prior_div=8.0 if fam == 2 else 0.0)
        gm = E.DeviceModel(fam, X, y, intercept=True, guard=False, prior_div=8.0 if fam == 2 else 0.0)
        assert om.k == 256
        th = 0.05 * np.random.default_rng(fam).standard_normal((3, 256))
        th[:, -1] = np.abs(th[:, -1]) + 0.5
        got = gm.logpost(torch.as_tensor(th).cuda()).cpu().numpy()
        assert np.array_equal(bits(got), bits([om.logpost(r) for r in th]))


def test_argument_checks(E):
    import torch
    gm = E.DeviceModel(1, np.zeros((4, 1)), np.zeros(4))
    for bad in (np.zeros((2, 3)), torch.zeros((2, 3), dtype=torch.float64), torch.zeros((2, 2), dtype=torch.float64, device="cuda"),
                torch.zeros((2, 3), dtype=torch.float32, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError, match="theta must be a float64 tensor of shape"):
            gm.logpost(bad)
    assert tuple(gm.logpost(torch.zeros((0, 3), dtype=torch.float64, device="cuda")).shape) == (0,)
