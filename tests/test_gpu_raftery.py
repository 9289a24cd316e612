"""GPU tests of the device-side Raftery-Lewis diagnostic and of the per-chain order statistics (fmcmc_amd/summary.py:
raftery_diag, chain_quantiles -> csrc/raftery.hip: raftery_kernel, chain_order_kernel).

The device part is integer counting plus one exact selection, and both paths end in summary.raftery_finish, so there is no
tolerance anywhere: order statistics, the threshold u, the triple counts and last pairs, kthin, M, N and I are compared with
np.array_equal or bit for bit (NaN where the reference is NaN) against the host restatement (convergence.raftery_diag,
raftery_threshold, raftery_counts; np.sort for the order statistics) on the host copy of the same rows.  The looser
(q, r, s) = (0.25, 0.05, 0.9) and (0.5, 0.1, 0.8), with nmin = 203 and 42, keep the shapes small."""
import time

import numpy as np
import pytest

from test_gpu_summary import _bits, ar1, upload
from test_gpu_summary_edges import device_chains

pytestmark = pytest.mark.gpu
LDS_ROWS = 19456        # csrc/raftery.hip: rows of a series whose keys are staged in LDS
BATCH = 16              # summary.RAFTERY_BATCH: thinnings per launch
Q25, Q50 = (0.25, 0.05, 0.9), (0.5, 0.1, 0.8)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same(got, want):
    """NaN where the other is NaN, the same bits elsewhere."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(
        _bits(got[~np.isnan(got)]), _bits(want[~np.isnan(want)]))


def same_u(got, want):
    """The threshold: the same bits, except that a zero may carry either sign (np.sort leaves the order of -0.0 and +0.0 open;
    the device puts -0.0 first; x <= u does not depend on it)."""
    got, want = np.asarray(got), np.asarray(want)
    return np.array_equal(got, want) and np.array_equal(_bits(got[want != 0]), _bits(want[want != 0]))


def device_counts(dc, q, j0, nj, cols=None):
    """(head [C][p][4], tri [C][p][nj][8], last_pair [C][p][nj][2]) as fmcmc_raftery_dev left them."""
    from fmcmc_amd.summary import enqueue_raftery
    head, cnt, _work, _ = enqueue_raftery(dc, q, j0, nj, cols)
    cnt = cnt.cpu().numpy()
    return head.cpu().numpy(), cnt[..., :8], cnt[..., 8:]


def check(dc, qrs, cols=None, batches=2):
    """Everything the device returns for `dc` against the host restatement, chain by chain.  Returns (RafteryDiag, host kthin)."""
    from fmcmc_amd.convergence import raftery_counts, raftery_diag, raftery_threshold
    from fmcmc_amd.summary import raftery_bound, raftery_search
    host = dc.samples.cpu().numpy()                                   # [C][k][N]
    C_, k, N = host.shape
    cols_ = list(range(k)) if cols is None else list(cols)
    q = qrs[0]
    iters = np.asarray(dc.iters)
    thin = int(iters[1] - iters[0])
    nmin = raftery_bound(*qrs)[1]
    rd = dc.raftery_diag(*qrs, cols=cols)
    assert rd.table.shape == (C_, len(cols_), 4) and rd.kthin.shape == (C_, len(cols_)) and rd.nmin == nmin
    kthin = np.full((C_, len(cols_)), np.nan)
    heads = [device_counts(dc, q, 1 + b * BATCH, BATCH, cols) for b in range(batches)]
    for c in range(C_):
        data = host[c].T[:, cols_]
        assert same(rd.table[c], raftery_diag(data, iters, *qrs)), c
        u = raftery_threshold(data, q)
        srt = np.sort(data, axis=0)
        Z = data <= u[None, :]
        for b, (head, tri, last) in enumerate(heads):
            assert same_u(head[c, :, 0], u), c
            assert np.all(head[c, :, 3] == 0)
            assert np.all((head[c, :, 1] <= u) & (u <= head[c, :, 2])) and np.all(np.isin(head[c, :, 1:3], srt))
            wt, wl = raftery_counts(Z, 1 + b * BATCH, BATCH)
            assert np.array_equal(tri[c], wt) and np.array_equal(last[c], wl), (c, b)
        if nmin <= N:
            assert same_u(rd.u[c], u)
            fin = raftery_search(lambda j0, nj: raftery_counts(Z, j0, nj), N, thin, *qrs)
            kthin[c] = fin.kthin
            assert same(rd.kthin[c], fin.kthin) and same(rd.alpha[c], fin.alpha) and same(rd.beta[c], fin.beta)
    return rd, kthin


def mixed(N, seed, chains=2):
    """[chains][N][3]: an iid column, an AR(1) column far from 0, and one rounded to a tenth (many exact repeats; + 0.0 turns
    the -0.0 of np.round into +0.0, so that the order statistics have one set of bits)."""
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.standard_normal(N), ar1(0.9, N, rng, mu=-40.0), np.round(ar1(0.7, N, rng), 1) + 0.0], axis=1)
                     for _ in range(chains)])


# ------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("qrs,N", [(Q25, 202), (Q25, 203), (Q25, 204), (Q50, 41), (Q50, 42), (Q50, 43)])
def test_rows_around_nmin(qrs, N):
    rd, _ = check(upload(mixed(N, N)), qrs)
    nmin = 203 if qrs is Q25 else 42
    assert np.all(rd.table[:, :, 2] == nmin)
    if N < nmin:
        assert np.all(np.isnan(rd.table[:, :, [0, 1, 3]])) and "at least %d" % nmin in str(rd)


@pytest.mark.parametrize("N", (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, LDS_ROWS - 1, LDS_ROWS, LDS_ROWS + 1))
def test_lengths_at_the_word_block_and_tile_edges(N):
    """64-row words of the indicator, 512-row steps of the workgroup, 4096-row steps of the staging loop, and the LDS tile:
    19456 rows are held in LDS, 19457 are re-read from global memory every pass."""
    rd, _ = check(upload(mixed(N, N)), Q25)
    assert np.all(rd.table[:, :, 2] == 203)


def test_many_pass_global_path():
    """N = 200003: 49 steps of the staging loop per walk, ten walks over global memory, 3126 words of indicator a series."""
    rd, _ = check(upload(mixed(200003, 200003, chains=1)), (0.025, 0.005, 0.95))
    assert np.all(np.isfinite(rd.table)) and rd.nmin == 3746


# ------------------------------------------------------------------------------------------------ thinning
@pytest.mark.parametrize("N", (3, 4, 5, 31, 32, 33, 42, 47, 48, 49, 64, 65))
def test_thinned_length_crosses_3_within_a_batch(N):
    """m = ceil(N / j) falls to 3, 2 and 1 inside the thinnings 1 .. 80 asked for in three launches: the counts are 0 from
    m < 3 on and the last pair is that of the rows left."""
    from fmcmc_amd.convergence import raftery_counts, raftery_threshold
    dc = upload(mixed(N, 1000 + N))
    host = dc.samples.cpu().numpy()
    for j0, nj in ((1, 32), (33, 32), (65, 16)):
        head, tri, last = device_counts(dc, 0.5, j0, nj)
        for c in range(2):
            data = host[c].T
            Z = data <= raftery_threshold(data, 0.5)[None, :]
            wt, wl = raftery_counts(Z, j0, nj)
            assert np.array_equal(tri[c], wt) and np.array_equal(last[c], wl), (j0, c)
        m = -(-N // np.arange(j0, j0 + nj))
        assert np.all(tri[:, :, m < 3] == 0) and np.all(tri[:, :, m >= 3].sum(-1) == (m[m >= 3] - 2))


def test_kthin_beyond_the_first_batch(monkeypatch):
    """sin(2 pi t / 64), n = 8000, q = 0.25: the first thinning with BIC < 0 is 26, in the second launch; the iid series of
    the same call are decided in the first.  A call of iid series alone launches once."""
    import importlib
    S = importlib.import_module("fmcmc_amd.summary")     # (fmcmc_amd.summary is the function)
    rng = np.random.default_rng(8000)
    n = 8000
    arr = rng.standard_normal((3, n, 2))
    arr[1, :, 0] = np.sin(2 * np.pi * np.arange(n) / 64)
    launches = []
    real = S.enqueue_raftery
    monkeypatch.setattr(S, "enqueue_raftery", lambda dc, q, j0, nj, cols: launches.append((j0, nj)) or real(dc, q, j0, nj, cols))
    rd, kthin = check(upload(arr), Q25)
    assert kthin[1, 0] == 26 and np.all(np.delete(kthin.ravel(), 2) == 1)
    assert np.array_equal(rd.kthin, kthin)
    assert launches[:2] == [(1, BATCH), (1 + BATCH, BATCH)]
    del launches[:]
    upload(arr[[0, 2]]).raftery_diag(*Q25)
    assert launches == [(1, BATCH)]


# ------------------------------------------------------------------------------------------------ values
@pytest.fixture(scope="module")
def sweep48(readme_data):
    from fmcmc_amd import MCMC, gaussian_linreg, kernel_normal
    X, y = readme_data
    init = np.array([0.0, 0.0, np.std(y, ddof=1)])[None, :] + 0.1 * np.random.default_rng(48).standard_normal((48, 3))
    init[:, 2] = np.abs(init[:, 2])
    return MCMC(init, gaussian_linreg(X, y), 2000, nchains=48, seed=11, kernel=kernel_normal(scale=0.6), _return_device=True)


def test_sweep_output_with_rejected_steps(sweep48):
    """A real sweep with a wide proposal: most steps are rejected, so a row repeats the one before it exactly; x_(lo) == x_(hi)
    in many series and ties straddle u."""
    host = sweep48.samples.cpu().numpy()
    assert (host[:, :, 1:] == host[:, :, :-1]).mean() > 0.5
    from fmcmc_amd.summary import enqueue_raftery
    for qrs in (Q25, Q50):
        check(sweep48, qrs)
        head = enqueue_raftery(sweep48, qrs[0], 1, 1, None)[0].cpu().numpy()
        assert (head[:, :, 1] == head[:, :, 2]).sum() > 10


def test_adjacent_doubles_around_the_threshold():
    """n = 204, q = 0.25: index = 51.75, so h = 0.75 between the 51st and 52nd values, which are made neighbouring doubles
    (and, in column 1, the same pair with a tie on each side)."""
    rng = np.random.default_rng(204)
    arr = rng.standard_normal((2, 204, 2)) + 5.0
    for c in range(2):
        for j in range(2):
            order = np.argsort(arr[c, :, j])
            arr[c, order[51], j] = np.nextafter(arr[c, order[50], j], np.inf)
            if j == 1:
                arr[c, order[49], j] = arr[c, order[50], j]
                arr[c, order[52], j] = arr[c, order[51], j]
    dc = upload(arr)
    check(dc, Q25)
    head, _, _ = device_counts(dc, 0.25, 1, 1)
    assert np.all(np.nextafter(head[:, :, 1], np.inf) == head[:, :, 2])
    assert np.all((head[:, :, 0] == head[:, :, 1]) | (head[:, :, 0] == head[:, :, 2]))


def test_signed_zeros_negative_columns_and_extreme_ranks():
    """-0.0 beside +0.0 at the threshold (they compare equal: the indicator does not depend on which of them the selection
    returns, and np.array_equal treats them alike); a column of negative values only; q whose lower order statistic is the
    smallest value (rank 0) and the second largest (rank n - 2)."""
    rng = np.random.default_rng(500)
    n = 500
    arr = np.empty((2, n, 3))
    for c in range(2):
        z = rng.standard_normal(n)
        z[np.abs(z) < 0.6] = 0.0
        z[rng.random(n) < 0.5] *= -1.0                       # -0.0 and +0.0 mixed, and the signs of the rest
        arr[c, :, 0] = z
        arr[c, :, 1] = -np.exp(ar1(0.5, n, rng))
        arr[c, :, 2] = ar1(0.3, n, rng, mu=2.0)
    assert np.signbit(arr[:, :, 0][arr[:, :, 0] == 0]).any() and not np.signbit(arr[:, :, 0][arr[:, :, 0] == 0]).all()
    dc = upload(arr)
    for qrs in (Q50, Q25, (0.001, 0.05, 0.9), (0.999, 0.05, 0.9)):
        check(dc, qrs)
    from fmcmc_amd.summary import host_chain_order, enqueue_chain_order
    host = dc.samples.cpu().numpy()
    ranks = [0, 1, 249, 250, n - 2, n - 1]
    out, nbad, _ = enqueue_chain_order(dc, ranks, None)
    assert np.array_equal(out.cpu().numpy(), host_chain_order(host, ranks)) and not nbad.cpu().numpy().any()
    # away from the zeros the bits are those of the sort as well; among the zeros -0.0 comes first
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:, 1:]), _bits(host_chain_order(host, ranks)[:, 1:]))
    nneg0 = (np.signbit(host[:, 0]) & (host[:, 0] == 0)).sum(-1)
    nneg = (host[:, 0] < 0).sum(-1)
    for c in range(2):
        for t, r in enumerate(ranks):
            if got[c, 0, t] == 0:
                assert np.signbit(got[c, 0, t]) == (r < nneg[c] + nneg0[c])


# ------------------------------------------------------------------------------------------------ placement
def test_a_series_gives_the_same_bits_wherever_it_sits():
    """Chain 0 of 1, 2 of 5, 300 of 301; column 3 of 7 under several `cols`; among different neighbours."""
    rng = np.random.default_rng(1025)
    N = 1025
    s = np.round(ar1(0.8, N, rng, mu=3.0), 2) + 0.0

    def fields(dc, c, a, cols=None):
        rd = dc.raftery_diag(*Q25, cols=cols)
        head, tri, last = device_counts(dc, 0.25, 1, BATCH, cols)
        cq = dc.chain_quantiles([0.0, 0.25, 0.5, 1.0], cols=cols)
        return [_bits(v).tolist() for v in (rd.table[c, a], rd.kthin[c, a], rd.u[c, a], head[c, a], cq[c, a])] + [
            tri[c, a].tolist(), last[c, a].tolist()]

    want = fields(device_chains(s[None, None, :]), 0, 0)
    assert np.all(np.isfinite(device_chains(s[None, None, :]).raftery_diag(*Q25).table))
    for nchains, at in ((5, 2), (301, 300)):
        cks = rng.standard_normal((nchains, 1, N)) * 10.0
        cks[at, 0] = s
        assert fields(device_chains(cks), at, 0) == want, (nchains, at)
    cks = rng.standard_normal((1, 7, N)) * np.arange(1, 8)[None, :, None]
    cks[0, 3] = s
    dc = device_chains(cks)
    for cols, where in (([3], [0]), ([5, 3, 0], [1]), ([3, 3], [0, 1]), (None, [3])):
        for a in where:
            assert fields(dc, 0, a, cols) == want, (cols, a)
    check(dc, Q25, cols=[5, 3, 0])


def test_history_with_a_row_stride_larger_than_its_rows():
    """More rows allocated than kept, an odd row stride: chain c's rows start at an odd multiple of 8 bytes for odd c.  The
    result is that of the rows uploaded alone, bit for bit."""
    rng = np.random.default_rng(7101)
    nrows, cap = 5005, 7101
    cks = np.full((3, 2, cap), np.nan)
    for c in range(3):
        cks[c, 0, :nrows] = ar1(0.6, nrows, rng, mu=3.0)
        cks[c, 1, :nrows] = np.round(ar1(0.3, nrows, rng, mu=-2.0), 1) + 0.0
    hist = device_chains(cks, nrows=nrows)
    assert hist.capacity % 2 == 1 and hist.capacity - hist.nrows == 2096
    rd, _ = check(hist, (0.025, 0.005, 0.95))
    alone_dc = device_chains(cks[:, :, :nrows])
    alone = alone_dc.raftery_diag()
    assert same(rd.table, alone.table) and same(rd.kthin, alone.kthin) and np.array_equal(_bits(rd.u), _bits(alone.u))
    probs = [0.0, 0.1, 0.5, 0.9, 1.0]
    assert np.array_equal(_bits(hist.chain_quantiles(probs)), _bits(alone_dc.chain_quantiles(probs)))


def test_256_columns_two_chains():
    rng = np.random.default_rng(256)
    N = 210
    arr = np.stack([np.stack([ar1(0.9 * j / 256.0, N, rng, mu=1.0 + j) for j in range(256)], axis=1) for _ in range(2)])
    rd, _ = check(upload(arr), Q25, batches=1)
    assert rd.table.shape == (2, 256, 4) and len(rd.varnames) == 256


# ------------------------------------------------------------------------------------------------ errors, plumbing
def test_non_finite_rows_are_refused():
    arr = mixed(500, 5, chains=3)
    for row, bad in ((3, np.nan), (499, np.inf), (250, -np.inf)):
        a = arr.copy()
        a[2, row, 1] = bad
        with pytest.raises(ValueError, match=r"non-finite.*\[1\]"):
            upload(a).raftery_diag(*Q25)
        with pytest.raises(ValueError, match=r"non-finite.*\[1\]"):
            upload(a).chain_quantiles([0.5])
    assert np.all(np.isfinite(upload(arr).raftery_diag(*Q25).table[:, :, 2]))


def test_accepts_mcmc_and_mcmclist_and_prints(sweep48):
    import fmcmc_amd as F
    host = sweep48.to_host()
    rd = F.raftery(host, *Q25)
    want = sweep48.raftery_diag(*Q25)
    assert same(rd.table, want.table)
    one = F.raftery(host[0], *Q25, cols=[1])
    assert same(one.table[0, 0], want.table[0, 1]) and len(one.varnames) == 1
    text = str(one)
    print(text)
    for piece in ("Quantile (q) = 0.25", "Accuracy (r) = +/- 0.05", "Probability (s) = 0.9", "Burn-in", "(M)", "Total", "(N)",
                  "Lower bound", "(Nmin)", "Dependence", "factor (I)", "203", "%d" % one.N[0, 0], "%.3g" % one.I[0, 0]):
        assert piece in text, piece
    assert np.array_equal(want.I, want.N / 203.0, equal_nan=True)


def test_only_reads(sweep48):
    import torch
    kept = (sweep48._samples, sweep48._logpost, sweep48._draws)
    before = [t.clone() for t in kept]
    sweep48.raftery_diag(*Q25)
    sweep48.chain_quantiles(cols=[1])
    torch.cuda.synchronize()
    for b, a in zip(before, kept):
        assert torch.equal(b.view(torch.int64), a.view(torch.int64))


def test_refuses_sharded_chains(sweep48, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="sharded"):
        sweep48.raftery_diag(*Q25)
    with pytest.raises(NotImplementedError, match="sharded"):
        sweep48.chain_quantiles()


def test_argument_errors_name_the_argument(sweep48):
    from fmcmc_amd.summary import enqueue_chain_order, enqueue_raftery
    with pytest.raises(ValueError, match="nj = 33"):
        enqueue_raftery(sweep48, 0.25, 1, 33, None)
    with pytest.raises(ValueError, match="j0 = 0"):
        enqueue_raftery(sweep48, 0.25, 0, 4, None)
    with pytest.raises(ValueError, match="q = 1.5"):
        enqueue_raftery(sweep48, 1.5, 1, 4, None)
    with pytest.raises(ValueError, match=r"ranks\[1\] = 2000"):
        enqueue_chain_order(sweep48, [0, 2000], None)
    with pytest.raises(ValueError, match="nranks = 33"):
        enqueue_chain_order(sweep48, list(range(33)), None)
    with pytest.raises(ValueError, match="at most|between"):
        sweep48.chain_quantiles(np.linspace(0, 1, 17))


# ------------------------------------------------------------------------------------------------ per-chain quantiles
PROBS = {1: [0.5], 5: [0.025, 0.25, 0.5, 0.75, 0.975],
         16: [0.0, 0.001, 0.025, 0.1, 0.25, 1 / 3, 0.4, 0.5, 0.5, 0.6, 2 / 3, 0.75, 0.9, 0.975, 0.999, 1.0]}


@pytest.mark.parametrize("N", (257, LDS_ROWS, LDS_ROWS + 1))
@pytest.mark.parametrize("nprobs", (1, 5, 16))
def test_chain_quantiles_against_a_sort(nprobs, N):
    """1, 5 and 16 probs (2, 10 and 32 targets: up to eight walks per pass), ties among them, staged and re-read series."""
    from fmcmc_amd.summary import type7_quantiles, type7_ranks
    probs = PROBS[nprobs]
    dc = upload(mixed(N, 3 * N + nprobs, chains=3))
    got = dc.chain_quantiles(probs)
    host = dc.samples.cpu().numpy()
    assert got.shape == (3, 3, nprobs)
    _, lo, hi = type7_ranks(N, probs)
    for c in range(3):
        for j in range(3):
            srt = np.sort(host[c, j])
            want = type7_quantiles(np.stack([srt[lo - 1], srt[hi - 1]], axis=-1), N, probs)
            assert np.array_equal(_bits(got[c, j]), _bits(want)), (c, j)
    sub = dc.chain_quantiles(probs, cols=[2, 0])
    assert np.array_equal(_bits(sub), _bits(got[:, [2, 0]]))


def test_chain_quantiles_of_one_chain_are_those_of_summary(sweep48):
    one = device_chains(sweep48.samples[7:8].cpu().numpy())
    for probs in PROBS.values():
        assert np.array_equal(_bits(one.chain_quantiles(probs)[0]), _bits(one.summary(quantiles=probs).quantiles))
    # and a per-chain median tells the chains apart where the pooled one cannot
    med = sweep48.chain_quantiles([0.5])
    assert med.shape == (48, 3, 1) and np.unique(med[:, 0, 0]).size > 40


# ------------------------------------------------------------------------------------------------ time
def test_headline_shape_is_faster_than_the_copy_it_replaces():
    """1024 chains x 5 parameters x 10^4 kept rows: the wall time of raftery_diag(), copy back and finish included, stays below
    the wall time of to_host() of the same rows in the same process (one warm-up each, then the best of three)."""
    import torch
    from fmcmc_amd import DeviceChains
    g = torch.Generator(device="cuda").manual_seed(1024)
    smp = torch.randn((1024, 5, 10000), dtype=torch.float64, device="cuda", generator=g)
    dc = DeviceChains(smp, None, None, np.arange(1, 10001), 1, None, 0, 1024)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    wall(dc.raftery_diag)
    wall(dc.to_host)
    t_raf, rd = min((wall(dc.raftery_diag) for _ in range(3)), key=lambda v: v[0])
    t_host, _ = min((wall(dc.to_host) for _ in range(3)), key=lambda v: v[0])
    print("raftery_diag() wall %.1f ms, to_host() wall %.1f ms" % (1e3 * t_raf, 1e3 * t_host))
    assert rd.table.shape == (1024, 5, 4) and (rd.kthin == 1).mean() > 0.99       # iid rows: G2 ~ chi2(2) against 2 log(9998)
    assert np.median(np.abs(rd.I - 1.0)) < 0.1                                      # ... and N close to nmin
    assert t_raf < t_host
