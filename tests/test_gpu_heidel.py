"""GPU tests of the device-side Heidelberger-Welch diagnostic (fmcmc_amd/summary.py: heidel -> csrc/summary.hip:
summary_cvm_kernel and stages 1-2 on every window).

References are computed on the host copy of the same rows in longdouble: `host_series` of tests/test_gpu_summary.py for the
windows' mean / spec0 / order, a longdouble cumsum of the centred tail for Q = sum_t B_t^2.  Tolerances are computed in the
tests from the references alone:
 * Q: 16 x the worst relative distance, over the same series and candidates, between the longdouble value and two float64
   host evaluations (np.cumsum forward; the bridge summed from the last row backwards, on a mean summed backwards);
 * spec0 (S0 of the stationarity test, spec0 of the chosen tail behind halfwidth): `spec0_tolerance`, the same rule;
 * I = Q / (n^2 S0): the sum of the two; pvalue: within the span of pcramer over I (1 +- that), plus 4 x 2^-53 for the
   rounding of the series itself; mean: within n 2^-53 mean(|y|), which holds for any summation order;
 * stest / start / htest: equal, except for series whose reference is within 1e-9 of a threshold (p-value of a candidate
   examined, |halfwidth / mean| against eps) or has an AIC gap below 1e-6 in a window used; at most 1 % of the series may be
   left out for that, asserted from the reference alone.
Measured distances (MI355X, printed with -s): DESIGN.md section 5.10.
"""
import numpy as np
import pytest

from test_gpu_summary import LD, U, _bits, ar1, host_series, spec0_tolerance, upload
from test_gpu_summary_edges import device_chains
from test_heidel_host import CASES, synthetic_set, windows_of

pytestmark = pytest.mark.gpu
CT = 4608               # csrc/summary.hip: rows of a tail the scan stages in LDS at once (512 threads x 9 rows)
LDS_ROWS = 19456        # rows of a series stages 1-2 stage in LDS at once


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------ reference
def bridge_q(y):
    """Q of one tail: longdouble, and the two float64 host evaluations."""
    n = y.size
    yl = y.astype(LD)
    B = np.cumsum(yl - yl.sum() / LD(n))
    fwd = np.cumsum(y - y.mean())
    back = np.cumsum((y - y[::-1].sum() / n)[::-1])[:-1]          # minus the bridge, from its last row to its first
    return (B * B).sum(), float(np.sum(fwd * fwd)), float(np.sum(back * back))


def reference(host, iters, cols, label, eps=0.1, pvalue=0.05):
    """host [C][k][N] -> the longdouble reference of heidel(cols=cols) and the tolerances, as a dict of [C][p] arrays (Q, I:
    [C][p][ncand]); `skip` marks the series whose decisions the reference itself cannot tell."""
    from fmcmc_amd.summary import pcramer          # (bit for bit convergence._pcramer: tests/test_heidel_host.py)
    labels, rows, half = windows_of(iters)         # restated from heidel_diag, not taken from the code under test
    first_label = np.asarray(iters, dtype=np.float64)[rows]
    C_, _, N = host.shape
    p, ncand = len(cols), rows.size
    n = (N - rows).astype(np.float64)
    Q = np.empty((C_, p, ncand), dtype=LD)
    worst_q = 0.0
    for c in range(C_):
        for a, col in enumerate(cols):
            for s, lo in enumerate(rows):
                Q[c, a, s], qf, qb = bridge_q(host[c, col, lo:])
                if Q[c, a, s] > 0:
                    worst_q = max(worst_q, float(abs(LD(qf) - Q[c, a, s]) / Q[c, a, s]), float(abs(LD(qb) - Q[c, a, s]) / Q[c, a, s]))
    tol_q = 16 * worst_q
    tol_s0, half_refs = spec0_tolerance([host[c, col, half:] for c in range(C_) for col in cols], label + ", S0 window")
    S0 = np.array([r["spec0"] for r in half_refs], dtype=LD).reshape(C_, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        I = (Q / (LD(1) * n * n) / S0[:, :, None]).astype(np.float64)
    pc = pcramer(I)
    ok = np.isfinite(I) & (pc < 1 - pvalue)
    converged = ok.any(axis=2)
    pick = np.where(converged, ok.argmax(axis=2), ncand - 1)
    tol_tail, tail_refs = spec0_tolerance([host[c, col, rows[pick[c, a]]:] for c in range(C_) for a, col in enumerate(cols)],
                                          label + ", chosen tails")
    ref = dict(labels=labels, first_label=first_label, rows=rows, n=n, Q=Q, I=I, tol_q=tol_q, tol_i=tol_q + tol_s0, tol_tail=tol_tail, S0=S0,
               converged=converged, pick=pick)
    for f in ("start", "pvalue", "htest", "mean", "halfwidth", "mean_bound"):
        ref[f] = np.full((C_, p), np.nan)
    ref["skip"] = np.zeros((C_, p), dtype=bool)
    for c in range(C_):
        for a, col in enumerate(cols):
            s, tr, hr = pick[c, a], tail_refs[c * p + a], half_refs[c * p + a]
            y = host[c, col, rows[s]:]
            hw = np.float64(1.96 * np.sqrt(tr["spec0"] / LD(y.size)))
            ratio = abs(hw / np.float64(tr["mean"])) if tr["mean"] != 0 else np.inf
            margins = [abs(pc[c, a, u] - (1 - pvalue)) for u in range(s + 1) if np.isfinite(I[c, a, u])] + [abs(ratio - eps)]
            ref["skip"][c, a] = min(margins) < 1e-9 or min(tr["gap"], hr["gap"]) < 1e-6
            ref["mean_bound"][c, a] = y.size * U * np.abs(y).mean()
            if np.isfinite(I[c, a, s]):
                ref["pvalue"][c, a] = 1 - pc[c, a, s]
            if converged[c, a] and np.isfinite(hw):
                ref["start"][c, a], ref["htest"][c, a] = first_label[s], float(ratio <= eps)
                ref["mean"][c, a], ref["halfwidth"][c, a] = np.float64(tr["mean"]), hw
    print("[%s] %d series x %d candidates: worst float64-vs-longdouble relative distance of Q %.3g -> tolerance %.3g; %d of the "
          "series left out of the decisions" % (label, C_ * p, ncand, worst_q, tol_q, int(ref["skip"].sum())))
    assert ref["skip"].sum() <= 0.01 * C_ * p, ref["skip"].sum()
    return ref


def device_q(dc, cols):
    """Q [C][p][ncand] as fmcmc_heidel_dev left it."""
    from fmcmc_amd.summary import enqueue_heidel
    _, rows, half = windows_of(dc.iters)
    out, _, cols_ = enqueue_heidel(dc, half, rows, cols)
    Cn, p, ncand = int(dc._samples.shape[0]), int(cols_.size), rows.size
    return out.cpu().numpy()[(1 + ncand) * Cn * p * 4:].reshape(ncand, Cn, p).transpose(1, 2, 0)


def check(dc, cols, label, eps=0.1, pvalue=0.05):
    from fmcmc_amd.summary import pcramer
    host = dc.samples.cpu().numpy()
    cols_ = list(range(host.shape[1])) if cols is None else list(cols)
    ref = reference(host, dc.iters, cols_, label, eps, pvalue)
    hd = dc.heidel(eps=eps, pvalue=pvalue, cols=cols)
    C_, p, ncand = ref["I"].shape
    assert hd.table.shape == (C_, p, 6) and hd.cvm.shape == (C_, p, ncand) and np.array_equal(hd.candidates, ref["labels"])
    # Q and the statistic of every candidate
    Qd = device_q(dc, cols)
    pos = ref["Q"] > 0
    dq = np.abs(Qd.astype(LD) - ref["Q"])[pos] / ref["Q"][pos]
    worst_q = float(dq.max()) if dq.size else 0.0
    assert np.all(Qd[~pos] == 0.0)
    fin = np.isfinite(ref["I"])
    assert np.all(~np.isfinite(hd.cvm[~fin]))
    di = np.abs(hd.cvm[fin] - ref["I"][fin]) / ref["I"][fin]
    print("device vs longdouble: worst relative distance of Q %.3g (tolerance %.3g), of I %.3g (tolerance %.3g)"
          % (worst_q, ref["tol_q"], float(di.max()) if di.size else 0.0, ref["tol_i"]))
    assert worst_q <= ref["tol_q"] and np.all(di <= ref["tol_i"])
    # decisions
    keep = ~ref["skip"]
    assert np.array_equal(hd.stest[keep], ref["converged"][keep].astype(np.float64))
    assert np.array_equal(hd.start[keep], ref["start"][keep], equal_nan=True)
    assert np.array_equal(hd.htest[keep], ref["htest"][keep], equal_nan=True)
    # pvalue, mean, halfwidth of the series whose start is the reference's
    same = keep & (np.isnan(hd.start) == np.isnan(ref["start"])) & ((hd.start == ref["start"]) | np.isnan(ref["start"]))
    assert np.array_equal(np.isnan(hd.pvalue[same]), np.isnan(ref["pvalue"][same]))
    I_s = np.take_along_axis(ref["I"], ref["pick"][:, :, None], axis=2)[:, :, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        ends = np.stack([1 - pcramer(I_s * (1 - ref["tol_i"])), 1 - pcramer(I_s * (1 + ref["tol_i"]))])
    m = same & np.isfinite(ref["pvalue"])
    assert np.all(hd.pvalue[m] >= ends.min(0)[m] - 4 * U) and np.all(hd.pvalue[m] <= ends.max(0)[m] + 4 * U)
    m = same & np.isfinite(ref["start"])
    assert np.all(np.abs(hd.mean[m] - ref["mean"][m]) <= ref["mean_bound"][m])
    assert np.all(np.abs(hd.halfwidth[m] - ref["halfwidth"][m]) <= ref["tol_tail"] * ref["halfwidth"][m])
    return hd, ref


# ------------------------------------------------------------------------------------------------ inputs
@pytest.fixture(scope="module")
def sweep48(readme_data):
    from fmcmc_amd import MCMC, gaussian_linreg, kernel_normal
    X, y = readme_data
    init = np.array([0.0, 0.0, np.std(y, ddof=1)])[None, :] + 0.1 * np.random.default_rng(48).standard_normal((48, 3))
    init[:, 2] = np.abs(init[:, 2])
    return MCMC(init, gaussian_linreg(X, y), 2000, nchains=48, seed=11, kernel=kernel_normal(scale=0.15), _return_device=True)


def synthetic_chains(case):
    """The synthetic set of tests/test_heidel_host.py, its ten columns as they are: one chain [1][N][10]."""
    data, iters = synthetic_set(*case)
    return data[None], int(iters[0]), case[1]


# ------------------------------------------------------------------------------------------------ tests
def test_real_sweep_48_chains(sweep48):
    assert tuple(sweep48.samples.shape) == (48, 3, 2000)
    hd, ref = check(sweep48, None, "48 chains kernel_normal(scale = .15)")
    # table[c] lines up with the single-chain function
    from fmcmc_amd.convergence import heidel_diag
    host = sweep48.samples.cpu().numpy()
    for c in (0, 47):
        want = heidel_diag(host[c].T, sweep48.iters)
        keep = ~ref["skip"][c]
        assert np.array_equal(hd.table[c][keep][:, [0, 1, 3]], want[keep][:, [0, 1, 3]], equal_nan=True)
    print(str(hd).split("[[2]]")[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-thin%d-seed%d" % (c[0], c[1], c[3]))
def test_synthetic_set_of_the_host_test(case):
    """Level shifts, drifts, a mean near zero, a constant column; thin = 3 with first label 31 among them."""
    arr, start, thin = synthetic_chains(case)
    dc = upload(arr, thin=thin, start=start)
    hd, ref = check(dc, None, "synthetic %s" % (case,))
    t = hd.table[0]
    assert np.all(t[:4, 0] == 1) and np.all(t[:3, 1] == start) and np.all(t[4:6, 1] > start)   # (as heidel_diag has them)
    assert t[8, 0] == 1 and t[8, 3] == 0
    assert t[9, 0] == 0 and np.all(np.isnan(t[9, 1:])) and np.all(np.isnan(hd.cvm[0, 9]))
    # table[0] lines up with the single-chain function; off the thinning grid (N = 2003, 607) `start` is the first row kept
    from fmcmc_amd.convergence import heidel_diag
    data, iters = synthetic_set(*case)
    want, keep = heidel_diag(data, iters), ~ref["skip"][0]
    assert np.array_equal(t[keep][:, [0, 1, 3]], want[keep][:, [0, 1, 3]], equal_nan=True)
    assert np.all(np.isin(t[np.isfinite(t[:, 1]), 1], iters))


def test_shortest_series():
    """N = 4 at thin = 1: candidates at rows 0, 1, 1, the S0 window is three rows.  N = 3 leaves it two rows: refused."""
    rng = np.random.default_rng(4)
    arr = np.stack([np.stack([ar1(0.5, 4, rng, mu=3.0), ar1(0.0, 4, rng, mu=-2.0)], axis=1) for _ in range(3)])
    hd, ref = check(upload(arr), None, "N = 4")
    assert hd.cvm.shape == (3, 2, 3) and np.array_equal(_bits(hd.cvm[:, :, 1]), _bits(hd.cvm[:, :, 2]))
    with pytest.raises(ValueError, match="needs 3"):
        upload(arr[:, :3]).heidel()


@pytest.mark.parametrize("N", (CT - 1, CT, CT + 1, LDS_ROWS - 1, LDS_ROWS, LDS_ROWS + 1))
def test_tails_at_the_tile_edges(N):
    """The longest tail has N rows: one row less than a tile, a tile, one row more (the scan's tile of 4608 rows and the
    19456 rows of stages 1-2); the largest steps of the bridge sit at the tile boundary."""
    rng = np.random.default_rng(N)
    arr = np.stack([ar1(0.5, N, rng, mu=3.0), ar1(0.9, N, rng, mu=-2.0)], axis=1)[None]
    edge = CT if N < 2 * CT else LDS_ROWS
    arr[0, min(edge, N) - 1] += 25.0
    arr[0, min(edge, N - 1)] -= 25.0
    check(upload(arr), None, "N = %d" % N)


def test_every_window_multi_tile():
    """N = 40000: the shortest tail has 24000 rows, beyond the 19456 rows of stages 1-2 and five tiles of the scan."""
    rng = np.random.default_rng(40000)
    arr = np.stack([ar1(0.7, 40000, rng, mu=3.0), ar1(0.2, 40000, rng, mu=0.5)], axis=1)[None]
    check(upload(arr), None, "N = 40000")


def test_carry_over_many_tiles():
    """N = 200003: 44 tiles, the running bridge is carried from tile to tile; two series."""
    rng = np.random.default_rng(200003)
    arr = np.stack([ar1(0.5, 200003, rng, mu=3.0), ar1(0.95, 200003, rng, mu=-1.0)], axis=1)[None]
    check(upload(arr), None, "N = 200003")


def test_history_with_odd_capacity_and_odd_first_row():
    """More rows allocated than kept, an odd row stride: chain c's rows start at an odd multiple of 8 bytes for odd c, and
    the candidate tails start at odd and even rows.  The result is that of the rows uploaded alone, bit for bit."""
    rng = np.random.default_rng(7101)
    nrows, cap = 5005, 7101
    cks = np.full((3, 2, cap), np.nan)
    for c in range(3):
        cks[c, 0, :nrows] = ar1(0.6, nrows, rng, mu=3.0)
        cks[c, 1, :nrows] = ar1(0.3, nrows, rng, mu=-2.0)
        cks[c, 1, :700] += 1.0
    hist = device_chains(cks, nrows=nrows)
    assert hist.capacity % 2 == 1 and hist.capacity - hist.nrows == 2096
    hd, ref = check(hist, None, "history")
    assert list(ref["rows"]) == [0, 501, 1001, 1502, 2002]             # tails from odd and from even rows
    alone = device_chains(cks[:, :, :nrows]).heidel()
    assert np.array_equal(_bits(hd.table), _bits(alone.table)) and np.array_equal(_bits(hd.cvm), _bits(alone.cvm))


def test_cols_subset_in_any_order(sweep48):
    full = sweep48.heidel()
    sub = sweep48.heidel(cols=[2, 0])
    assert sub.varnames == [full.varnames[2], full.varnames[0]]
    assert np.array_equal(_bits(sub.table), _bits(full.table[:, [2, 0]]))
    assert np.array_equal(_bits(sub.cvm), _bits(full.cvm[:, [2, 0]]))
    check(sweep48, [2, 0], "48 chains, cols = [2, 0]")


def test_256_columns_two_chains():
    rng = np.random.default_rng(256)
    N = 130
    arr = np.stack([np.stack([ar1(0.9 * j / 256.0, N, rng, mu=1.0 + j) for j in range(256)], axis=1) for _ in range(2)])
    arr[:, :20, 100:120] += 1.5
    hd, _ = check(upload(arr), None, "256 columns")
    assert hd.table.shape == (2, 256, 6)


@pytest.mark.parametrize("N", (1025, 2 * CT + 1))
def test_a_series_gives_the_same_bits_wherever_it_sits(N):
    """Chain 0 of 1, 2 of 5, 300 of 301; column 0 of 1, 3 of 7 under several `cols`; among different neighbours."""
    rng = np.random.default_rng(N)
    s = ar1(0.6, N, rng, mu=3.0)
    s[:N // 7] += 1.0
    fields = lambda hd, c, a: [_bits(v).tolist() for v in (hd.cvm[c, a], hd.pvalue[c, a], hd.halfwidth[c, a], hd.table[c, a])]
    want = fields(device_chains(s[None, None, :]).heidel(), 0, 0)
    assert np.all(np.isfinite(device_chains(s[None, None, :]).heidel().cvm))
    for nchains, at in ((5, 2), (301, 300)):
        cks = rng.standard_normal((nchains, 1, N)) * 10.0
        cks[at, 0] = s
        assert fields(device_chains(cks).heidel(), at, 0) == want, (nchains, at)
    cks = rng.standard_normal((1, 7, N)) * np.arange(1, 8)[None, :, None]
    cks[0, 3] = s
    dc = device_chains(cks)
    for cols, where in (([3], [0]), ([5, 3, 0], [1]), ([3, 3], [0, 1]), (None, [3])):
        hd = dc.heidel(cols=cols)
        for a in where:
            assert fields(hd, 0, a) == want, (cols, a)


def test_mean_has_the_bits_of_summary(sweep48):
    hd, sm = sweep48.heidel(), sweep48.summary(quantiles=())
    first = hd.start == sweep48.iters[0]
    print("%d of %d series start at the first candidate" % (first.sum(), first.size))
    assert first.any()
    assert np.array_equal(_bits(hd.mean[first]), _bits(sm.per_chain.mean[first]))
    assert np.array_equal(_bits(hd.halfwidth[first]), _bits(1.96 * np.sqrt(sm.per_chain.spec0[first] / 2000.0)))


def test_heidel_only_reads(sweep48):
    import torch
    kept = (sweep48._samples, sweep48._logpost, sweep48._draws)
    before = [t.clone() for t in kept]
    sweep48.heidel()
    sweep48.heidel(cols=[1])
    torch.cuda.synchronize()
    for b, a in zip(before, kept):
        assert torch.equal(b.view(torch.int64), a.view(torch.int64))


def test_non_finite_rows_are_refused():
    rng = np.random.default_rng(5)
    arr = np.stack([np.stack([ar1(0.6, 500, rng, mu=1.0), ar1(0.2, 500, rng)], axis=1) for _ in range(3)])
    for row, bad in ((3, np.nan), (499, np.inf)):
        a = arr.copy()
        a[2, row, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            upload(a).heidel()
    assert np.all(np.isfinite(upload(arr).heidel().cvm))


def test_refuses_sharded_chains(sweep48, monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="sharded"):
        sweep48.heidel()
