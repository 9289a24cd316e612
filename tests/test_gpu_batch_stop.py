"""MCMC_batch(stop_each = convergence_gelman(...)): every dataset stops on its own (fmcmc_mcmc_run_batch_sel_dev's dataset mask,
fmcmc_gelman_groups_dev's grouped check, the loop in mcmc._batch_stop_each) on the GPU.

Two references, both built here.  The oracle's: per dataset, a loop of O.run(..., chain_base = d Cm, state = ...) per bulk with
the restart from the last kept row and O.gelman_check, as O.mcmc_with_conv_checker runs it.  The device's: per dataset, a loop of
engine.sweep(DeviceModel_d, chain_base = d Cm, into = ...) and convergence_gelman.check_device -- the code MCMC(conv_checker =
...) runs.  A chain does not depend on the verdicts, so both references run every bulk of every dataset once and a threshold
only cuts them; `StopRef.stops` gives the stop bulks of a threshold and asserts what makes a case worth running: at least two
distinct stop bulks, a dataset that runs every bulk, and no statistic within 1e-6 (relative) of the threshold.

Against the device loop everything is bitwise (the same operations in the same order); against the oracle the rows are bitwise,
the stop bulks equal, and the statistic within rtol 1e-8 (tests/test_gpu_api.py: test_mcmc_autostop_matches_the_oracle)."""
import copy

import numpy as np
import pytest

from test_gpu_batch import LINREG, Case, bad_dataset_case, linreg_case, linreg_data
from test_gpu_parity import _bits_equal

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("theta0", "f0", "abs_iter", "Sigma", "mean_prev", "have_mean", "nerrors")


@pytest.fixture(scope="module")
def E():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fmcmc_amd import engine
    return engine


def stop_starts(base, D, Cm):
    """[D Cm][k]: dataset d's chains start at base + 0.5 N(0, 1) (default_rng(80 + d)), the last column (sigma) made positive"""
    init = np.concatenate([np.asarray(base)[None, :] + 0.5 * np.random.default_rng(80 + d).standard_normal((Cm, len(base)))
                           for d in range(D)])
    init[:, -1] = np.abs(init[:, -1]) + 0.5
    return init


class StopRef:
    """The oracle's run of every bulk of every dataset: rows, labels, the statistic after each bulk and the state the kernel
    carries behind each bulk."""

    def __init__(self, O, Xs, ys, kind, init, Cm, nsteps, freq, burnin=0, thin=1, seed=77, model_kw=None, **kw):
        from fmcmc_amd import bulk_plan
        self.O, self.Xs, self.ys, self.Cm, self.D = O, Xs, np.asarray(ys), Cm, len(ys)
        self.nsteps, self.freq, self.burnin, self.thin, self.seed = nsteps, freq, burnin, thin, seed
        self.init = np.ascontiguousarray(init, dtype=np.float64)
        self.k = self.init.shape[1]
        self.ok = ok = O.Kernel(kind, self.k, **kw)
        self.free = np.where(ok.fixed == 0)[0]
        self.bulks = bulk_plan(nsteps, burnin, freq)
        self.model_kw = dict(model_kw or {})
        self.rows_after, self.vals, self.samples, self.draws, self.logpost, self.states = [], [], [], [], [], []
        for d in range(self.D):
            om = O.Model(LINREG, Xs[d], ys[d], **self.model_kw)
            st = O.ChainState(self.init[d * Cm:(d + 1) * Cm], ok.kf)
            parts, dparts, lparts, iters, vals, rows, states = [], [], [], None, [], [], []
            for bi, nb in enumerate(self.bulks):
                r = O.run(om, ok, nsteps=nb, burnin=burnin if bi == 0 else 0, thin=thin, seed=seed, chain_base=d * Cm, state=st)
                assert (r.status == 0).all()
                states.append({f: getattr(st, f).copy() for f in STATE_FIELDS})
                parts.append(r.samples_cks); dparts.append(r.draws_cks); lparts.append(r.logpost)
                if r.samples.shape[1]:
                    st.theta0[:] = r.samples[:, -1, :]          # the next bulk starts from the last KEPT row
                    iters = r.iters.copy() if iters is None else np.concatenate([iters, r.iters - r.iters[0] + iters[-1] + thin])
                val = float("nan")
                if iters is not None:
                    ans = np.concatenate(parts, axis=2).transpose(0, 2, 1)       # [Cm][S][k]
                    _conv, val = O.gelman_check(ans[:, :, self.free], iters, 0.0)
                vals.append(val)
                rows.append(0 if iters is None else int(iters.size))
            self.iters = iters                                                      # (the same labels for every dataset)
            self.samples.append(np.concatenate(parts, axis=2)); self.draws.append(np.concatenate(dparts, axis=2))
            self.logpost.append(np.concatenate(lparts, axis=1))
            self.vals.append(vals); self.rows_after.append(rows); self.states.append(states)
        self.vals = np.array(self.vals)                                             # [D][bulks]
        self.rows_after = np.array(self.rows_after[0])                              # [bulks]

    def stops(self, threshold):
        """stop[d]: the number of bulks dataset d runs (len(bulks) when it never passes), and did it pass; with the
        conditions on the inputs asserted on this reference"""
        nb = len(self.bulks)
        below = self.vals < threshold
        stop = np.array([int(np.argmax(b)) + 1 if b.any() else nb for b in below])
        conv = below.any(axis=1)
        seen = [self.vals[d, :stop[d]] for d in range(self.D)]
        assert len(set(stop.tolist())) >= 2, "the datasets stop at one bulk: %s" % stop
        assert (stop == nb).any(), "no dataset runs every bulk: %s" % stop
        for v in seen:
            v = np.asarray(v, dtype=np.float64)
            v = v[np.isfinite(v)]
            assert (np.abs(v - threshold) > 1e-6 * threshold).all(), "a statistic sits on the threshold"
        return stop, conv

    def threshold(self):
        """a threshold from the oracle's own sequences: of the midpoints of two neighbouring statistics under which `stops`
        holds, the one that spreads the datasets over the most stop bulks (the smallest of those)"""
        v = np.unique(self.vals[np.isfinite(self.vals)])
        best, spread = None, 0
        for t in 0.5 * (v[:-1] + v[1:]):
            try:
                stop, _conv = self.stops(t)
            except AssertionError:
                continue
            if len(set(stop.tolist())) > spread:
                best, spread = float(t), len(set(stop.tolist()))
        assert best is not None, "no threshold separates the datasets of this case"
        return best

    def fkernel(self, F):
        O, ok = self.O, self.ok
        if ok.kind == O.K_NORMAL:
            return F.kernel_normal(scale=float(ok.scale[0]))
        if ok.kind == O.K_RAM:
            return F.kernel_ram(warmup=ok.warmup)
        assert ok.kind == O.K_ADAPT and not ok.fixed.any()
        return F.kernel_adapt(warmup=ok.warmup)

    def spec(self, E):
        return Case.spec(self, E)

    def batch(self, F):
        return F.model_batch(F.gaussian_linreg(self.Xs[d], self.ys[d], **self.model_kw) for d in range(self.D))

    def run(self, F, threshold, **kw):
        kern = self.fkernel(F)
        chk = F.convergence_gelman(self.freq, threshold=threshold)
        ans = F.MCMC_batch(self.init.reshape(self.D, self.Cm, self.k), self.batch(F), self.nsteps, nchains=self.Cm, burnin=self.burnin,
                           thin=self.thin, seed=self.seed, kernel=kern, stop_each=chk, **kw)
        assert chk.history == [] and chk.last is None           # the checker object is only read
        return ans, kern

    def assert_result(self, ans, threshold):
        """an McmcBatch of a stop_each call against this reference: stop bulks, statistics, rows, labels, NaN beyond"""
        stop, conv = self.stops(threshold)
        nb, Cm = len(self.bulks), self.Cm
        steps = np.array([sum(self.bulks[:s]) for s in stop])
        nrows = self.rows_after[stop - 1]
        print("stop bulks", stop.tolist(), "statistics at the stop", [float(self.vals[d, stop[d] - 1]) for d in range(self.D)])
        assert ans.steps.tolist() == steps.tolist() and ans.nrows.tolist() == nrows.tolist()
        assert ans.converged.tolist() == conv.tolist()
        assert [t for t, _ in ans.rhat_history] == [sum(self.bulks[:b + 1]) for b in range(stop.max())]
        for b, (_total, vals) in enumerate(ans.rhat_history):
            for d in range(self.D):
                if b < stop[d] and np.isfinite(self.vals[d, b]):
                    np.testing.assert_allclose(vals[d], self.vals[d, b], rtol=1e-8)
                else:
                    assert np.isnan(vals[d])
        hs, hd, hl = (t.cpu().numpy() for t in (ans.history._samples, ans.history._draws, ans.history._logpost))
        for d in range(self.D):
            sl, nr = slice(d * Cm, (d + 1) * Cm), int(nrows[d])
            assert _bits_equal(hs[sl, :, :nr], self.samples[d][:, :, :nr]), "samples of dataset %d" % d
            assert _bits_equal(hd[sl, :, :nr], self.draws[d][:, :, :nr]), "draws of dataset %d" % d
            assert _bits_equal(hl[sl, :nr], self.logpost[d][:, :nr]), "logpost of dataset %d" % d
            assert np.isnan(hs[sl, :, nr:]).all() and np.isnan(hd[sl, :, nr:]).all() and np.isnan(hl[sl, nr:]).all()
            dc = ans[d]
            assert dc.nrows == nr and dc.iters.tolist() == self.iters[:nr].tolist() and dc.chain_base == d * Cm
        assert ans.chains.nrows == nrows.min() and np.isfinite(ans.chains.samples.cpu().numpy()).all()
        return stop, conv


def device_loop(E, ref, threshold):
    """today's code, dataset by dataset: engine.sweep(into = ...) per bulk, the restart from the last kept row and
    convergence_gelman.check_device -> per dataset (stop bulk, the statistics, samples / draws / logpost [Cm][..][rows])"""
    import torch
    import fmcmc_amd as F
    out = []
    gk = ref.spec(E)
    for d in range(ref.D):
        Cm = ref.Cm
        model = E.DeviceModel(LINREG, ref.Xs[d], ref.ys[d], **ref.model_kw)
        st = E.ChainState(ref.init[d * Cm:(d + 1) * Cm], ref.ok.kf)
        cap = int(ref.rows_after[-1])
        # (the checker sees the dataset as a run of its own -- chain_base 0 --, so it centres on the dataset's first chain)
        hist = F.DeviceChains.allocate(Cm, ref.k, cap, ref.thin, None, 0, Cm, st.device)
        chk = F.convergence_gelman(ref.freq, threshold=threshold)
        vals, stop = [], None
        for bi, nb in enumerate(ref.bulks):
            if bi > 0 and hist.nrows > 0:
                st.theta0.copy_(hist._samples[:, :, hist.nrows - 1])
            r = E.sweep(model, gk, st, nb, burnin=ref.burnin if bi == 0 else 0, thin=ref.thin, seed=ref.seed, chain_base=d * Cm,
                        want_bits=False, into=(hist._samples, hist._logpost, hist._draws), row0=hist.nrows)
            hist.extend(r.iters)
            chk.last = None
            done = chk.check_device(hist, ref.free)
            vals.append(float("nan") if chk.last is None else chk.last)
            if done:
                stop = bi + 1
                break
        torch.cuda.synchronize()
        out.append((stop or len(ref.bulks), vals, hist.samples.cpu().numpy(), hist.draws.cpu().numpy(), hist.logpost.cpu().numpy()))
    return out


def assert_equals_device_loop(E, ref, ans, threshold):
    loop = device_loop(E, ref, threshold)
    Cm = ref.Cm
    for d, (stop, vals, smp, drw, lp) in enumerate(loop):
        nr = int(ans.nrows[d])
        assert ans.steps[d] == sum(ref.bulks[:stop]) and smp.shape[2] == nr, "stop bulk of dataset %d" % d
        got = [float(v[d]) for _t, v in ans.rhat_history[:stop]]
        assert _bits_equal(got, vals), "statistics of dataset %d: %s against %s" % (d, got, vals)
        dc = ans[d]
        assert _bits_equal(dc.samples.cpu().numpy(), smp) and _bits_equal(dc.draws.cpu().numpy(), drw)
        assert _bits_equal(dc.logpost.cpu().numpy(), lp)


@pytest.fixture(scope="module")
def normal_refs(O):
    """the case of the issue for 5, 3 and 2 chains per dataset: 6 datasets (linreg_data(6, 130, 3, 5)), kernel_normal(scale =
    0.1), seed 77, 600 steps in bulks of 100, threshold 1.2"""
    Xs, ys, base = linreg_data(6, 130, 3, 5)
    return {Cm: StopRef(O, Xs, ys, O.K_NORMAL, stop_starts(base, 6, Cm), Cm, 600, 100, scale=0.1) for Cm in (5, 3, 2)}


@pytest.mark.parametrize("Cm", [5, 3, 2])
def test_every_dataset_stops_where_the_oracle_and_the_device_loop_stop_it(E, normal_refs, Cm):
    import fmcmc_amd as F
    from fmcmc_amd import _abi as abi
    ref = normal_refs[Cm]
    ans, _kern = ref.run(F, 1.2)
    assert abi.last_kernel() == "batch-lds"
    ref.assert_result(ans, 1.2)
    assert_equals_device_loop(E, ref, ans, 1.2)
    # the per-dataset diagnostics of the ragged result, one reduction for all: each dataset on its own rows
    diags = ans.gelman_diag()
    for d in range(ref.D):
        h = F.gelman_diag(ans[d])
        assert _bits_equal(diags[d].psrf, h.psrf) and diags[d].mpsrf == h.mpsrf
        if ans.converged[d]:
            assert diags[d].mpsrf == ans.rhat_history[int(ans.steps[d]) // 100 - 1][1][d] < 1.2
    assert ans.ragged
    with pytest.raises(ValueError, match="ragged"):
        F.MCMC_batch(ans, ref.batch(F), 100, nchains=Cm, seed=77, kernel=_kern)


def test_the_masked_sweep_with_the_data_streamed(E, O, normal_refs):
    """the same case through engine.sweep_batch(stream_data = True, active = ...), the mask from the oracle's stop bulks:
    the rows of the datasets that run are the oracle's, the others keep their NaN, status 0 and accept count 0"""
    import torch
    from fmcmc_amd import _abi as abi
    ref = normal_refs[3]
    stop, _conv = ref.stops(1.2)
    D, Cm, k = ref.D, ref.Cm, ref.k
    batch = E.DeviceModelBatch(LINREG, ref.Xs, ref.ys)
    gk, gst = ref.spec(E), E.ChainState(ref.init, ref.ok.kf)
    cap = int(ref.rows_after[-1])
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    hs, hl, hd = nan(D * Cm, k, cap), nan(D * Cm, cap), nan(D * Cm, k, cap)
    rows = 0
    for bi, nb in enumerate(ref.bulks):
        act = stop > bi
        if not act.any():
            break
        mask = torch.as_tensor(act.astype(np.int32)).cuda()
        chains = torch.as_tensor(np.repeat(act, Cm)).cuda()
        if bi > 0:
            gst.theta0.copy_(torch.where(chains[:, None], hs[:, :, rows - 1], gst.theta0))
        r = E.sweep_batch(batch, gk, gst, nb, seed=ref.seed, into=(hs, hl, hd), row0=rows, stream_data=True, active=mask)
        torch.cuda.synchronize()
        assert abi.last_kernel() == "batch-stream"
        assert (r.status[~chains] == 0).all() and (r.accept_count[~chains] == 0).all() and (r.accept_count[chains] > 0).all()
        assert (r.accept_bits[~chains] == 0).all()
        rows += nb
    for d in range(D):
        sl, nr = slice(d * Cm, (d + 1) * Cm), int(ref.rows_after[stop[d] - 1])
        assert _bits_equal(hs[sl, :, :nr].cpu().numpy(), ref.samples[d][:, :, :nr])
        assert _bits_equal(hd[sl, :, :nr].cpu().numpy(), ref.draws[d][:, :, :nr])
        assert _bits_equal(hl[sl, :nr].cpu().numpy(), ref.logpost[d][:, :nr])
        assert torch.isnan(hs[sl, :, nr:]).all() and torch.isnan(hl[sl, nr:]).all() and torch.isnan(hd[sl, :, nr:]).all()


@pytest.mark.parametrize("name,kw", [("ram", dict()), ("adapt", dict(warmup=50))])
def test_frozen_chains_keep_the_state_of_their_stop_bulk(E, O, name, kw):
    """kernel_ram and kernel_adapt carry Sigma / abs_iter / mean_prev / have_mean per chain: after the call a frozen dataset's
    chains hold the oracle's state behind their stop bulk, whatever the other datasets ran afterwards"""
    import fmcmc_amd as F
    kind = {"ram": O.K_RAM, "adapt": O.K_ADAPT}[name]
    Xs, ys, base = linreg_data(5, 130, 3, 5)
    ref = StopRef(O, Xs, ys, kind, stop_starts(base, 5, 3), 3, 800, 100, **kw)
    t = ref.threshold()
    ans, kern = ref.run(F, t)
    stop, _conv = ref.assert_result(ans, t)
    assert_equals_device_loop(E, ref, ans, t)
    gst = kern._state
    cpu = lambda x: x.cpu().numpy()
    for d in range(ref.D):
        sl, want = slice(d * ref.Cm, (d + 1) * ref.Cm), ref.states[d][stop[d] - 1]
        assert _bits_equal(cpu(gst.theta0[sl]), want["theta0"]) and _bits_equal(cpu(gst.f0[sl]), want["f0"]), "dataset %d" % d
        assert _bits_equal(cpu(gst.Sigma[sl]), want["Sigma"]) and np.array_equal(cpu(gst.abs_iter[sl]), want["abs_iter"])
        assert np.array_equal(cpu(gst.nerrors[sl]), want["nerrors"])
        if kind == O.K_ADAPT:
            assert np.array_equal(cpu(gst.have_mean[sl]), want["have_mean"])
            hm = want["have_mean"].astype(bool)
            assert _bits_equal(cpu(gst.mean_prev[sl])[hm], want["mean_prev"][hm])


def test_burnin_and_thinning(E, O):
    """burnin = 30, thin = 3, bulks of 100 (33 rows each; the first bulk is 130 steps): the window starts at coda's row, an
    active chain restarts from its last KEPT row (step 129 of the first bulk, 99 of the others), which is not the last row it
    visited, and the labels continue by 3"""
    import fmcmc_amd as F
    Xs, ys, base = linreg_data(5, 130, 3, 5)
    ref = StopRef(O, Xs, ys, O.K_NORMAL, stop_starts(base, 5, 4), 4, 630, 100, burnin=30, thin=3, scale=0.1)
    assert ref.bulks == [130] + [100] * 5 and ref.rows_after.tolist() == [33, 66, 99, 132, 165, 198]
    assert ref.iters[:3].tolist() == [33, 36, 39] and ref.iters[32:35].tolist() == [129, 132, 135]
    t = ref.threshold()
    ans, _kern = ref.run(F, t)
    ref.assert_result(ans, t)
    assert_equals_device_loop(E, ref, ans, t)
    assert ans.to_host()[0][0].mcpar[2] == 3


def test_null_and_an_all_ones_mask_are_the_entry_of_before(E, O):
    """Case.refs of tests/test_gpu_batch.py, two calls with the carried state, both data forms"""
    import torch
    from fmcmc_amd import _abi as abi
    case = linreg_case(O, O.K_RAM, calls=2, lb=-2.0, ub=3.0)
    ones = torch.ones(case.D, dtype=torch.int32, device="cuda")
    for stream_data in (False, True):
        for active in (None, ones):
            gst = E.ChainState(case.init, case.ok.kf)
            for call in range(case.calls):
                rg = E.sweep_batch(case.batch(E), case.spec(E), gst, case.nsteps, seed=case.seed, check=False,
                                   stream_data=stream_data, active=active)
                torch.cuda.synchronize()
                assert abi.last_kernel() == ("batch-stream" if stream_data else "batch-lds")
                case.assert_call(rg, gst, call)
    with pytest.raises(ValueError, match="active"):
        E.sweep_batch(case.batch(E), case.spec(E), E.ChainState(case.init, case.ok.kf), 10, active=torch.ones(case.D, device="cuda"))


def test_a_switched_off_dataset_keeps_every_buffer(E, O):
    """dataset 1 of 3 switched off in the second call of a kernel_adapt case: its chains' state is the first call's, its
    entries of the call's outputs are the prefill, and the other datasets' are the oracle's second call"""
    import torch
    case = linreg_case(O, O.K_ADAPT, calls=2, warmup=10)
    gst = E.ChainState(case.init, case.ok.kf)
    E.sweep_batch(case.batch(E), case.spec(E), gst, case.nsteps, seed=case.seed, check=False)
    torch.cuda.synchronize()
    before = copy.deepcopy({f: getattr(gst, f).cpu().numpy() for f in STATE_FIELDS})
    mask = torch.as_tensor(np.array([1, 0, 1], dtype=np.int32)).cuda()
    rg = E.sweep_batch(case.batch(E), case.spec(E), gst, case.nsteps, seed=case.seed, check=False, active=mask)
    torch.cuda.synchronize()
    off, on = slice(case.Cm, 2 * case.Cm), [0, 1, 4, 5]
    for f in STATE_FIELDS:
        assert _bits_equal(getattr(gst, f)[off].cpu().numpy().astype(np.float64), before[f][off].astype(np.float64)), f
    assert torch.isnan(rg.samples[off]).all() and (rg.status[off] == 0).all() and (rg.accept_count[off] == 0).all()
    assert (rg.status_step[off] == 0).all() and (rg.accept_bits[off] == 0).all() and (rg.status_theta[off] == 0).all()
    ref = case.refs[1]
    assert _bits_equal(rg.samples[on].cpu().numpy(), ref["samples"][on]) and _bits_equal(gst.Sigma[on].cpu().numpy(), ref["Sigma"][on])
    assert _bits_equal(gst.theta0[on].cpu().numpy(), ref["theta0"][on]) and np.array_equal(rg.accept_count[on].cpu().numpy(), ref["accept_count"][on])


def test_a_bad_dataset_still_raises_naming_the_global_chain(E, O):
    import fmcmc_amd as F
    case = bad_dataset_case(O)
    b = F.model_batch(F.gaussian_linreg(case.Xs[d], case.ys[d], guard=False) for d in range(3))
    with pytest.raises(RuntimeError, match=r"fun\(par\) is undefined.*\(chain 2\)"):
        F.MCMC_batch(case.init.reshape(3, 2, 5), b, 30, nchains=2, seed=case.seed, kernel=F.kernel_normal(scale=0.05),
                     stop_each=F.convergence_gelman(10))
