"""MCMC_batch(stop_each = convergence_rhat(...)): every dataset stops on its own on the rank-normalised split R-hat (the grouped
call fmcmc_rank_rhat_groups_dev, the loop in mcmc._batch_stop_each) on the GPU.

The reference is built here, dataset by dataset, from the code MCMC(fun = batch[d], conv_checker = convergence_rhat(...)) runs:
engine.sweep(DeviceModel_d, chain_base = d Cm, into = ...) per bulk with the restart from the last kept row, and
convergence_rhat.check_device on the history (tests/test_gpu_batch_stop.py: device_loop does the same for convergence_gelman).  A
chain does not depend on the verdicts, so the reference runs every bulk of every dataset once with a checker that never stops and
a threshold only cuts it.  The threshold (and min_ess) of a case is picked from the reference's own sequences so that at least
one dataset stops before the last bulk, at least one runs them all, and no statistic sits on the threshold.  Everything is
compared to the bit: the same operations in the same order."""
import numpy as np
import pytest

from test_gpu_batch import LINREG, linreg_data
from test_gpu_batch_stop import stop_starts
from test_gpu_parity import _bits_equal

pytestmark = pytest.mark.gpu


class RhatRef:
    """every bulk of every dataset, run on its own: rows, labels, after each bulk the R-hat value and (with min_ess) the least
    effective sample size"""

    def __init__(self, D, Cm, nsteps, freq, autoburnin=True, with_ess=False, n=130, seed=77, scale=0.1, data_seed=5):
        import torch
        import fmcmc_amd as F
        from fmcmc_amd import engine as E
        self.D, self.Cm, self.nsteps, self.freq, self.seed, self.scale = D, Cm, nsteps, freq, seed, scale
        self.autoburnin, self.with_ess = autoburnin, with_ess
        self.Xs, self.ys, base = linreg_data(D, n, 3, data_seed)
        self.init = stop_starts(base, D, Cm)
        self.k = self.init.shape[1]
        self.bulks = F.bulk_plan(nsteps, 0, freq)
        nb, free = len(self.bulks), np.arange(self.k)
        self.vals, self.least = np.full((D, nb), np.nan), np.full((D, nb), np.nan)
        self.samples, self.rows_after = [], None
        for d in range(D):
            model = E.DeviceModel(LINREG, self.Xs[d], self.ys[d])
            kern = F.kernel_normal(scale=scale)
            kern._init(self.k)
            spec, st = kern.spec(model.device), kern.state_for(self.init[d * Cm:(d + 1) * Cm], model.device)
            hist = F.DeviceChains.allocate(Cm, self.k, nsteps, 1, None, 0, Cm, st.device)
            # (min_ess = 0 lets the checker compute the effective sample sizes; the threshold 0 never stops it)
            chk = F.convergence_rhat(freq, threshold=0.0, autoburnin=autoburnin, min_ess=0.0 if with_ess else None)
            rows = []
            for bi, nbulk in enumerate(self.bulks):
                if bi > 0:
                    st.theta0.copy_(hist._samples[:, :, hist.nrows - 1])
                r = E.sweep(model, spec, st, nbulk, seed=seed, chain_base=d * Cm, want_bits=False,
                            into=(hist._samples, hist._logpost, hist._draws), row0=hist.nrows)
                hist.extend(r.iters)
                rows.append(hist.nrows)
                chk.last = None
                assert chk.check_device(hist, free) is False
                if chk.last is not None:
                    self.vals[d, bi] = chk.last
                    if with_ess:
                        both = chk.history[-1][3]
                        self.least[d, bi] = np.nan if np.isnan(both).any() else both.min()
            torch.cuda.synchronize()
            self.samples.append(hist.samples.cpu().numpy())
            self.iters, self.rows_after = hist.iters.copy(), np.array(rows)

    def stops(self, threshold, min_ess=None):
        """(stop[d] = the bulks dataset d runs, did it pass) under convergence_rhat's verdict, from the reference alone"""
        ok = self.vals < threshold
        if min_ess is not None:
            ok &= self.least >= min_ess
        nb = len(self.bulks)
        return np.array([int(np.argmax(b)) + 1 if b.any() else nb for b in ok]), ok.any(axis=1)

    def worth_running(self, threshold, min_ess=None):
        stop, conv = self.stops(threshold, min_ess)
        nb = len(self.bulks)
        v = self.vals[np.isfinite(self.vals)]
        clear = (np.abs(v - threshold) > 1e-6 * threshold).all()
        if min_ess is not None:
            e = self.least[np.isfinite(self.least)]
            clear = clear and (np.abs(e - min_ess) > 1e-6 * min_ess).all()
        return bool((stop < nb).any() and (~conv).any() and clear)

    def threshold(self):
        """of the midpoints of two neighbouring statistics that make the case worth running, the one with the most distinct stop bulks"""
        v = np.unique(self.vals[np.isfinite(self.vals)])
        best, spread = None, 0
        for t in 0.5 * (v[:-1] + v[1:]):
            if self.worth_running(t) and len(set(self.stops(t)[0].tolist())) > spread:
                best, spread = float(t), len(set(self.stops(t)[0].tolist()))
        assert best is not None, "no threshold separates the datasets of this case: %s" % self.vals
        return best

    def threshold_and_min_ess(self):
        """a pair under which the case is worth running AND the effective sample size holds a dataset back whose R-hat passed"""
        v = np.unique(self.vals[np.isfinite(self.vals)])
        e = np.unique(self.least[np.isfinite(self.least)])
        for t in (0.5 * (v[:-1] + v[1:]))[::-1]:                 # (generous thresholds first: the R-hat passes early)
            for m in 0.5 * (e[:-1] + e[1:]):
                if self.worth_running(t, m) and (self.stops(t, m)[0] != self.stops(t)[0]).any():
                    return float(t), float(m)
        raise AssertionError("no (threshold, min_ess) makes the effective sample size decide a stop")

    def run(self, checker):
        import fmcmc_amd as F
        batch = F.model_batch(F.gaussian_linreg(self.Xs[d], self.ys[d]) for d in range(self.D))
        ans = F.MCMC_batch(self.init.reshape(self.D, self.Cm, self.k), batch, self.nsteps, nchains=self.Cm, seed=self.seed,
                           kernel=F.kernel_normal(scale=self.scale), stop_each=checker)
        assert checker.history == [] and checker.last is None and checker.msg == ""      # the checker object is only read
        return ans

    def assert_result(self, ans, threshold, min_ess=None):
        stop, conv = self.stops(threshold, min_ess)
        nb, Cm = len(self.bulks), self.Cm
        print("stop bulks", stop.tolist(), "passed", conv.tolist(), "R-hat\n", self.vals, "\nleast ESS\n", self.least)
        assert (stop < nb).any() and (~conv).any()
        assert ans.steps.tolist() == [sum(self.bulks[:s]) for s in stop] and ans.nrows.tolist() == self.rows_after[stop - 1].tolist()
        assert ans.converged.tolist() == conv.tolist() and ans.ragged
        assert [t for t, _ in ans.rhat_history] == [sum(self.bulks[:b + 1]) for b in range(stop.max())]
        for b, (_total, vals) in enumerate(ans.rhat_history):
            for d in range(self.D):
                if b < stop[d]:
                    assert _bits_equal([float(vals[d])], [float(self.vals[d, b])]), (b, d, vals[d], self.vals[d, b])
                else:
                    assert np.isnan(vals[d]), (b, d)                              # frozen before: not tested
        hs = ans.history._samples.cpu().numpy()
        for d in range(self.D):
            sl, nr = slice(d * Cm, (d + 1) * Cm), int(ans.nrows[d])
            assert _bits_equal(hs[sl, :, :nr], self.samples[d][:, :, :nr]), "rows of dataset %d" % d
            assert np.isnan(hs[sl, :, nr:]).all(), "rows behind the stop of dataset %d" % d
            dc = ans[d]
            assert dc.nrows == nr and dc.iters.tolist() == self.iters[:nr].tolist() and dc.chain_base == d * Cm
            assert _bits_equal(dc.samples.cpu().numpy(), self.samples[d][:, :, :nr])
        return stop, conv


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_every_dataset_stops_where_its_own_run_stops(gpu):
    import fmcmc_amd as F
    ref = RhatRef(5, 3, 600, 100)
    t = ref.threshold()
    ans = ref.run(F.convergence_rhat(100, threshold=t))
    stop, conv = ref.assert_result(ans, t)
    # the diagnostics of the ragged result from the grouped call: a dataset that passed shows the value that stopped it
    diags = F.rhat(ans, autoburnin=True, cols=np.arange(ref.k))
    for d in range(ref.D):
        if conv[d]:
            assert diags[d].rhat.max() == ans.rhat_history[stop[d] - 1][1][d] < t


def test_all_rows_instead_of_the_second_half(gpu):
    import fmcmc_amd as F
    ref = RhatRef(4, 2, 500, 100, autoburnin=False, data_seed=9)
    t = ref.threshold()
    ref.assert_result(ref.run(F.convergence_rhat(100, threshold=t, autoburnin=False)), t)


def test_min_ess_holds_a_dataset_back(gpu):
    import fmcmc_amd as F
    ref = RhatRef(5, 3, 600, 100, with_ess=True)
    t, m = ref.threshold_and_min_ess()
    ans = ref.run(F.convergence_rhat(100, threshold=t, min_ess=m))
    stop, _conv = ref.assert_result(ans, t, m)
    assert (stop != ref.stops(t)[0]).any()


def test_one_chain_per_dataset(gpu):
    import fmcmc_amd as F
    ref = RhatRef(5, 1, 600, 100, data_seed=7)
    t = ref.threshold()
    ref.assert_result(ref.run(F.convergence_rhat(100, threshold=t)), t)


def test_a_window_too_short_is_not_converged(gpu):
    """bulks of 6 steps without autoburnin and with min_ess: the first check sees 6 rows (fewer than 8), value NaN, nobody stops"""
    import fmcmc_amd as F
    Xs, ys, base = linreg_data(3, 50, 3, 5)
    batch = F.model_batch(F.gaussian_linreg(Xs[d], ys[d]) for d in range(3))
    ans = F.MCMC_batch(stop_starts(base, 3, 2).reshape(3, 2, -1), batch, 12, nchains=2, seed=3, kernel=F.kernel_normal(scale=0.1),
                       stop_each=F.convergence_rhat(6, threshold=100.0, autoburnin=False, min_ess=1e-9))
    assert np.isnan(ans.rhat_history[0][1]).all() and np.isfinite(ans.rhat_history[1][1]).all()
    assert ans.steps.tolist() == [12] * 3 and ans.nrows.tolist() == [12] * 3 and not ans.ragged


def test_a_window_beyond_the_grouped_limit_is_checked_dataset_by_dataset(gpu):
    """3 datasets x 1 chain, two bulks of 4200 steps, all rows: the first check ranks M = 4200 values a dataset in the grouped
    call, the second M = 8400, more than a workgroup sorts, through fmcmc_rank_rhat_dev per dataset; both give the values of
    the per-dataset run (the threshold 0 stops nobody: what is compared are the values)"""
    import fmcmc_amd as F
    from fmcmc_amd.summary import rank_groups_fit
    ref = RhatRef(3, 1, 8400, 4200, autoburnin=False, n=50)
    assert ref.bulks == [4200, 4200] and rank_groups_fit(1, 4200) and not rank_groups_fit(1, 8400)
    ans = ref.run(F.convergence_rhat(4200, threshold=0.0, autoburnin=False))
    assert ans.steps.tolist() == [8400] * 3 and not ans.converged.any() and len(ans.rhat_history) == 2
    for b, (_total, vals) in enumerate(ans.rhat_history):
        assert np.isfinite(vals).all() and _bits_equal(vals, ref.vals[:, b]), (b, vals, ref.vals[:, b])
