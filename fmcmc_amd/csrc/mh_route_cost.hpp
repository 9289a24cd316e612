// mh_route_cost.hpp -- the cost models of the planners of mh_route.hpp: pure functions of the call (`Call`) and of the shape a
// planner asks about, microseconds per step.  Each is fitted to a named audit; none tests eligibility -- that is the planners'.
// The constants and the order of the floating-point operations decide verdicts at their thresholds: tests/test_route_host.py
// pins them.  Included by mh_route.hpp behind `Call`.
#pragma once

// ---- wide linear models (p >= 16): the chain-sharded / general kernel against the observation-sharded forms.
// Refitted to tools/dispatch_audit.py (profiles/r04_dispatch_audit.md: p = 16 .. 60, n = 1e3 .. 1e4, 64 .. 2048 chains): the
// chain-sharded kernel streams the data set per workgroup (~4 + X bytes / 65 GB/s, the per-CU L2 rate) and pays kernel_ram's
// owner phase (~0.15 us per parameter) in the open.
// (with four / eight chains per workgroup -- more than 512 / 1024 chains -- the data stream is shared by more chains but a step
//  takes 1.3x / 2.4x as long (and the owners of a workgroup queue), and the workgroups run in rounds)
static double est_wide_chain(const Call& c, int cw_now) {
  const fmcmc_model* m = c.m;
  const double rounds = (double)((c.run->nchains + (long long)cw_now * c.ncu - 1) / ((long long)cw_now * c.ncu));
  return (4.0 + (double)m->n * (double)m->p * 8.0 / 65000.0 * (cw_now >= 8 ? 2.4 : (cw_now == 4 ? 1.3 : 1.0)) +
          (c.ram ? (cw_now <= 2 ? 0.12 : 0.075 * (double)cw_now) * (double)c.kn->k : 0.0)) * rounds;
}
// One launch of the sharded forms (the sweep runs as consecutive launches of `per_launch` chains): ~9 us of hand-overs plus a
// slice product that grows with the chains of a launch -- on the matrix cores p (0.08 + 0.00475 slice observations) per 512
// chains -- and the RAM owners hidden in the dataflow form, ~0.17 us per parameter in the sequential one.  `slice`: the
// observation slots of a workgroup's slice, lpw x nslots; `mfma`: the matrix-core form; `cached`: the slice stays in the
// scalar cache (the scalar form walks an uncached one at 2.1x per slot).
static double est_wide_sharded(const Call& c, int slice, long long per_launch, int cw_now, bool mfma, bool cached) {
  const fmcmc_model* m = c.m;
  const long long nchains = c.run->nchains;
  if (!mfma) {
    // (the scalar / register form, fitted at k = 50: ~14 of hand-overs and fixed work + 0.0085 per column and walked observation
    //  slot, + ~6 of barrier imbalance under kernel_ram: n = 2500 loses (23.9 vs 19.1), n = 5000 wins (24.3 vs 30.1), C4 wins 2x)
    const double walked = (cached ? 1.0 : 2.1) * ((slice <= SH_MAXO / 2) ? SH_MAXO / 2 : SH_MAXO);
    return 14.0 + 0.0085 * (double)m->p * walked + (c.ram ? 6.0 : 0.0);
  }
  const double frac = (double)(nchains < per_launch ? nchains : per_launch) / 512.0;
  // (more than three M-tiles: the run-time K-block loop, +5 us; kernel_ram's owners are hidden by the dataflow form only -- more
  //  than 256 chains, at most three M-tiles --, else ~0.17 us per parameter for few chains, ~0.3 in full launches)
  const bool tall = slice > SH_MAXO;
  // (round 5: the dataflow form for 256 chains and fewer too -- two chains per workgroup, half of the workgroups without chains:
  //  C4's shape at 256 / 128 / 64 chains 15.0 / 14.7 / 12.7 us per step against 20.6 / 18.0 / 17.1 on the sequential form)
  const bool hidden = c.ram && !tall && !c.kn->constr && c.K.wide2 != 0 && (nchains > 256 || cw_now == 2);
  // (refitted once more after the compile-time K-block counts of every width: ~10 of hand-overs, 0.4 + p (0.083 + 0.004 slice observations) per 512
  //  chains at up to three M-tiles; the dataflow form's kernel_ram runs ~2 us UNDER the normal kernels' sequential form)
  const bool tall_rt = tall && (m->p + 3) / 4 > 12;     // (tall slices beyond 12 K-blocks keep the run-time loop: ~5 us more)
  double est = 10.2 + (tall_rt ? 5.0 : 0.0) + frac * ((tall ? 0.6 : 0.4) + (double)m->p * ((tall ? 0.08 : 0.083) + (tall ? 0.00475 : 0.004) * (double)slice)) +
               ((c.ram && !hidden) ? (nchains <= 256 ? 0.17 : 0.3) * (double)c.kn->k : 0.0);
  if (hidden) {   // (what the dataflow form hides is at most a quarter of its slice product)
    const double prod = frac * (0.4 + (double)m->p * (0.083 + 0.004 * (double)slice));
    est -= (prod * 0.25 < 2.0 * frac) ? prod * 0.25 : 2.0 * frac;
  }
  return est;
}

// ---- the latency form of the normal / uniform kernels: chains per workgroup (1 .. 3) where mh_sweep_lat beats the MFMA kernel's
// four, else 4.  Fitted to tools/bench_lat_grid.sh and `tools/dispatch_audit.py --only=few` (profiles/r05_dispatch_audit_few.md):
// mh_sweep_lat costs ~0.45 us of fold, barrier and decision plus, per chain of the workgroup, its evaluation (n (p + 2) fp64
// instructions at ~4.7 cycles over four SIMDs; shorter lanes of p >= 4 run at a lower rate) or -- short data -- its coefficient
// broadcast and tree; the MFMA kernel's four chains cost ~0.8 us + 0.06 us per operand group and observation slot.
// n = 10,000, p = 3: 1.03 | 1.62 | 2.15 us with 1 | 2 | 3 chains against 2.0; p = 1: three chains still win (1.54 against
// 2.07); p = 7, n = 1000: two lose (1.22 against 1.13).
static int lat_chains_auto(const Call& c) {
  const fmcmc_model* m = c.m;
  const double w = (double)m->n * (double)(m->p + 2), rate = (m->p <= 3) ? 9.2e-6 : 1.25e-5;
  const double per_chain = (0.10 + rate * w > 0.18 + 0.025 * (double)m->p) ? 0.10 + rate * w : 0.18 + 0.025 * (double)m->p;
  const double t_lat = 0.45 + (double)c.per_cu * per_chain;
  const double ns = (double)c.nsl, ng = (m->p <= 3) ? 1.0 : 2.0;
  const double t_floor = 0.98 + 0.10 * (ng - 1.0);
  const double t_mfma = (0.80 + 0.06 * ng * ns > t_floor) ? 0.80 + 0.06 * ng * ns : t_floor;
  return t_lat < t_mfma ? (int)c.per_cu : 4;
}

// ---- the long-data form (shard_long): fitted on `tools/dispatch_audit.py --only=long` (profiles/r04_dispatch_audit.md): ~8 us of
// hand-overs, the walk of a lane's slots (1.6e-5 us per observation; sums of the logistic terms 1.0e-5) once per group of `lcg`
// chains whose terms fit the LDS, and per chain its terms and its share of the exchange.
static double est_long(const Call& c, long long lcg, bool logistic) {
  const double pn = (double)c.m->n;
  const double groups = (double)((c.run->nchains + lcg - 1) / lcg);
  return 8.3 + groups * (logistic ? 1.0e-5 : 1.6e-5) * pn + (logistic ? 2.0e-6 : 0.5e-6) * pn * (double)(c.m->p + 1) +
         (double)c.run->nchains * (0.17 + 0.028 * (double)c.m->p + (logistic ? 3.0e-6 : 1.2e-6) * pn) +
         (c.adaptive_kind ? 3.5 : 0.0);
}
// what a linear model with few chains costs without it: the chain-sharded kernel beyond the matrix-core slices (p >= 16), the
// fp64-MFMA kernels' rates per observation below (same audit)
static double est_linreg_now(const Call& c) {
  const fmcmc_model* m = c.m;
  const double pn = (double)m->n;
  const double now_rate = (m->p <= 3) ? (pn <= 2e5 ? 3.3e-4 : 5.1e-4) : (m->p <= 7 ? 4.9e-4 /* (round 5 audit: n = 2e4, p = 7, one chain: 9.75 us on the streamed MFMA kernel, the long-data form 10.6) */ : (m->p <= 11 ? 8.5e-4 : 1.17e-3));
  return (m->p >= 16) ? 4.0 + pn * (double)m->p * 8.0 / 65000.0
                      : (m->n <= (long long)NT * fmh::mfma_reg_slots(m->p) ? 2.2 : now_rate * pn) + (c.adaptive_kind ? 2.0 : 0.0);
}
// and a logistic model: the cheaper of one chain-sharded workgroup and the sharded loop, which keeps ONE thread per chain busy
// with its whole slice (n = 1e5, 1 .. 64 chains: 31 .. 36 us per step)
static double est_logit_now(const Call& c) {
  const fmcmc_model* m = c.m;
  const double w1 = (double)m->n * (double)(m->p + 12), stream1 = (double)m->n * (double)(m->p + 1) * 8.0 / 9.0e4;
  const double chain1 = 4.5 + ((w1 * 1.35e-5 > stream1) ? w1 * 1.35e-5 : stream1);
  const double shard1 = 10.3 + 1.78e-5 * (double)m->n * ((double)m->p + 10.3);
  return (chain1 < shard1 || m->p > 16) ? chain1 : shard1;
}

// ---- the logistic family, chain-sharded against observation-sharded (refitted to tools/dispatch_audit.py,
// profiles/r04_dispatch_audit.md: n = 2e3 .. 1e5, p = 2, 5, 8, 64 .. 4096 chains).  The chain-sharded loop costs ~(p + 12)
// instructions per observation and chain, 4.5 + n cw (p + 12) 1.35e-5 with the coefficients in SGPRs (p <= 28 / cw - 1; 2.8e-5 on
// the run-time loop beyond that) -- its lookups scatter over the table: LDS-bound -- but never less than one pass of the
// workgroup over the data set (X only: the term does not read y) at ~90 GB/s; `nblk` workgroups run in rounds.
static double est_logit_chain(const Call& c, int cw, long long nblk) {
  const fmcmc_model* m = c.m;
  const double w = (double)m->n * (double)(m->p + 12);
  const double stream_us = (double)m->n * ((double)m->p + 0.5) * 8.0 / 9.0e4;
  const double loop_us = w * cw * ((m->p <= 28 / cw - 1) ? 1.35e-5 : 2.8e-5);
  const double rounds = (double)((nblk + c.ncu - 1) / c.ncu);
  return (4.5 + (loop_us > stream_us ? loop_us : stream_us)) * rounds;
}
// The sharded form, all launches of the sweep: ~10 us of hand-overs + n (p + 10.3) 1.72e-5 per 512 chains of a launch of
// `ch_launch` chains on `nb_launch` workgroups.  `shadow`: the normal / uniform kernels on mh_sweep_logit2, four chains per
// workgroup whatever cw says and the owners' work in the shadow of the hand-overs -- with logit_shard's issue-priority turns
// 5 .. 15 % off every row of profiles/r05_dispatch_audit_logistic.md (round 5).
static double est_logit_sharded(const Call& c, long long nb_launch, long long ch_launch, bool shadow) {
  const fmcmc_model* m = c.m;
  const long long nchains = c.run->nchains;
  const double launches = (double)((nchains + ch_launch - 1) / ch_launch);
  const double passes = (double)((ch_launch + NT - 1) / NT);                       // chains per thread of the sharded loop
  const double launches_s = shadow ? (double)((nchains + 4 * nb_launch - 1) / (4 * nb_launch)) : launches;
  const double passes_s = shadow ? (double)(((nchains < 4 * nb_launch ? nchains : 4 * nb_launch) + NT - 1) / NT) : passes;
  return ((shadow ? 8.5 : 10.0) + 2.2 * (passes_s - 1.0) +
          (shadow ? 1.62e-5 : 1.72e-5) * (double)m->n * ((double)m->p + 10.3) * passes_s) * launches_s;
}
