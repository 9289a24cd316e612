// mh_route.hpp -- the route of a call: which kernel runs it, and in which shape.  plan_route() is a pure function of the
// normalised call, the compute units and the FMCMC_AMD_DEBUG knobs (no HIP call, no allocation); launch_sweep (mh_engine.hip)
// launches what it returns and only steps down from it at run time, fmcmc_plan_route prints it.  The call and what every
// planner needs to know of it are one `Call`, built once; the planners read it and write the `Route`, in the order of the
// table of DESIGN.md section 5; the cost models they ask are mh_route_cost.hpp.  Capacities of the instantiations: mh_kernels.hpp.
// Host code, included by mh_engine.hip behind the kernel headers whose shape helpers it uses.
#pragma once

// LDS bytes of the chain-sharded kernels (mh_streamed.hpp): CW chains per workgroup, tb rows of the sample tile
static size_t sweep_lds_bytes(int k, int kf, int kind, int CW, int tb, int kz, bool resident) {
  size_t d = 5 * (size_t)k + (k / 2 + 1) + (size_t)NW * CW + 1 + (size_t)CW * tb * (kz + 1) + (size_t)CW * k +
             (resident ? (size_t)CW * NT : 0) + (size_t)CW * chain_lds_doubles(k, kf, kind);
  return d * sizeof(double);
}

// ---- diagnosis knobs: ONE environment variable, read once per call --------------------------------------------------------
//   FMCMC_AMD_DEBUG="key=value,key=value"   (unset = product behaviour; nothing else in the environment is looked at)
//   streamed=1   general streamed kernel for everything          cw=1|2|4|8  chains per workgroup of the streamed kernels
//   pipe=0       no materialised-stream kernels (mfma / spec)      lat=0|1|2|3 latency form of mh_sweep_spec: off / chains per workgroup
//   mfma=0       VALU evaluation instead of the fp64-MFMA kernels
//   shard=0|1    wide models: never / always (when eligible) observation-sharded; unset: cost model
//   shard_mfma=0 VALU form of the sharded slice product           wide2=0|1   never / always (when eligible) the dataflow form
//   groups=4     four chain groups in the dataflow form (default two)       tiles=0     even N-tile shares of its evaluator waves
//   window=N     step-window length of the stream-fed kernels (multiple of 32; default: ~256 MiB of stream per window)
//   t10=0        the sharded slice product's third M-tile as a 16x16x4 tile even where 8 of its rows are padding
//   shadow=0     logistic, observation-sharded: the normal / uniform kernels on the general kernel's form, not on mh_sweep_logit2
//   speclogit=0  logistic family: not on the wave-specialised kernel (mh_sweep_spec<.., LOGISTIC>)
//   specbnd=0    the bounded kernel_ram: not on the wave-specialised kernel (SpecSyncB)
//   specmirror=0 the mirror kernels: not on the wave-specialised kernel
//   tinymfma=0   the streamed MFMA forms (8 .. 15 covariates, mirror / adaptive kernels) only from 513 observations on
//   specwide=0   kernel_adapt / kernel_ram with 8 .. 14 covariates on small data: not on the wave-specialised kernel
//   specp0=0     models without a covariate (iid Normal): adaptive / mirror kernels not on the wave-specialised kernel
//   turn=<t>     logit_shard's issue-priority turn (timing only): thousandths of the younger wave's passes it starts from, + 10000: and
//                stays at, + 100000 x (lead in units of 256 cycles it is regulated towards); turn=0: no turn
//   bigkhbm=1    more parameters than a wavefront has lanes: the HBM form of mh_sweep_bigk even where the LDS form fits
//   mode=<bits>  timing ablations and stamps (SweepArgs.debug)
// The kernel a call ended up on is reported by fmcmc_last_kernel(); DESIGN.md section 5 has the shape -> kernel table.
#define FMCMC_KNOBS(X) \
  X(streamed, -1) X(cw, -1) X(pipe, -1) X(lat, -1) X(mfma, -1) X(shard_mfma, -1) X(shard, -1) X(wide2, -1) X(groups, -1) X(tiles, -1) \
  X(t10, -1) X(window, -1) X(mode, 0) X(shadow, -1) X(turn, -1) X(speclogit, -1) X(specbnd, -1) X(specmirror, -1) X(specp0, -1) \
  X(tinymfma, -1) X(specwide, -1) X(bigkhbm, -1)
struct Knobs {
#define X(name, unset) int name = unset;
  FMCMC_KNOBS(X)
#undef X
};
static Knobs read_knobs() {
  Knobs K;
  const char* e = getenv("FMCMC_AMD_DEBUG");
  if (!e) return K;
#define X(name, unset) {#name, &K.name},
  struct { const char* name; int* dst; } tab[] = {FMCMC_KNOBS(X)};
#undef X
  while (*e) {
    const char* eq = strchr(e, '=');
    const char* end = strchr(e, ',');
    if (!end) end = e + strlen(e);
    if (eq && eq < end)
      for (auto& t : tab)
        if ((size_t)(eq - e) == strlen(t.name) && !strncmp(e, t.name, (size_t)(eq - e))) *t.dst = atoi(eq + 1);
    e = (*end == ',') ? end + 1 : end;
  }
  return K;
}

// ---- the route of a call: which kernel runs it, and in which shape (DESIGN.md section 5 has the table) ------------------------
// (one per kernel family and form; kernel_name: what fmcmc_last_kernel() reports for it)
enum class Form { BIGK, RESIDENT, GENERAL, LONG, MFMA, MFMA_STREAMED, MFMA_ADAPTIVE, LAT, LAT_LOGIT, SPEC, SPEC_LOGIT,
                  LOGISTIC, LOGISTIC_SHARDED, LOGISTIC_SHADOW, WIDE, WIDE_SHARDED, WIDE_SHARDED_MFMA, WIDE_DATAFLOW, BIGK_HBM };
struct Route {
  Form form = Form::GENERAL;   // what runs the call (LONG and LOGISTIC_SHADOW: set by their launchers only, once they ran)
  Form base = Form::GENERAL;   // the chain-sharded form beneath a fast or sharded one: what a run-time step down takes
  const void* kfn = nullptr, *kfn_base = nullptr;   // their handles (MFMA forms: chosen per launch, BIG depends on its size)
  size_t lds = 0, lds_run = 0;  // LDS bytes of `base`, of a sharded `form`
  bool lds_exceeded = false;   // the call's chain blocks do not fit the LDS: unsupported
  bool no_kernel = false;      // the planned form has no kernel handle and nothing beneath it: refused with a message
  int cw = 1, tb = 32, res_p = -1;
  long long nblk = 0;
  bool wide_switched = false;  // two chains per workgroup BECAUSE the observation-sharded sweep pays
  // stream-fed forms (mh_sweep_mfma / _mfma_ad / _spec / _lat)
  int pipe_opt = 0, spec_cw = 4, mfma_ng = 0, mfma_ext = 0, mfma_ad = 0, kx = 0;
  bool ring = false;           // kernel_adapt(freq > 1) on the LDS ring of mh_sweep_spec
  long long win = 0;           // step-window length (0: one launch)
  // observation-sharded forms: workgroups and chains per launch, slots of 512
  long long nb_launch = 256, ch_launch = 0;
  int nslots = 0;
  // logistic: the instantiation without generators (stream-fed), the shadow form and its launch width
  const void* kfn_fed = nullptr, *kfn_shadow = nullptr;
  size_t lds_shadow = 0;
  long long ch_shadow = 0;
  // wide: lanes per workgroup, matrix-core slices, the dataflow form's tiles and groups
  int lpw = 0, nmt = 0, t10 = 0, mblk = 0, ngrp = 0, tiles = 0;
  bool mfma_form = false, wide2 = false;
  // the long-data form, tried first when set: its handle, LDS, chains per group and LDS doubles per chain
  const void* kfn_long = nullptr; size_t lds_long = 0; long long lcg = 0, lrow = 0;
};

// the stream-fed forms (step windows, launch_fast)
static bool stream_fed(Form f) {
  return f == Form::MFMA || f == Form::MFMA_STREAMED || f == Form::MFMA_ADAPTIVE || f == Form::LAT || f == Form::LAT_LOGIT || f == Form::SPEC || f == Form::SPEC_LOGIT;
}

// the report of fmcmc_last_kernel()
static const char* kernel_name(const Route& R) {
  static const char* const name[] = {"big-k", "resident", "streamed", "long-sharded", "mfma", "mfma-streamed", "mfma-adaptive", "lat",
      "lat-logit", "spec", "spec-logit", "streamed-logistic", "logistic-sharded", "logistic-shadow", "streamed-wide",
      "streamed-wide-sharded", "streamed-wide-sharded-mfma", "wide-dataflow", "big-k-hbm"};
  // (the register forms by their chains per workgroup: lat1 .. lat4, lat-logit1 .. 4; spec-lat1 .. 3 | spec, spec-logit-lat1 .. 3 | spec-logit)
  static const char* const by_cw[4][4] = {{"lat1", "lat2", "lat3", "lat4"}, {"lat-logit1", "lat-logit2", "lat-logit3", "lat-logit4"},
      {"spec-lat1", "spec-lat2", "spec-lat3", "spec"}, {"spec-logit-lat1", "spec-logit-lat2", "spec-logit-lat3", "spec-logit"}};
  static_assert(sizeof(name) / sizeof(name[0]) == (size_t)Form::BIGK_HBM + 1, "one name per Form");
  static_assert(sizeof(by_cw) / sizeof(by_cw[0]) == (size_t)Form::SPEC_LOGIT - (size_t)Form::LAT + 1, "one row per register form");
  const int c = (R.spec_cw >= 1 && R.spec_cw <= 3) ? R.spec_cw - 1 : 3;
  if (R.form >= Form::LAT && R.form <= Form::SPEC_LOGIT) return by_cw[(int)R.form - (int)Form::LAT][c];
  return name[(int)R.form];
}

// ---- the call as the planners see it: the normalised call (iid Normal as the linear model without covariate, the uniform
// kernels as the normal ones), the device's compute units, the knobs, and the facts more than one planner asks for
struct Call {
  const fmcmc_model* m; const fmcmc_kernel* kn; const fmcmc_run* run;
  int kf, ram_bounded, kz;     // free parameters, a bounded free parameter (kernel_ram's second evaluation), variates per step
  long long ldS;               // row stride of the outputs
  int ncu;
  Knobs K;
  bool linreg, logistic;
  bool normal_kind;            // kernel_normal(_reflective), and the uniform kernels they stand for
  bool adaptive_kind;          // kernel_adapt / kernel_ram
  bool mirror, adapt, ram, ram_bnd, joint, philox;
  bool adapt_hist;             // kernel_adapt that reads earlier rows (bw > 0 or freq > 1) ...
  bool adapt_ring;             // ... and can keep them in the LDS ring of mh_sweep_spec
  bool single_lat;             // a single-parameter scheme the latency form's candidate wave takes
  long long nsl, nsl2;         // observation slots of 512, rounded up to even
  long long per_cu;            // chains per compute unit, rounded up
  bool lat_forced, force;      // knobs lat=1|2|3, streamed=1
};

// Step windows of the stream-fed kernels (library's own stream): ~256 MiB of stream per window, from 32 steps, a multiple of 32
// (knob window=N).  The ring of kernel_adapt(freq > 1) on mh_sweep_spec is only correct for a call that is one window.
static long long step_window(const fmcmc_run* run, int kz, const Knobs& K) {
  const long long per_step = (long long)run->nchains * (kz + 1) * 8;
  long long win = ((256ll << 20) / (per_step > 0 ? per_step : 1)) & ~31ll;
  if (win < 32) win = 32;     // (the kernels take windows from 32 steps; a 512-step floor let the buffer grow with nchains without bound)
  if (K.window >= 32) win = (long long)K.window & ~31ll;      // (diagnosis / tests: a window length)
  return win;
}

static Call make_call(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run, int kf, int ram_bounded, int kz, long long ldS,
                      int ncu, const Knobs& K) {
  Call c{m, kn, run, kf, ram_bounded, kz, ldS, ncu, K};
  c.linreg = m->family == FMCMC_FAM_GAUSSIAN_LINREG;
  c.logistic = m->family == FMCMC_FAM_LOGISTIC;
  c.normal_kind = kn->kind == FMCMC_KERNEL_NORMAL || kn->kind == FMCMC_KERNEL_NORMAL_REFLECTIVE;
  c.adapt = kn->kind == FMCMC_KERNEL_ADAPT;
  c.ram = kn->kind == FMCMC_KERNEL_RAM;
  c.adaptive_kind = c.adapt || c.ram;
  c.mirror = kn->kind == FMCMC_KERNEL_NMIRROR || kn->kind == FMCMC_KERNEL_UMIRROR;
  c.ram_bnd = c.ram && ram_bounded;
  c.joint = kn->scheme == FMCMC_SCHEME_JOINT;
  c.philox = run->rng_mode == FMCMC_RNG_PHILOX;
  c.adapt_hist = c.adapt && (kn->bw > 0 || kn->freq > 1);
  // kernel_adapt(freq = 2 .. 8, bw = 0) on the register owner of mh_sweep_spec (round 5: the last `freq` rows of a chain in an LDS ring;
  // tools/option_audit.py had it on the general kernel at 14.7 us per step where freq = 1 takes 3.3): no fixed parameter, k <= 8, and a
  // call that is ONE step window (the ring does not travel between windows)
  c.adapt_ring = c.adapt && kn->bw == 0 && kn->freq >= 2 && kn->freq <= SPEC_FREQMAX && kf == kn->k && kz == kn->k &&
                 kn->k <= SPEC_KA && (run->nsteps <= step_window(run, kz, K) + 1 || !c.philox);
  // single-parameter schemes of the normal / uniform kernels ("ordered", an explicit sequence, "random"): on mh_sweep_lat's candidate
  // wave (round 5: they ran on the general kernel, 2.9 us per step at the README's size where the joint scheme takes 0.63), one to FOUR
  // chains per workgroup; "random" draws its plan in the kernel and hands it back (a caller-fed plan stays general)
  c.single_lat = c.normal_kind && !c.joint && K.lat != 0 && (kn->scheme != FMCMC_SCHEME_RANDOM || c.philox);
  c.nsl = (m->n + NT - 1) / NT;
  c.nsl2 = (c.nsl + 1) & ~1ll;
  c.per_cu = (run->nchains + ncu - 1) / ncu;
  c.lat_forced = K.lat >= 1 && K.lat <= 3;
  c.force = K.streamed == 1;
  return c;
}

#include "mh_route_cost.hpp"

// What is left of the size limits of the stream-fed kernels (round 3: rows and variates are addressed as 64-bit chain base +
// 32-bit offset, and a long call runs as step windows with a bounded stream): offsets inside ONE chain's blocks are 32 bits.
static bool offsets_fit(const Call& c, long long step_bound) {
  return (unsigned long long)c.run->nsteps * (unsigned long long)c.kz * 8ull < (1ull << 32) && c.run->nsteps < step_bound &&
         (unsigned long long)c.kn->k * (unsigned long long)c.ldS * 8ull < (1ull << 32);
}

// The matrix-core slice of a workgroup of the observation-sharded wide forms: slots per lane group, M-tiles, doubles of the
// slice block in LDS (lpw = 0, not sharded: an empty slice)
struct SliceShape { int spg, nmt, mblk; };
static SliceShape wide_slice_shape(long long nsl, int lpw, int p) {
  SliceShape s;
  s.spg = lpw > 0 ? ((int)nsl + 4 / lpw - 1) / (4 / lpw) : 0;
  s.nmt = (s.spg + 3) / 4;
  s.mblk = shm_hdr(s.nmt) + s.nmt * ((p + 3) / 4) * 64;
  return s;
}

// Observation-sharded evaluation (mh_common.hpp, eval_sharded): `nb` workgroups per launch must split the 512 canonical
// lanes evenly (128 or 256 of them), be co-resident (cooperative launch) and hold their slice in SH_MAXO registers.
// Returns the canonical lanes per workgroup (2 or 4), or 0 when the shape is not eligible or the cost model (est_wide_chain
// against est_wide_sharded) prefers the chain-sharded kernel.  `shard`: knob shard -- 1 forces the sharded kernel for every
// eligible shape (tests), 0 disables it.  cw_now: chains per workgroup the call would run with on the chain-sharded / general kernel.
static bool shard_mfma_enabled(const Knobs& K) { return K.shard_mfma != 0; }
static int wide_sharded_lanes(const Call& c, int shard, long long nb, int cw_now) {
  const fmcmc_model* m = c.m;
  if (shard == 0) return 0;
  if (!c.linreg || m->p < 16) return 0;
  if (!c.ram && !c.normal_kind) return 0;
  const int lpw = (nb == 128 || nb == 256) ? (int)(NT / nb) : 0;
  const int slice = lpw * (int)c.nsl;
  const long long per_launch = nb * 2;   // (upper bound of the chains of one launch: at most two per workgroup)
  // A slice of more than 49 columns (15.5 KB) no longer stays in the scalar cache: 2.1x per walked slot, still ahead for the
  // normal kernels (k = 64, n = 10k: 57 us per step against 78); kernel_ram stays chain-sharded there, its owner phase
  // dominates at that width and runs slower in the sharded instantiation (121 against 108).
  const bool cached = shard_mfma_enabled(c.K) || (size_t)m->p * SH_MAXO * sizeof(double) <= 15872;   // (the MFMA form keeps the slice in LDS)
  // (a slice holds up to SH_MAXO = 40 observations in the scalar / register form, up to 4 SHM_T = 96 -- six M-tiles -- in LDS for the
  //  matrix-core form: n <= 24,576 at 256 workgroups)
  const bool mf_ok = shard_mfma_enabled(c.K) && m->p <= 4 * SHM_KBMAX;
  const bool ok = lpw > 0 && !(c.ram && (c.ram_bounded || !cached)) && slice <= (mf_ok ? 4 * SHM_T : SH_MAXO) && nb <= c.ncu &&
                  (long long)m->p * SH_MAXO * nb < (1ll << 28) && (long long)(m->p + 1) * (per_launch + SH_PAD) < (1ll << 31) &&
                  c.run->nsteps < 30000000;   /* barrier epochs (2 per step) x workgroups per group stay below 2^32 */
  if (!ok) return 0;
  if (shard != 1) {
    const double launches = (double)((c.run->nchains + per_launch - 1) / per_launch);
    if (!(est_wide_sharded(c, slice, per_launch, cw_now, mf_ok, cached) * launches < 0.95 * est_wide_chain(c, cw_now))) return 0;
  }
  return lpw;
}

// ---- the planners, in the order plan_route calls them.  Each reads the Call and the Route so far and writes the Route.

// more parameters than a wavefront has lanes: one workgroup per chain (mh_bigk.hpp); fmcmc_validate has refused what it lacks.
// Its matrices in LDS wherever they fit (every k <= 128; kernel_adapt up to 133, kernel_ram up to 183 free parameters),
// in the chain's own Sigma square in HBM beyond (knob bigkhbm=1: always)
static bool plan_bigk(const Call& c, Route& R) {
  const fmcmc_kernel* kn = c.kn;
  if (kn->k <= FMCMC_MAX_K_WAVE) return false;
  const size_t lds = sizeof(double) * bigk_lds_doubles(kn->k, c.kf, kn->kind);
  const bool hbm = c.K.bigkhbm == 1 || lds > 160 * 1024;
  R.form = R.base = hbm ? Form::BIGK_HBM : Form::BIGK;
  R.kfn = R.kfn_base = fmh::k_bigk(hbm ? 1 : 0);
  R.lds = hbm ? sizeof(double) * bigk_lds_doubles(kn->k, c.kf, kn->kind, true) : lds;
  R.lds_exceeded = R.lds > 160 * 1024;
  R.no_kernel = R.kfn == nullptr;
  return true;
}

// kernel_ram on a wide model with ONE chain per CU or fewer: two per workgroup all the same, so that the sweep is eligible for the
// dataflow form (mh_wide2.hpp: two chain groups half a step out of phase; workgroups without chains evaluate like the others)
static bool dataflow_for_few_chains(const Call& c) {
  const fmcmc_model* m = c.m; const fmcmc_kernel* kn = c.kn; const fmcmc_run* run = c.run;
  const SliceShape s = wide_slice_shape(c.nsl, 2, m->p);
  return c.ncu == 256 && c.K.wide2 != 0 && c.linreg && m->p >= 16 && m->p <= 4 * SHM_KBMAX &&
         c.ram && !c.ram_bounded && !kn->constr && shard_mfma_enabled(c.K) &&
         2 * c.nsl <= SH_MAXO && run->nchains >= 2 &&
         !((run->nchains + 1) / 2 == 128 && 4 * c.nsl <= SH_MAXO) &&      /* (exactly 128 workgroups of four lanes: the sequential form's own shape) */
         c.nsl >= 6 &&      /* (short data: the chain-sharded sweep is ahead -- p = 30, n = 1000, 64 chains: 9.7 against 11.6 us) */
         /* (its LDS: two owners' factor and partial sums + the slice block -- k = 62 does not fit) */
         s.nmt >= 1 && s.nmt <= 3 && sizeof(double) * wide2_lds_doubles(kn->k, c.kf, kn->kind, c.kz, s.mblk) <= 160 * 1024 &&
         wide_sharded_lanes(c, c.K.shard, (long long)c.ncu, 2) > 0;
}

// The chain blocks of the chain-sharded kernels, which every other form steps down to: the register-resident variant, chains
// per workgroup, rows of the sample tile, LDS.  False: they do not fit the LDS (R.lds_exceeded).
static bool plan_chain_blocks(const Call& c, Route& R) {
  const fmcmc_model* m = c.m; const fmcmc_kernel* kn = c.kn; const fmcmc_run* run = c.run; const Knobs& K = c.K;
  // register-resident variant: Gaussian linreg whose data fits the VGPR budget of 512 threads
  if (!c.force && c.linreg && !c.mirror) {
    static const int variants[][2] = {{1, 4}, {3, 20}};
    for (auto& v : variants)
      if (m->p == v[0] && m->n > (long long)NT * (v[1] - RES_MASKED) && m->n <= (long long)NT * v[1]) R.res_p = v[0];
  }
  const bool resident = R.res_p >= 0;
  // chains per workgroup: fill the CUs first, then stack chains on a workgroup
  int cw = 1;
  if (resident) {
    cw = 4;
  } else {
    while (cw < NW && (long long)cw * c.ncu < run->nchains) cw <<= 1;
    if (K.cw == 1 || K.cw == 2 || K.cw == 4 || K.cw == 8) cw = K.cw;   // diagnosis: chains per workgroup of the streamed kernel
    // wide linear models with more than two chains per CU: two chains per workgroup, so that the sweep can run as
    // consecutive observation-sharded launches of 2 x CUs chains each (plan_base_wide) when that pays off
    // (measured at k = 50, n = 10k: 1024 chains 63.8 us per step instead of 71.6 with four chains per workgroup; at 2048
    //  chains the general kernel with eight chains per workgroup is level, 123 vs 128, and keeps the sweep)
    else if (cw >= 4 && wide_sharded_lanes(c, K.shard, (long long)c.ncu, cw) > 0) { cw = 2; R.wide_switched = true; }
    else if (cw == 1 && dataflow_for_few_chains(c)) { cw = 2; R.wide_switched = true; }
    // the logistic-only instantiations (table in LDS; observation-sharded form) exist for up to four chains per workgroup: more
    // than 1024 chains run as more workgroups / consecutive sharded launches there, not on the all-family kernel with eight
    // chains per workgroup (tools/dispatch_audit.py: 4096 chains, n = 1e5, p = 5 took 1244 us per step, 4.7x four launches)
    else if (cw > 4 && c.logistic && !c.mirror) cw = 4;
  }
  int tb = 32;
  while (tb > 1 && sweep_lds_bytes(kn->k, c.kf, kn->kind, cw, tb, c.kz, resident) > 60 * 1024) tb >>= 1;
  while (cw > 1 && !resident && sweep_lds_bytes(kn->k, c.kf, kn->kind, cw, tb, c.kz, resident) > 150 * 1024) cw >>= 1;
  R.cw = cw; R.tb = tb;
  R.lds = sweep_lds_bytes(kn->k, c.kf, kn->kind, cw, tb, c.kz, resident);
  if (R.lds > 160 * 1024) { R.lds_exceeded = true; return false; }
  R.nblk = (run->nchains + cw - 1) / cw;
  R.ch_launch = run->nchains;
  R.nslots = (int)c.nsl;
  return true;
}

// mh_sweep_spec / mh_sweep_lat hold the model of `c` in their compute lanes' registers (the slot count an even run-time choice
// among their compute loops): 1 .. 7 covariates; none at all -- the iid Normal family, intercept + sigma: the lanes then hold
// no x (round 5, knob specp0=0: off); 8 .. 14 on up to 2048 observations -- four slots of P doubles per lane, the register
// owner at the compile-time width k <= 16 (round 5, knob specwide=0: the streamed MFMA evaluation with the owners in LDS)
static bool spec_holds_p(const Call& c) {
  const fmcmc_model* m = c.m;
  const bool p_ok = m->p >= 1 || (m->p == 0 && m->intercept && c.K.specp0 != 0);
  return p_ok && (m->p <= 7 || (m->p <= 14 && c.K.specwide != 0));
}

// ---- the stream-fed forms of the linear model: mh_sweep_mfma (fp64-MFMA), mh_sweep_mfma_ad, mh_sweep_spec, mh_sweep_lat.
// Writes the form and its shape (pipe_opt, spec_cw, mfma_ng / _ext / _ad, kx); commit_register_form confirms a register form.
static void plan_linreg_stream_fed(const Call& c, Route& R) {
  const fmcmc_model* m = c.m; const fmcmc_kernel* kn = c.kn; const fmcmc_run* run = c.run; const Knobs& K = c.K;
  const int kf = c.kf, kz = c.kz;
  const long long nsl = c.nsl, nsl2 = c.nsl2;
  if (!(!c.force && K.pipe != 0 && c.linreg &&
        (c.normal_kind || (c.adapt && (!c.adapt_hist || c.adapt_ring)) || (c.ram && !kn->constr) ||
         (c.mirror && c.joint && kf == kn->k && K.mfma != 0)) &&
        (c.joint || c.adaptive_kind || c.single_lat) && kn->k <= PIPE_KMAX && offsets_fit(c, 1ll << 30) &&
        /* (round 5: kernel_adapt / kernel_ram run in step windows too -- their step-dependent rules read the CALL's step;
            what still materialises its whole stream, kept below 8 GiB: host-fed variates are the caller's, and the mirror kernels) */
        (!c.mirror || (unsigned long long)run->nchains * (unsigned long long)run->nsteps * (unsigned long long)(kz + 1) * 8ull < (8ull << 30)))) return;
  int pipe_opt = 0, mfma_ng = 0, mfma_ad = 0, mfma_ext = 0, spec_cw = 4;
  bool lat_normal = false;   // the latency form (mh_sweep_lat)
  // the wave-specialised kernel (mh_sweep_spec): x of a compute lane in VGPRs, up to reg_slots(p) slots
  // (the bounded kernel_ram decides on f of the REFLECTED proposal: a second evaluation in the steps in which the reflection
  //  moved something -- the barrier-synchronised owners of mh_sweep_mfma_ad ask for it between barriers, this kernel's register
  //  owners through a second evaluation slot per step (round 5, SpecSyncB: k <= 8, no fixed parameter; knob specbnd=0: off))
  const bool bnd_ok = K.specbnd != 0 && kf == kn->k && (kn->k <= SPEC_KA || (kn->k == 9 && m->p == 7)) && kz == kn->k && !kn->constr;   // (k = 9: the compile-time owner of p = 7)
  if (spec_holds_p(c) && nsl2 <= fmh::reg_slots(m->p) && c.adaptive_kind && (!c.ram_bnd || bnd_ok)) pipe_opt = (int)nsl2;
  // (normal / uniform kernels run on the MFMA kernel; knob mfma=0 keeps them here for the two shapes they were tuned at)
  if (m->p == 3 && nsl == 20 && c.normal_kind && c.joint) pipe_opt = 20;
  if (m->p == 1 && nsl == 2 && c.normal_kind && c.joint) pipe_opt = 2;
  // (round 5: the streamed forms from ONE observation on -- up to 512 the one resident slot is the last, nothing is streamed; models with
  //  8 .. 15 covariates on small data ran on the general kernel, 2.4 - 5 / 9 - 26 us per step.  Knob tinymfma=0: from 513 on, as before)
  const long long nt_min = (K.tinymfma != 0) ? 0 : (long long)NT;
  const int ng_p = (m->p <= 3) ? 1 : (m->p <= 7 ? 2 : (m->p <= 11 ? 3 : 4));   // operand groups per observation slot
  const int nsr_p = (ng_p == 1) ? MfmaAdShape<1>::NSR : (ng_p == 2 ? MfmaAdShape<2>::NSR : MfmaAdShape<3>::NSR);
  // fp64-MFMA evaluation: general in n and p up to what 80 operand registers per lane hold (normal / uniform kernels)
  if (K.mfma != 0 && c.normal_kind && c.joint) {
    if (m->n <= (long long)NT * fmh::mfma_reg_slots(m->p)) mfma_ng = (m->p <= 3) ? 1 : 2;
    // beyond the operand registers: 16 (8) slots resident, the rest streamed from an operand-order copy every step (EXT)
    else if (m->p <= 3 && m->n < (1ll << 29)) { mfma_ng = 1; mfma_ext = 16; }
    else if (m->p <= 7 && m->n < (1ll << 29)) { mfma_ng = 2; mfma_ext = 8; }
    // 8 .. 15 covariates (k <= 16): three / four operand groups per observation slot, four / two slots resident (one for short
    // data), the rest streamed -- tools/dispatch_audit.py found these models on the general kernel at 0.10 of the fp64 peak where
    // p = 7 runs at 0.44
    else if (m->p <= 11 && m->n > nt_min && m->n < (1ll << 29)) { mfma_ng = 3; mfma_ext = (m->n > (long long)NT * 4) ? 4 : 1; }
    else if (m->p <= 15 && m->n > nt_min && m->n < (1ll << 29)) { mfma_ng = 4; mfma_ext = (m->n > (long long)NT * 2) ? 2 : 1; }
    // (the wave-specialised VALU kernel, which overlaps owners and evaluation, used to win at its small shape
    //  (p = 1, n ~ 1000); since the instruction diet of the owner phase the MFMA kernel is 1.2-1.35x ahead there too:
    //  tools/bench_small.py.  Knob mfma=0 still selects it.)
  }
  // kernel_adapt / kernel_ram beyond mh_sweep_spec's registers: the same streamed MFMA evaluation with the register-row
  // adaptive owners between barriers (mh_mfma_ad.hpp); no fixed parameter, k <= 8
  // (k = 9 -- seven covariates, intercept and sigma -- as a compile-time row count: tools/dispatch_audit.py found these calls on
  //  the general kernel, 7x the time of the normal kernels at the same shape)
  // (mfma_ad == 2: the owners with their matrices in LDS -- 8 .. 15 covariates, or a fixed parameter; not the bounded kernel_ram,
  //  which then stays on the general kernel)
  if (K.mfma != 0 && !pipe_opt && !c.adapt_hist && c.adaptive_kind && m->p >= 0 && m->p <= 15 && m->n < (1ll << 29)) {   // (p = 0: iid Normal)
    // (round 5: the run-time-width register owner takes fixed parameters -- free ones first, the fixed ones as passengers)
    const bool reg_owner = m->p <= 7 && kz == kf && kf >= 1 && ((kf == kn->k && (kn->k <= SPEC_KA || kn->k == 9)) || (kf < kn->k && kn->k <= SPEC_KA));
    if (m->n > (long long)NT * nsr_p && (reg_owner || !c.ram_bnd)) {   // (its resident slots are all full)
      mfma_ad = reg_owner ? 1 : 2;
      mfma_ng = ng_p;
      mfma_ext = nsr_p;
    } else if (m->n > nt_min && ((reg_owner && (c.ram_bnd || m->p == 0)) || (!reg_owner && !c.ram_bnd && run->nchains <= 2048 /* (beyond: level with the general kernel at eight chains per workgroup) */))) {
      // short data (one slot resident, the rest streamed) for what the wave-specialised kernel does not take: the bounded
      // kernel_ram, 8 .. 15 covariates, no covariate at all (iid Normal)
      mfma_ad = reg_owner ? 1 : 2;
      mfma_ng = ng_p;
      mfma_ext = 1;
    }
  }
  // the mirror kernels (joint scheme, no fixed parameter): their owner between the barriers of the same streamed MFMA evaluation
  // (round 5: within mh_sweep_spec's registers their owner runs there -- beside the evaluation instead of between barriers, and in
  //  the latency forms; up to 512 observations they ran on the general kernel.  Knob specmirror=0: off)
  if (c.mirror) {
    if (K.specmirror != 0 && spec_holds_p(c) && nsl2 <= fmh::k_spec_optmax(m->p, kn->kind)) pipe_opt = (int)nsl2;
    else if (m->p <= 15 && m->n > nt_min && m->n < (1ll << 29)) { mfma_ad = 3; mfma_ng = ng_p; mfma_ext = (m->n > (long long)NT * nsr_p) ? nsr_p : 1; }
  }
  // ---- the LATENCY form (round 5): fewer than four chains per compute unit.  The reference scales a FIXED number of chains
  // over its workers (R/mcmc.R:536-641), and a sharded call leaves every GPU nchains / G of them: with four chains per
  // workgroup a step of C2's shape costs the same 2 us at 64 chains and at 1024.  Here the wave-specialised kernel runs one,
  // two or three chains per workgroup -- all eight compute waves on the chain(s) there are (an evaluation of n = 10,000 is
  // 0.33 us of one CU's fp64 issue), no owner queued behind the evaluation of other chains -- for every shape its compute
  // lanes hold in registers: kernel_adapt / kernel_ram on mh_sweep_spec (its owners no longer queue behind the evaluation of
  // other chains), the normal / uniform kernels on mh_sweep_lat (mh_lat.hpp: chain state replicated in every wave, ONE barrier
  // per step).  Same canonical lanes and tree: the bits do not depend on the form.  Knob lat=0: off; lat=1|2|3: forced.
  // (8 .. 15 covariates on up to 2048 observations, round 5: mh_sweep_lat<KIND, P, 4> -- the joint scheme with ONE chain per compute unit
  //  (1.2 us per step on the streamed MFMA form at any chain count), the single-parameter schemes up to four (general kernel before))
  const bool wide_lat = K.lat != 0 && K.specwide != 0 && c.normal_kind && m->p >= 8 && m->p <= 15 && nsl2 <= fmh::reg_slots(m->p) && kf >= 1;
  if (wide_lat && c.joint && (c.per_cu <= 1 || c.lat_forced)) {
    pipe_opt = (int)nsl2; mfma_ng = 0; mfma_ext = 0; lat_normal = true;
    spec_cw = c.lat_forced ? K.lat : 1;
  } else if (c.single_lat) {
    if (c.per_cu <= 4 && m->p >= 0 && (m->p <= 7 ? nsl2 <= fmh::k_spec_optmax(m->p, kn->kind) : wide_lat)) {
      pipe_opt = (int)nsl2; mfma_ng = 0; lat_normal = true;
      spec_cw = c.lat_forced ? K.lat : (int)c.per_cu;
    }
  } else if (K.lat != 0 && (pipe_opt || (mfma_ng && !mfma_ext && !mfma_ad))) {
    // kernel_adapt / kernel_ram (mh_sweep_spec) gain up to 25 % with one chain per workgroup, 18 % with two, 6 % with three at
    // n = 10,000 and are level at small n -- their step is the owner's dependent chain --: one to three, always.  The normal
    // kernels by lat_chains_auto's cost model.
    const int lcw_auto = c.per_cu > 3 ? 4 : (c.normal_kind ? lat_chains_auto(c) : (int)c.per_cu);
    const int lcw = c.lat_forced ? K.lat : lcw_auto;
    // (p = 0 -- the iid Normal family -- included: the compute lanes then hold no x)
    if (lcw < 4 && nsl2 <= fmh::k_spec_optmax(m->p, kn->kind)) {
      if (c.normal_kind) { pipe_opt = (int)nsl2; mfma_ng = 0; lat_normal = true; }
      if (pipe_opt && !mfma_ng) spec_cw = lcw;
    }
  }
  R.pipe_opt = pipe_opt; R.spec_cw = spec_cw; R.mfma_ng = mfma_ng; R.mfma_ext = mfma_ext; R.mfma_ad = mfma_ad;
  if (mfma_ng) {
    R.form = mfma_ad ? Form::MFMA_ADAPTIVE : (mfma_ext ? Form::MFMA_STREAMED : Form::MFMA);
    if (mfma_ad) {
      // kernel_adapt / kernel_ram / mirror kernels: the adaptive owners between the barriers of the streamed evaluation (mh_mfma_ad.hpp)
      R.kx = (mfma_ad == 3) ? -2 : (mfma_ad == 2) ? -1 : ((kf != kn->k) ? 0 : (mfma_ng == 1 ? (kn->k == 5 ? 5 : 0) : (kn->k == 9 ? 9 : 0)));
      const bool bnd = mfma_ad == 1 && c.ram_bnd;
      R.kfn = fmh::k_mfma_ad(kn->kind, mfma_ng, R.kx, bnd ? 1 : 0, mfma_ext == 1 ? 1 : 0);   // (mfma_ext == 1, short data: one resident slot)
    }
  } else if (pipe_opt) {
    R.form = lat_normal ? Form::LAT : Form::SPEC;
  }
}

// ---- the logistic family on the wave-specialised kernel (round 5; mh_spec.hpp, FAM = LOGISTIC): data in the compute lanes'
// registers, g table in LDS, the register owners.  The workflow vignette's own model (mcmc::logit: 100 observations, k = 5) ran
// on the general kernel at 2.6 / 5.9 us per step (kernel_normal / kernel_adapt).  Knob speclogit=0: off.
static void plan_logit_register(const Call& c, Route& R) {
  const fmcmc_model* m = c.m; const fmcmc_kernel* kn = c.kn; const Knobs& K = c.K;
  const int kf = c.kf, kz = c.kz;
  const bool lat_on = K.lat != 0 && K.speclogit != 2;
  // (a fixed parameter under the normal / uniform kernels: the latency form's candidate wave handles it, the owners of mh_sweep_spec do not)
  const bool lg_lat_fixed = c.normal_kind && c.joint && kf != kn->k && lat_on;
  // (8 .. 15 covariates, k <= 16, up to 2048 observations, the normal / uniform kernels: the latency form only -- four slots of P doubles
  //  per lane; they ran on the general kernel, 3 - 4.5 us per step at n = 200)
  const bool wide_p = m->p >= 8 && m->p <= 15 && kn->k <= PIPE_KMAX;
  const bool lg_lat_wide = wide_p && c.normal_kind && lat_on && kf >= 1 && (c.joint || c.single_lat);
  // (and under kernel_adapt / kernel_ram -- unbounded, stride 1, no fixed parameter --: mh_sweep_spec<P, 4, KIND, LOGISTIC> with the register
  //  owner at the compile-time width k <= 16; general kernel: 6 - 14 us per step at n = 200.  Knob specwide=0: off)
  const bool lg_spec_wide = wide_p && K.specwide != 0 && ((c.adapt && !c.adapt_hist) || (c.ram && !c.ram_bounded && !kn->constr));
  if (!(!c.force && K.pipe != 0 && K.speclogit != 0 && K.shard < 0 && c.logistic && !c.mirror && m->p >= 1 && (m->p <= 7 || lg_lat_wide || lg_spec_wide) &&
        kn->k == m->p + (m->intercept ? 1 : 0) && ((kf == kn->k && kz == kn->k) || c.single_lat || (lg_lat_fixed && kf >= 1)) &&
        ((c.normal_kind && (c.joint || c.single_lat)) || (c.adapt && (!c.adapt_hist || c.adapt_ring)) ||
         (c.ram && !kn->constr && (!c.ram_bounded || K.specbnd != 0))) &&
        offsets_fit(c, 1ll << 28))) return;
  if ((!c.joint || lg_lat_fixed || lg_lat_wide) && c.normal_kind) {
    // single-parameter schemes: the latency form's candidate wave, one to four chains per workgroup (as for the linear model)
    // (a fixed parameter: at most 12 slots)
    if (c.per_cu <= 4 && (m->p <= 7 || lg_lat_wide) && c.nsl2 <= (lg_lat_fixed && fmh::reg_slots(m->p) > 12 ? 12 : fmh::reg_slots(m->p))) {
      R.pipe_opt = (int)c.nsl2; R.form = Form::LAT_LOGIT;
      R.spec_cw = c.lat_forced ? K.lat : (int)c.per_cu;
    }
  } else if (c.nsl2 <= fmh::k_spec_optmax(m->p, kn->kind)) {
    R.pipe_opt = (int)c.nsl2; R.form = Form::SPEC_LOGIT;
    R.spec_cw = c.lat_forced ? K.lat : ((K.lat != 0 && c.per_cu <= 3) ? (int)c.per_cu : 4);
    // the normal / uniform kernels with fewer than four chains per CU: the latency form (mh_sweep_lat<.., LOGISTIC>: replicated decision)
    // (measured, tools/bench_small_logit.py and the pair of forms at 256 / 512 / 768 chains: the replicated decision wins up to ~3,000
    //  observations at any count -- 0.85 / 1.18 / 1.59 us against 1.25 / 1.34 / 1.78 at n = 1000 -- and up to ~6,000 with one chain
    //  per workgroup, 1.66 against 2.15 at n = 5000; beyond, the lookups' LDS time is the step and the owners' overlap pays:
    //  n = 10,000: 6.4 against 4.8 at 512 chains.  Knob speclogit=2: never.)
    if (R.spec_cw < 4 && K.speclogit != 2 && c.normal_kind && fmh::k_lat_logit(m->p, kn->kind) &&
        c.nsl2 <= (R.spec_cw == 1 ? 12 : 6)) R.form = Form::LAT_LOGIT;
  }
}

// ---- the commit check: a register form is kept only where its instantiation exists and holds the slot count (a launch with a
// slot count it does not hold would run no loop and hand back zeros -- round 5's soak found one such route); else the form below
static void commit_register_form(const Call& c, Route& R) {
  const int p = c.m->p, kind = c.kn->kind;
  R.ring = c.adapt_ring;
  if (R.form < Form::LAT || R.form > Form::SPEC_LOGIT) return;
  const void* h = (R.form == Form::LAT) ? fmh::k_lat(p, kind) : (R.form == Form::LAT_LOGIT) ? fmh::k_lat_logit(p, kind)
                : (R.form == Form::SPEC) ? (R.ring ? fmh::k_spec_ring(p, 0) : fmh::k_spec(p, kind))
                : (R.ring ? fmh::k_spec_ring(p, 1) : fmh::k_spec_logit(p, kind));
  if (!h || R.pipe_opt > fmh::reg_slots(p) || (R.pipe_opt & 1)) {
    if (c.K.mode) fprintf(stderr, "fmcmc_amd: slot count %d beyond the register kernels' %d at p = %d: general kernel\n", R.pipe_opt, h ? fmh::reg_slots(p) : 0, p);
    R.form = Form::GENERAL; R.pipe_opt = 0; R.spec_cw = 4;
  } else {
    R.kfn = h;
  }
}

// ---- the LONG-DATA form (mh_common.hpp, shard_long): few chains on long data.  Up to four chains are one workgroup of the
// chain-sharded kernels, i.e. ONE compute unit walks the whole data set per step (n = 1e5, p = 3: 34 us per step, 255 CUs idle);
// here all 256 workgroups evaluate their 1/256 of the observations for every chain and the canonical lane sums cross the chip as
// in the other observation-sharded forms.  Taken (R.kfn_long: tried first by the launcher) when est_long -- or knob shard=1 --
// says so.  kfn: its kernel; lds_base: its LDS bytes without the term block; est_now: what the call costs otherwise.
static void plan_long(const Call& c, Route& R, const void* kfn, size_t lds_base, double est_now, bool logistic) {
  const fmcmc_model* m = c.m; const fmcmc_run* run = c.run;
  if (c.force || c.K.shard == 0 || R.cw != 1 || c.ncu != 256 || run->nchains > 64 || m->n < 8 * NT || m->n >= (1ll << 31) || run->nsteps >= 30000000 ||
      c.ram_bnd || c.mirror) return;
  const long long room = ((long long)150 * 1024 - (long long)lds_base) / 8 - 2;
  const long long lrow = 2ll * shard_long_row((int)c.nsl) + SHL_BS;     // LDS doubles per chain of a group
  long long lcg = room / lrow;
  if (lcg > run->nchains) lcg = run->nchains;
  if (lcg < 1) return;
  if (!(c.K.shard == 1 || est_long(c, lcg, logistic) < 0.9 * est_now)) return;
  R.kfn_long = kfn; R.lcg = lcg; R.lrow = lrow;
  R.lds_long = lds_base + sizeof(double) * (size_t)(lcg * lrow + 2);
}
// (the linear model: one chain per workgroup, every proposal kernel.  Wide models, p >= 16: where the matrix-core slices end -- 96
//  observations per workgroup, n = 24,576 -- the chain-sharded kernel is what is left)
static void plan_linreg_long(const Call& c, Route& R) {
  const fmcmc_model* m = c.m;
  if (c.linreg && (m->p <= 15 || (m->p <= 62 && m->n > (long long)NT * 2 * SHM_T)))
    plan_long(c, R, fmh::k_wide(1, 2, c.kn->kind), R.lds, est_linreg_now(c), false);
}

// ---- the chain-sharded forms: what runs a call no fast form takes, and what a fast one steps down to

// The logistic-only instantiations: the g table in LDS; up to 28 / cw - 1 covariates their number is a compile-time constant
// of the evaluation loop and the coefficients of the CW chains live in SGPRs (mh_common.hpp, logit_partials), beyond that
// the run-time loop (logit_partials_any) -- still with the table in LDS, which is what the all-family kernel lacks
// (round 4: kernel_adapt / kernel_ram too -- the workflow vignette's own model is a logistic regression under kernel_adapt;
//  tools/option_audit.py found them on the all-family kernel at 3.9x the time per step of the normal kernels)
static bool plan_base_logistic(const Call& c, Route& R) {
  const fmcmc_model* m = c.m; const fmcmc_kernel* kn = c.kn; const fmcmc_run* run = c.run; const Knobs& K = c.K;
  if (!(!c.force && c.logistic && R.cw <= 4 && R.lds + sizeof(double) * (LG_LDS_DOUBLES + LG_LDS_TAIL) <= 160 * 1024 && !c.mirror)) return false;
  const bool fast = stream_fed(R.form);
  const int lkv = kn->kind, lcw = R.cw <= 2 ? R.cw : 4;   // 1 .. 4
  R.base = Form::LOGISTIC;
  R.kfn_base = fmh::k_logit(lcw, 0, lkv);
  R.lds += sizeof(double) * (LG_LDS_DOUBLES + LG_LDS_TAIL);   // the table staged behind the chain blocks (16-byte aligned), logit_shard's control words
  // few chains: the long-data form (shard_long<LOGISTIC>) -- the chain-sharded kernel walks the data set in one workgroup
  if (!fast && m->p >= 1 && m->p <= 16) plan_long(c, R, fmh::k_logit(1, 1, lkv), R.lds, est_logit_now(c), true);
  // Observation-sharded form (mh_common.hpp, logit_shard): 256 workgroups of two canonical lanes each evaluate ALL chains
  // of the launch, up to 256 x cw of them; more chains run as consecutive launches.  est_logit_chain against
  // est_logit_sharded; knob shard=1 forces it for every eligible shape (tests), shard=0 disables it.
  R.nb_launch = 256;
  R.ch_launch = (R.nblk > R.nb_launch) ? R.nb_launch * R.cw : (long long)run->nchains;
  // (for the normal / uniform kernels mh_sweep_logit2, the shadow form -- four chains per workgroup whatever cw says; knob shadow=0: off)
  const bool shadow_ok = K.shadow != 0 && c.normal_kind && c.joint && c.kf == kn->k;
  // (not the bounded kernel_ram: its second evaluation of a step runs only in the workgroups where a proposal was reflected
  //  -- the grid-wide evaluation needs every workgroup in every hand-over)
  const bool lshard = K.shard != 0 && m->p >= 1 && m->p <= 16 && c.ncu == 256 && m->n >= 2 * NT && m->n < (1ll << 28) && !c.ram_bnd &&
                      (K.shard == 1 || est_logit_sharded(c, R.nb_launch, R.ch_launch, shadow_ok) < 0.95 * est_logit_chain(c, R.cw, R.nblk));
  if (!lshard || fast) return true;
  R.form = Form::LOGISTIC_SHARDED;
  R.kfn = fmh::k_logit(lcw, 1, lkv);
  R.lds_run = R.lds;
  // (variates from a stream, the library's or the caller's: the instantiation without the generators in its body)
  R.kfn_fed = fmh::k_logit(lcw, 2, lkv);
  // (mh_sweep_logit2 holds four chains per workgroup whatever cw says)
  R.ch_shadow = (run->nchains < 4 * R.nb_launch) ? (long long)run->nchains : 4 * R.nb_launch;
  // the normal / uniform proposal kernels, joint scheme, no fixed parameter: mh_sweep_logit2 (mh_logit2.hpp) -- the owners' work in
  // the shadow of the hand-overs
  // (kernel_adapt / kernel_ram with up to eight parameters, none fixed, no window / constraint / bound: the same sweep with the
  //  register owner of mh_spec.hpp, mh_sweep_logit2a)
  const bool adaptive3 = (c.adapt && !c.adapt_hist) || (c.ram && !kn->constr && !c.ram_bounded);
  R.kfn_shadow = (K.shadow == 0 || c.kf != kn->k || c.kz != kn->k) ? nullptr
               : (c.normal_kind ? (c.joint ? fmh::k_logit2(lkv) : nullptr)
                  : ((adaptive3 && kn->k <= SPEC_KA && kn->k <= PIPE_KMAX) ? fmh::k_logit2a(lkv) : nullptr));
  if (R.kfn_shadow) R.lds_shadow = c.normal_kind ? fmh::k_logit2_lds(kn->k) : fmh::k_logit2a_lds();
  return true;
}

// Wide linear models (config C4: k = 50): one family and one proposal kernel compiled in, which leaves the streamed
// evaluation the registers for 4 observations x 8 columns in flight per thread (mh_common.hpp); observation-sharded in the
// sequential form (scalar / matrix-core slice product) or the dataflow form
static bool plan_base_wide(const Call& c, Route& R) {
  const fmcmc_model* m = c.m; const fmcmc_kernel* kn = c.kn; const fmcmc_run* run = c.run; const Knobs& K = c.K;
  if (!(c.linreg && m->p >= 16 && R.cw <= 2 && (c.ram || c.normal_kind))) return false;
  const int kv = kn->kind, nslots = (int)c.nsl, cw = R.cw;   // cw: 1 or 2
  R.base = Form::WIDE;
  R.kfn_base = fmh::k_wide(cw, 0, kv);
  // Observation-sharded evaluation: one cooperative launch when the call has 128 or 256 workgroups, consecutive launches
  // of 256 workgroups when it has a multiple of that (more than 512 chains per GPU at two chains per workgroup)
  // (a launch may hold workgroups WITHOUT chains -- they own canonical lanes like the others -- so any chain count works:
  //  up to 512 chains run as one launch of 256 workgroups, exactly 128 workgroups keep 4 lanes each when n allows)
  R.nb_launch = (R.nblk == 128 && 4 * nslots <= SH_MAXO) ? 128 : 256;
  R.ch_launch = (R.nblk > R.nb_launch) ? R.nb_launch * cw : (long long)run->nchains;
  // (two chains per workgroup BECAUSE the sharded sweep pays: no second verdict)
  const int lpw = wide_sharded_lanes(c, (R.wide_switched && K.shard != 0) ? 1 : K.shard, R.nb_launch, cw);
  bool shard = lpw > 0;
  if (K.mode & 256) fprintf(stderr, "fmcmc_amd: wide path nblk=%lld lpw=%d nslots=%d p=%d bounded=%d shard=%d\n", R.nblk, lpw, nslots, m->p, (int)c.ram_bounded, (int)shard);
  // the slice product on the matrix cores (shard_columns_mfma): the slice lives in LDS behind the chain blocks
  const SliceShape s = wide_slice_shape(c.nsl, lpw, m->p);
  // (three M-tiles of which the third holds values 8, 9 only, at the width with a compile-time K-block count -- config C4:
  //  its 8 rows go through two 4x4x4 MFMAs per K-block instead of a 16x16x4 that is half padding; knob t10=0: off)
  //  (the form reads values 0 .. SHM_T10_FULL - 1 of every lane group without a mask: slots spg h + t <= nslots - 2 are full)
  const bool t10_full = shard && s.spg * (4 / lpw - 1) + (SHM_T10_FULL - 1) <= nslots - 2;
  R.t10 = (s.nmt == 3 && s.spg <= 10 && (m->p + 3) / 4 == 12 && t10_full && K.t10 != 0) ? 1 : 0;
  R.mfma_form = shard && shard_mfma_enabled(K) && m->p <= 4 * SHM_KBMAX && s.spg <= SHM_T &&
                R.lds + sizeof(double) * (size_t)(s.mblk + 1) <= 160 * 1024;
  if (shard && !R.mfma_form && lpw * nslots > SH_MAXO) shard = false;      // (more than 40 observations per slice: the matrix-core form or none)
  // the dataflow form (mh_wide2.hpp): owner and evaluator waves decoupled, two chain groups half a step out of phase.
  // It pays where the owners have real work to hide -- kernel_ram: 35.8 -> 27.9 us per step at C4 -- and costs the normal
  // kernels 6 % (26.2 against 24.6: their owner phase is short and two of eight waves no longer evaluate).
  // Knob wide2=0 keeps the sequential form everywhere, wide2=1 takes the dataflow form for every eligible call (tests).
  const bool w2on = K.wide2 == 1 || (K.wide2 != 0 && c.ram);
  R.wide2 = shard && R.mfma_form && w2on && lpw == 2 && cw == 2 && R.nb_launch == 256 && c.ncu == 256 &&
            !(c.ram && kn->constr) && (c.ram || c.joint) &&
            s.nmt >= 1 && s.nmt <= 3 && run->nsteps < 100000000 &&
            sizeof(double) * wide2_lds_doubles(kn->k, c.kf, kn->kind, c.kz, s.mblk) <= 160 * 1024;
  R.lpw = lpw; R.nmt = s.nmt; R.mblk = s.mblk;
  if (stream_fed(R.form)) {
  } else if (R.wide2) {
    R.form = Form::WIDE_DATAFLOW;
    R.kfn = fmh::k_wide2(kv, s.nmt);
    R.lds_run = sizeof(double) * wide2_lds_doubles(kn->k, c.kf, kn->kind, c.kz, s.mblk);
    R.ngrp = (K.groups == 4) ? 4 : 2;
    R.tiles = (K.tiles == 0 || R.ngrp == 4) ? 0 : 1;
  } else if (shard) {
    // the sharded evaluation is its own instantiation (OPT = lanes per workgroup): sharing one with the streamed loop
    // cost 200-300 spilled registers in BOTH paths
    R.form = R.mfma_form ? Form::WIDE_SHARDED_MFMA : Form::WIDE_SHARDED;
    R.kfn = fmh::k_wide(cw, lpw, kv);
    R.lds_run = R.lds + (R.mfma_form ? sizeof(double) * (size_t)(s.mblk + 1) : 0);
  }
  return true;
}

// The route of a call: what it decides can only be stepped down at run time, to R.base (a refused cooperative launch, an
// operand stream the device cannot give).
static Route plan_route(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run, int kf, int ram_bounded, int kz, long long ldS,
                        int ncu, const Knobs& K) {
  const Call c = make_call(m, kn, run, kf, ram_bounded, kz, ldS, ncu, K);
  Route R;
  if (plan_bigk(c, R)) return R;
  if (!plan_chain_blocks(c, R)) return R;
  plan_linreg_stream_fed(c, R);
  plan_logit_register(c, R);
  commit_register_form(c, R);
  // step windows: the stream-fed forms with the library's own stream (the mirror kernels materialise theirs whole)
  if (stream_fed(R.form) && c.philox && !c.mirror) R.win = step_window(run, kz, K);
  plan_linreg_long(c, R);
  if (R.res_p >= 0) { R.base = Form::RESIDENT; R.kfn_base = fmh::k_resident(R.res_p, kn->kind); }
  else if (!plan_base_logistic(c, R) && !plan_base_wide(c, R)) { R.base = Form::GENERAL; R.kfn_base = fmh::k_general(R.cw); }
  if (R.form == Form::GENERAL) { R.form = R.base; R.kfn = R.kfn_base; }   // (no fast or sharded form)
  return R;
}
