// mh_route.hpp -- the route of a call: which kernel runs it, and in which shape.  plan_route() is a pure function of the
// normalised call, the compute units and the FMCMC_AMD_DEBUG knobs (no HIP call, no allocation); launch_sweep (mh_engine.hip)
// launches what it returns and only steps down from it at run time.  Capacities of the instantiations: mh_kernels.hpp.
// Host code, included by mh_engine.hip behind the kernel headers whose shape helpers it uses.
#pragma once

// LDS bytes of the chain-sharded kernels (mh_streamed.hpp): CW chains per workgroup, tb rows of the sample tile
static size_t sweep_lds_bytes(int k, int kf, int kind, int CW, int tb, int kz, bool resident) {
  size_t d = 5 * (size_t)k + (k / 2 + 1) + (size_t)NW * CW + 1 + (size_t)CW * tb * (kz + 1) + (size_t)CW * k +
             (resident ? (size_t)CW * NT : 0) + (size_t)CW * chain_lds_doubles(k, kf, kind);
  return d * sizeof(double);
}

// Observation-sharded evaluation (mh_common.hpp, eval_sharded): `nb` workgroups per launch must split the 512 canonical
// lanes evenly (128 or 256 of them), be co-resident (cooperative launch) and hold their slice in SH_MAXO registers.
// Returns the canonical lanes per workgroup (2 or 4), or 0 when the shape is not eligible or the cost model prefers the
// chain-sharded kernel.  Cost model (us per step, fitted at k = 50): chain-sharded ~4 + X bytes / 65 GB/s (the per-CU L2
// rate); sharded ~14 of hand-overs and fixed work + 0.0085 per column and walked observation slot (+ ~6 of barrier
// imbalance under kernel_ram): n = 2500 loses (23.9 vs 19.1), n = 5000 wins (24.3 vs 30.1), C4 wins 2x.
// Knob shard=1 (FMCMC_AMD_DEBUG) forces the sharded kernel for every eligible shape (tests), shard=0 disables it.
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
struct Knobs {
  int streamed = -1, cw = -1, pipe = -1, lat = -1, mfma = -1, shard = -1, shard_mfma = -1, wide2 = -1, groups = -1, tiles = -1, t10 = -1, window = -1, mode = 0;
  int shadow = -1, turn = -1, speclogit = -1, specbnd = -1, specmirror = -1, specp0 = -1, tinymfma = -1, specwide = -1;
  int bigkhbm = -1;
};
static Knobs read_knobs() {
  Knobs K;
  const char* e = getenv("FMCMC_AMD_DEBUG");
  if (!e) return K;
  struct { const char* name; int* dst; } tab[] = {{"streamed", &K.streamed}, {"cw", &K.cw}, {"pipe", &K.pipe}, {"lat", &K.lat},
      {"mfma", &K.mfma}, {"shard_mfma", &K.shard_mfma}, {"shard", &K.shard}, {"wide2", &K.wide2}, {"groups", &K.groups}, {"tiles", &K.tiles}, {"t10", &K.t10}, {"window", &K.window}, {"mode", &K.mode}, {"shadow", &K.shadow}, {"turn", &K.turn}, {"speclogit", &K.speclogit}, {"specbnd", &K.specbnd}, {"specmirror", &K.specmirror}, {"specp0", &K.specp0}, {"tinymfma", &K.tinymfma}, {"specwide", &K.specwide}, {"bigkhbm", &K.bigkhbm}};
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
static bool shard_mfma_enabled(const Knobs& K) { return K.shard_mfma != 0; }
static int wide_sharded_lanes(const Knobs& K, const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run, int ram_bounded, int ncu, long long nb,
                              int cw_now = 2 /* chains per workgroup the call would run with on the chain-sharded / general kernel */) {
  if (K.shard == 0) return 0;
  if (m->family != FMCMC_FAM_GAUSSIAN_LINREG || m->p < 16) return 0;
  if (kn->kind != FMCMC_KERNEL_RAM && kn->kind != FMCMC_KERNEL_NORMAL && kn->kind != FMCMC_KERNEL_NORMAL_REFLECTIVE) return 0;
  const int nslots = (int)((m->n + NT - 1) / NT);
  const int lpw = (nb == 128 || nb == 256) ? (int)(NT / nb) : 0;
  const long long per_launch = nb * 2;   // (upper bound of the chains of one launch: at most two per workgroup)
  // A slice of more than 49 columns (15.5 KB) no longer stays in the scalar cache: 2.1x per walked slot, still ahead for the
  // normal kernels (k = 64, n = 10k: 57 us per step against 78); kernel_ram stays chain-sharded there, its owner phase
  // dominates at that width and runs slower in the sharded instantiation (121 against 108).
  const bool cached = shard_mfma_enabled(K) || (size_t)m->p * SH_MAXO * sizeof(double) <= 15872;   // (the MFMA form keeps the slice in LDS)
  // (a slice holds up to SH_MAXO = 40 observations in the scalar / register form, up to 4 SHM_T = 96 -- six M-tiles -- in LDS for the
  //  matrix-core form: n <= 24,576 at 256 workgroups)
  const bool mf_ok = shard_mfma_enabled(K) && m->p <= 4 * SHM_KBMAX;
  const bool ok = lpw > 0 && !(kn->kind == FMCMC_KERNEL_RAM && (ram_bounded || !cached)) && lpw * nslots <= (mf_ok ? 4 * SHM_T : SH_MAXO) && nb <= ncu &&
                  (long long)m->p * SH_MAXO * nb < (1ll << 28) && (long long)(m->p + 1) * (per_launch + SH_PAD) < (1ll << 31) &&
                  run->nsteps < 30000000;   /* barrier epochs (2 per step) x workgroups per group stay below 2^32 */
  if (!ok) return 0;
  if (K.shard != 1) {
    // us per step, refitted to tools/dispatch_audit.py (profiles/r04_dispatch_audit.md: p = 16 .. 60, n = 1e3 .. 1e4, 64 .. 2048
    // chains): the chain-sharded kernel streams the data set per workgroup and pays kernel_ram's owner phase (~0.15 us per
    // parameter) in the open; the sharded forms cost ~9 us of hand-overs plus a slice product that grows with the chains of a
    // launch -- on the matrix cores p (0.08 + 0.00475 slice observations) per 512 chains -- and hide the RAM owners in the
    // dataflow form (more than 256 chains), pay ~0.17 us per parameter in the sequential one
    const bool ram = kn->kind == FMCMC_KERNEL_RAM;
    // (with four / eight chains per workgroup -- more than 512 / 1024 chains -- the data stream is shared by more chains but a
    //  step takes 1.3x / 2.4x as long (and the owners of a workgroup queue), and the workgroups run in rounds; the sharded sweep runs as consecutive launches)
    const double rounds = (double)((run->nchains + (long long)cw_now * ncu - 1) / ((long long)cw_now * ncu));
    const double launches = (double)((run->nchains + per_launch - 1) / per_launch);
    const double est_chain = (4.0 + (double)m->n * (double)m->p * 8.0 / 65000.0 * (cw_now >= 8 ? 2.4 : (cw_now == 4 ? 1.3 : 1.0)) +
                              (ram ? (cw_now <= 2 ? 0.12 : 0.075 * (double)cw_now) * (double)kn->k : 0.0)) * rounds;
    const double frac = (double)(run->nchains < per_launch ? run->nchains : per_launch) / 512.0;
    double est_shard;
    if (shard_mfma_enabled(K) && m->p <= 4 * SHM_KBMAX) {
      // (more than three M-tiles: the run-time K-block loop, +5 us; kernel_ram's owners are hidden by the dataflow form only -- more
      //  than 256 chains, at most three M-tiles --, else ~0.17 us per parameter for few chains, ~0.3 in full launches)
      const bool tall = lpw * nslots > SH_MAXO;
      // (round 5: the dataflow form for 256 chains and fewer too -- two chains per workgroup, half of the workgroups without chains:
      //  C4's shape at 256 / 128 / 64 chains 15.0 / 14.7 / 12.7 us per step against 20.6 / 18.0 / 17.1 on the sequential form)
      const bool hidden = ram && !tall && !kn->constr && K.wide2 != 0 && (run->nchains > 256 || cw_now == 2);
      // (refitted once more after the compile-time K-block counts of every width: ~10 of hand-overs, 0.4 + p (0.083 + 0.004 slice observations) per 512
      //  chains at up to three M-tiles; the dataflow form's kernel_ram runs ~2 us UNDER the normal kernels' sequential form)
      const bool tall_rt = tall && (m->p + 3) / 4 > 12;     // (tall slices beyond 12 K-blocks keep the run-time loop: ~5 us more)
      est_shard = 10.2 + (tall_rt ? 5.0 : 0.0) + frac * ((tall ? 0.6 : 0.4) + (double)m->p * ((tall ? 0.08 : 0.083) + (tall ? 0.00475 : 0.004) * (double)(lpw * nslots))) +
                  ((ram && !hidden) ? (run->nchains <= 256 ? 0.17 : 0.3) * (double)kn->k : 0.0);
      if (hidden) {   // (what the dataflow form hides is at most a quarter of its slice product)
        const double prod = frac * (0.4 + (double)m->p * (0.083 + 0.004 * (double)(lpw * nslots)));
        est_shard -= (prod * 0.25 < 2.0 * frac) ? prod * 0.25 : 2.0 * frac;
      }
    }
    else {
      const double walked = (cached ? 1.0 : 2.1) * ((lpw * nslots <= SH_MAXO / 2) ? SH_MAXO / 2 : SH_MAXO);
      est_shard = 14.0 + 0.0085 * (double)m->p * walked + (ram ? 6.0 : 0.0);
    }
    if (!(est_shard * launches < 0.95 * est_chain)) return 0;
  }
  return lpw;
}

// Step windows of the stream-fed kernels (library's own stream): ~256 MiB of stream per window, from 32 steps, a multiple of 32
// (knob window=N).  The ring of kernel_adapt(freq > 1) on mh_sweep_spec is only correct for a call that is one window.
static long long step_window(const fmcmc_run* run, int kz, const Knobs& K) {
  const long long per_step = (long long)run->nchains * (kz + 1) * 8;
  long long win = ((256ll << 20) / (per_step > 0 ? per_step : 1)) & ~31ll;
  if (win < 32) win = 32;     // (the kernels take windows from 32 steps; a 512-step floor let the buffer grow with nchains without bound)
  if (K.window >= 32) win = (long long)K.window & ~31ll;      // (diagnosis / tests: a window length)
  return win;
}

// ---- the route of a call: which kernel runs it, and in which shape (DESIGN.md section 5 has the table) ------------------------
// (one per kernel family and form; kernel_name: what fmcmc_last_kernel() reports for it)
enum class Form { BIGK, RESIDENT, GENERAL, LONG, MFMA, MFMA_STREAMED, MFMA_ADAPTIVE, LAT, LAT_LOGIT, SPEC, SPEC_LOGIT,
                  LOGISTIC, LOGISTIC_SHARDED, LOGISTIC_SHADOW, WIDE, WIDE_SHARDED, WIDE_SHARDED_MFMA, WIDE_DATAFLOW, BIGK_HBM };
struct Route {
  Form form = Form::GENERAL;   // what runs the call
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
  const int c = (R.spec_cw >= 1 && R.spec_cw <= 3) ? R.spec_cw - 1 : 3;
  if (R.form >= Form::LAT && R.form <= Form::SPEC_LOGIT) return by_cw[(int)R.form - (int)Form::LAT][c];
  return name[(int)R.form];
}

// The route of a normalised call (iid Normal as the linear model without covariate, the uniform kernels as the normal ones):
// a pure function of the call's shape, the compute units and the knobs -- no HIP call, no allocation.  What it decides can only
// be stepped down at run time, to R.base (a refused cooperative launch, an operand stream the device cannot give).
static Route plan_route(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run, int kf, int ram_bounded, int kz, long long ldS,
                        int ncu, const Knobs& K) {
  Route R;
  // more parameters than a wavefront has lanes: one workgroup per chain (mh_bigk.hpp); fmcmc_validate has refused what it lacks.
  // Its matrices in LDS wherever they fit (every k <= 128; kernel_adapt up to 133, kernel_ram up to 183 free parameters),
  // in the chain's own Sigma square in HBM beyond (knob bigkhbm=1: always)
  if (kn->k > FMCMC_MAX_K_WAVE) {
    const size_t lds = sizeof(double) * bigk_lds_doubles(kn->k, kf, kn->kind);
    const bool hbm = K.bigkhbm == 1 || lds > 160 * 1024;
    R.form = R.base = hbm ? Form::BIGK_HBM : Form::BIGK;
    R.kfn = R.kfn_base = fmh::k_bigk(hbm ? 1 : 0);
    R.lds = hbm ? sizeof(double) * bigk_lds_doubles(kn->k, kf, kn->kind, true) : lds;
    R.lds_exceeded = R.lds > 160 * 1024;
    R.no_kernel = R.kfn == nullptr;
    return R;
  }
  const bool mirror = (kn->kind == FMCMC_KERNEL_NMIRROR || kn->kind == FMCMC_KERNEL_UMIRROR);
  const bool adapt_hist = (kn->kind == FMCMC_KERNEL_ADAPT && (kn->bw > 0 || kn->freq > 1));
  const long long nsl = (m->n + NT - 1) / NT, nsl2 = (nsl + 1) & ~1ll;   // observation slots of 512, rounded up to even
  const long long per_cu = (run->nchains + ncu - 1) / ncu;
  const bool lat_forced = K.lat >= 1 && K.lat <= 3;
  // register-resident variant: Gaussian linreg whose data fits the VGPR budget of 512 threads
  const bool force = K.streamed == 1;
  if (!force && m->family == FMCMC_FAM_GAUSSIAN_LINREG && !mirror) {
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
    while (cw < NW && (long long)cw * ncu < run->nchains) cw <<= 1;
    if (K.cw == 1 || K.cw == 2 || K.cw == 4 || K.cw == 8) cw = K.cw;   // diagnosis: chains per workgroup of the streamed kernel
    // wide linear models with more than two chains per CU: two chains per workgroup, so that the sweep can run as
    // consecutive observation-sharded launches of 2 x CUs chains each (below) when that pays off
    // (measured at k = 50, n = 10k: 1024 chains 63.8 us per step instead of 71.6 with four chains per workgroup; at 2048
    //  chains the general kernel with eight chains per workgroup is level, 123 vs 128, and keeps the sweep)
    else if (cw >= 4 && wide_sharded_lanes(K, m, kn, run, ram_bounded, ncu, (long long)ncu, cw) > 0) { cw = 2; R.wide_switched = true; }
    // kernel_ram on a wide model with ONE chain per CU or fewer: two per workgroup all the same, so that the sweep is eligible for the
    // dataflow form (mh_wide2.hpp: two chain groups half a step out of phase; workgroups without chains evaluate like the others)
    else if (cw == 1 && ncu == 256 && K.wide2 != 0 && m->family == FMCMC_FAM_GAUSSIAN_LINREG && m->p >= 16 && m->p <= 4 * SHM_KBMAX &&
             kn->kind == FMCMC_KERNEL_RAM && !ram_bounded && !kn->constr && shard_mfma_enabled(K) &&
             2 * nsl <= SH_MAXO && run->nchains >= 2 &&
             !((run->nchains + 1) / 2 == 128 && 4 * nsl <= SH_MAXO) &&      /* (exactly 128 workgroups of four lanes: the sequential form's own shape) */
             nsl >= 6 &&      /* (short data: the chain-sharded sweep is ahead -- p = 30, n = 1000, 64 chains: 9.7 against 11.6 us) */
             [&]() {                           /* (the dataflow form's LDS: two owners' factor and partial sums + the slice block -- k = 62 does not fit) */
               const int spg = (int)(nsl + 1) / 2, nmt_ = (spg + 3) / 4;
               const int mblk_ = shm_hdr(nmt_) + nmt_ * ((m->p + 3) / 4) * 64;
               return nmt_ >= 1 && nmt_ <= 3 && sizeof(double) * wide2_lds_doubles(kn->k, kf, kn->kind, kz, mblk_) <= 160 * 1024;
             }() &&
             wide_sharded_lanes(K, m, kn, run, ram_bounded, ncu, (long long)ncu, 2) > 0) { cw = 2; R.wide_switched = true; }
    // the logistic-only instantiations (table in LDS; observation-sharded form) exist for up to four chains per workgroup: more
    // than 1024 chains run as more workgroups / consecutive sharded launches there, not on the all-family kernel with eight
    // chains per workgroup (tools/dispatch_audit.py: 4096 chains, n = 1e5, p = 5 took 1244 us per step, 4.7x four launches)
    else if (cw > 4 && m->family == FMCMC_FAM_LOGISTIC && kn->kind >= FMCMC_KERNEL_NORMAL && kn->kind <= FMCMC_KERNEL_RAM) cw = 4;
  }
  int tb = 32;
  while (tb > 1 && sweep_lds_bytes(kn->k, kf, kn->kind, cw, tb, kz, resident) > 60 * 1024) tb >>= 1;
  while (cw > 1 && !resident && sweep_lds_bytes(kn->k, kf, kn->kind, cw, tb, kz, resident) > 150 * 1024) cw >>= 1;
  R.cw = cw; R.tb = tb;
  R.lds = sweep_lds_bytes(kn->k, kf, kn->kind, cw, tb, kz, resident);
  if (R.lds > 160 * 1024) { R.lds_exceeded = true; return R; }
  R.nblk = (run->nchains + cw - 1) / cw;
  R.ch_launch = run->nchains;

  // ---- the stream-fed forms: mh_sweep_mfma (fp64-MFMA), mh_sweep_mfma_ad, mh_sweep_spec, mh_sweep_lat
  int pipe_opt = 0, mfma_ng = 0, mfma_ad = 0, mfma_ext = 0, spec_cw = 4;
  bool lat_normal = false, spec_logit = false;   // the latency form (mh_sweep_lat); the logistic instantiations
  // kernel_adapt(freq = 2 .. 8, bw = 0) on the register owner of mh_sweep_spec (round 5: the last `freq` rows of a chain in an LDS ring;
  // tools/option_audit.py had it on the general kernel at 14.7 us per step where freq = 1 takes 3.3): no fixed parameter, k <= 8, and a
  // call that is ONE step window (the ring does not travel between windows)
  const bool adapt_ring = kn->kind == FMCMC_KERNEL_ADAPT && kn->bw == 0 && kn->freq >= 2 && kn->freq <= SPEC_FREQMAX && kf == kn->k && kz == kn->k &&
                          kn->k <= SPEC_KA && (run->nsteps <= step_window(run, kz, K) + 1 || run->rng_mode != FMCMC_RNG_PHILOX);
  // single-parameter schemes of the normal / uniform kernels ("ordered", an explicit sequence, "random"): on mh_sweep_lat's candidate
  // wave (round 5: they ran on the general kernel, 2.9 us per step at the README's size where the joint scheme takes 0.63), one to FOUR
  // chains per workgroup; "random" draws its plan in the kernel and hands it back (a caller-fed plan stays general)
  const bool single_lat = (kn->kind == FMCMC_KERNEL_NORMAL || kn->kind == FMCMC_KERNEL_NORMAL_REFLECTIVE) && kn->scheme != FMCMC_SCHEME_JOINT &&
                          K.lat != 0 && (kn->scheme != FMCMC_SCHEME_RANDOM || run->rng_mode == FMCMC_RNG_PHILOX);
  // (round 5: no covariate at all -- the iid Normal family, intercept + sigma -- too: the compute lanes then hold no x)
  const bool spec_p_ok = m->p >= 1 || (m->p == 0 && m->intercept && K.specp0 != 0);
  // (round 5: 8 .. 14 covariates on up to 2048 observations -- four slots of P doubles per compute lane, the register owner at the
  //  compile-time width k <= 16; knob specwide=0: the streamed MFMA evaluation with the owners in LDS, as before)
  const bool spec_wide_ok = m->p <= 14 && K.specwide != 0;
  if (!force && K.pipe != 0 && m->family == FMCMC_FAM_GAUSSIAN_LINREG &&
      (kn->kind == FMCMC_KERNEL_NORMAL || kn->kind == FMCMC_KERNEL_NORMAL_REFLECTIVE ||
       ((kn->kind == FMCMC_KERNEL_ADAPT && (!adapt_hist || adapt_ring)) || (kn->kind == FMCMC_KERNEL_RAM && !kn->constr)) ||
       (mirror && kn->scheme == FMCMC_SCHEME_JOINT && kf == kn->k && K.mfma != 0)) &&
      (kn->scheme == FMCMC_SCHEME_JOINT || kn->kind == FMCMC_KERNEL_ADAPT || kn->kind == FMCMC_KERNEL_RAM || single_lat) && kn->k <= PIPE_KMAX &&
      // Sizes (round 3: rows and variates are addressed as 64-bit chain base + 32-bit offset, and a long call runs as step
      // windows with a bounded stream, so a call no longer leaves these kernels at 4 GiB of samples or stream).  What is
      // left: offsets inside one chain's blocks are 32 bits.
      (unsigned long long)run->nsteps * (unsigned long long)kz * 8ull < (1ull << 32) && run->nsteps < (1ll << 30) &&
      (unsigned long long)kn->k * (unsigned long long)ldS * 8ull < (1ull << 32) &&      /* 32-bit offsets inside ONE chain's block */
      /* (round 5: kernel_adapt / kernel_ram run in step windows too -- their step-dependent rules read the CALL's step, see below;
          what still materialises its whole stream, kept below 8 GiB: host-fed variates are the caller's, and the mirror kernels) */
      (!mirror || (unsigned long long)run->nchains * (unsigned long long)run->nsteps * (unsigned long long)(kz + 1) * 8ull < (8ull << 30))) {
    // the wave-specialised kernel (mh_sweep_spec): x of a compute lane in VGPRs, the slot count an (even) run-time choice among
    // its compute loops, up to reg_slots(p)
    {
      // (the bounded kernel_ram decides on f of the REFLECTED proposal: a second evaluation in the steps in which the reflection
      //  moved something -- the barrier-synchronised owners of mh_sweep_mfma_ad ask for it between barriers, this kernel's register
      //  owners through a second evaluation slot per step (round 5, SpecSyncB: k <= 8, no fixed parameter; knob specbnd=0: off))
      const bool bnd_ok = K.specbnd != 0 && kf == kn->k && (kn->k <= SPEC_KA || (kn->k == 9 && m->p == 7)) && kz == kn->k && !kn->constr;   // (k = 9: the compile-time owner of p = 7)
      if (spec_p_ok && (m->p <= 7 || spec_wide_ok) && nsl2 <= fmh::reg_slots(m->p) && (kn->kind == FMCMC_KERNEL_ADAPT || kn->kind == FMCMC_KERNEL_RAM) && (!(kn->kind == FMCMC_KERNEL_RAM && ram_bounded) || bnd_ok)) pipe_opt = (int)nsl2;
      // (normal / uniform kernels run on the MFMA kernel; knob mfma=0 keeps them here for the two shapes they were tuned at)
      if (m->p == 3 && nsl == 20 && kn->kind < FMCMC_KERNEL_ADAPT && kn->scheme == FMCMC_SCHEME_JOINT) pipe_opt = 20;
      if (m->p == 1 && nsl == 2 && kn->kind < FMCMC_KERNEL_ADAPT && kn->scheme == FMCMC_SCHEME_JOINT) pipe_opt = 2;
    }
    // (round 5: the streamed forms from ONE observation on -- up to 512 the one resident slot is the last, nothing is streamed; models with
    //  8 .. 15 covariates on small data ran on the general kernel, 2.4 - 5 / 9 - 26 us per step.  Knob tinymfma=0: from 513 on, as before)
    const long long nt_min = (K.tinymfma != 0) ? 0 : (long long)NT;
    const int ng_p = (m->p <= 3) ? 1 : (m->p <= 7 ? 2 : (m->p <= 11 ? 3 : 4));   // operand groups per observation slot
    const int nsr_p = (ng_p == 1) ? MfmaAdShape<1>::NSR : (ng_p == 2 ? MfmaAdShape<2>::NSR : MfmaAdShape<3>::NSR);
    // fp64-MFMA evaluation: general in n and p up to what 80 operand registers per lane hold (normal / uniform kernels)
    if (K.mfma != 0 && kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE && kn->scheme == FMCMC_SCHEME_JOINT) {
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
    // (mfma_ad == 2: the owners with their matrices in LDS -- 8 .. 15 covariates, or a fixed parameter; not the bounded kernel_ram)
    if (K.mfma != 0 && !pipe_opt && !adapt_hist && (kn->kind == FMCMC_KERNEL_ADAPT || kn->kind == FMCMC_KERNEL_RAM) && m->p >= 0 && m->p <= 15 && m->n < (1ll << 29)) {   // (p = 0: iid Normal)
      // (round 5: the run-time-width register owner takes fixed parameters -- free ones first, the fixed ones as passengers)
      const bool reg_owner = m->p <= 7 && kz == kf && kf >= 1 && ((kf == kn->k && (kn->k <= SPEC_KA || kn->k == 9)) || (kf < kn->k && kn->k <= SPEC_KA));
      if (m->n > (long long)NT * nsr_p && (reg_owner || !(kn->kind == FMCMC_KERNEL_RAM && ram_bounded))) {   // (its resident slots are all full)
        mfma_ad = reg_owner ? 1 : 2;
        mfma_ng = ng_p;
        mfma_ext = nsr_p;
      } else if (m->n > nt_min && ((reg_owner && ((kn->kind == FMCMC_KERNEL_RAM && ram_bounded) || m->p == 0)) || (!reg_owner && !(kn->kind == FMCMC_KERNEL_RAM && ram_bounded) && run->nchains <= 2048 /* (beyond: level with the general kernel at eight chains per workgroup) */))) {
        // short data (one slot resident, the rest streamed) for what the wave-specialised kernel does not take: the bounded
        // kernel_ram, 8 .. 15 covariates, no covariate at all (iid Normal)
        mfma_ad = reg_owner ? 1 : 2;
        mfma_ng = ng_p;
        mfma_ext = 1;
      }
    }
    if (kn->kind == FMCMC_KERNEL_RAM && ram_bounded && !mfma_ad && !pipe_opt) mfma_ng = 0;   // (general kernel)
    // the mirror kernels (joint scheme, no fixed parameter): their owner between the barriers of the same streamed MFMA evaluation
    if (mirror) {
      pipe_opt = 0; mfma_ng = 0;
      // (round 5: within mh_sweep_spec's registers their owner runs there -- beside the evaluation instead of between barriers, and in
      //  the latency forms; up to 512 observations they ran on the general kernel.  Knob specmirror=0: off)
      if (K.specmirror != 0 && spec_p_ok && (m->p <= 7 || spec_wide_ok) && nsl2 <= fmh::k_spec_optmax(m->p, kn->kind)) pipe_opt = (int)nsl2;
      else
      if (m->p <= 15 && m->n > nt_min && m->n < (1ll << 29)) { mfma_ad = 3; mfma_ng = ng_p; mfma_ext = (m->n > (long long)NT * nsr_p) ? nsr_p : 1; }
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
    const bool wide_lat = K.lat != 0 && K.specwide != 0 && !mirror && m->p >= 8 && m->p <= 15 && kn->k <= PIPE_KMAX && nsl2 <= fmh::reg_slots(m->p) &&
                          kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE && kn->kind >= FMCMC_KERNEL_NORMAL && kf >= 1;
    if (wide_lat && kn->scheme == FMCMC_SCHEME_JOINT && (per_cu <= 1 || lat_forced)) {
      pipe_opt = (int)nsl2; mfma_ng = 0; mfma_ext = 0; lat_normal = true;
      spec_cw = lat_forced ? K.lat : 1;
    } else
    if (single_lat && !mirror) {
      if (per_cu <= 4 && m->p >= 0 && (m->p <= 7 ? nsl2 <= fmh::k_spec_optmax(m->p, kn->kind) : wide_lat)) {
        pipe_opt = (int)nsl2; mfma_ng = 0; lat_normal = true;
        spec_cw = lat_forced ? K.lat : (int)per_cu;
      }
    } else
    if (K.lat != 0 && (!mirror || pipe_opt) && (pipe_opt || (mfma_ng && !mfma_ext && !mfma_ad))) {
      // kernel_adapt / kernel_ram (mh_sweep_spec) gain up to 25 % with one chain per workgroup, 18 % with two, 6 % with three at
      // n = 10,000 and are level at small n -- their step is the owner's dependent chain --: one to three, always.  The normal
      // kernels by a cost model (us per step, fitted to tools/bench_lat_grid.sh and `tools/dispatch_audit.py --only=few`,
      // profiles/r05_dispatch_audit_few.md): mh_sweep_lat costs ~0.45 us of fold, barrier and decision plus, per chain of the
      // workgroup, its evaluation (n (p + 2) fp64 instructions at ~4.7 cycles over four SIMDs; shorter lanes of p >= 4 run
      // at a lower rate) or -- short data -- its coefficient broadcast and tree; the MFMA kernel's four chains cost ~0.8 us
      // + 0.06 us per operand group and observation slot.  n = 10,000, p = 3: 1.03 | 1.62 | 2.15 us with 1 | 2 | 3 chains
      // against 2.0; p = 1: three chains still win (1.54 against 2.07); p = 7, n = 1000: two lose (1.22 against 1.13).
      int lcw_auto = 4;
      if (per_cu <= 3) {
        if (kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE) {
          const double w = (double)m->n * (double)(m->p + 2), rate = (m->p <= 3) ? 9.2e-6 : 1.25e-5;
          const double per_chain = (0.10 + rate * w > 0.18 + 0.025 * (double)m->p) ? 0.10 + rate * w : 0.18 + 0.025 * (double)m->p;
          const double t_lat = 0.45 + (double)per_cu * per_chain;
          const double ns = (double)nsl, ng = (m->p <= 3) ? 1.0 : 2.0;
          const double t_floor = 0.98 + 0.10 * (ng - 1.0);
          const double t_mfma = (0.80 + 0.06 * ng * ns > t_floor) ? 0.80 + 0.06 * ng * ns : t_floor;
          if (t_lat < t_mfma) lcw_auto = (int)per_cu;
        } else {
          lcw_auto = (int)per_cu;
        }
      }
      const int lcw = lat_forced ? K.lat : lcw_auto;
      // (p = 0 -- the iid Normal family -- included: the compute lanes then hold no x)
      if (lcw < 4 && nsl2 <= fmh::k_spec_optmax(m->p, kn->kind)) {
        if (kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE) { pipe_opt = (int)nsl2; mfma_ng = 0; lat_normal = true; }
        if (pipe_opt && !mfma_ng) spec_cw = lcw;
      }
    }
  }
  // ---- the logistic family on the wave-specialised kernel (round 5; mh_spec.hpp, FAM = LOGISTIC): data in the compute lanes'
  // registers, g table in LDS, the register owners.  The workflow vignette's own model (mcmc::logit: 100 observations, k = 5) ran
  // on the general kernel at 2.6 / 5.9 us per step (kernel_normal / kernel_adapt).  Knob speclogit=0: off.
  // (a fixed parameter under the normal / uniform kernels: the latency form's candidate wave handles it, the owners of mh_sweep_spec do not)
  const bool lg_lat_fixed = kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE && kn->kind >= FMCMC_KERNEL_NORMAL && kn->scheme == FMCMC_SCHEME_JOINT &&
                            kf != kn->k && K.lat != 0 && K.speclogit != 2;
  // (8 .. 15 covariates, k <= 16, up to 2048 observations, the normal / uniform kernels: the latency form only -- four slots of P doubles
  //  per lane; they ran on the general kernel, 3 - 4.5 us per step at n = 200)
  const bool lg_lat_wide = m->p >= 8 && m->p <= 15 && kn->k <= PIPE_KMAX && kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE && kn->kind >= FMCMC_KERNEL_NORMAL &&
                           K.lat != 0 && K.speclogit != 2 && kf >= 1 && (kn->scheme == FMCMC_SCHEME_JOINT || single_lat);
  // (and under kernel_adapt / kernel_ram -- unbounded, stride 1, no fixed parameter --: mh_sweep_spec<P, 4, KIND, LOGISTIC> with the register
  //  owner at the compile-time width k <= 16; general kernel: 6 - 14 us per step at n = 200.  Knob specwide=0: off)
  const bool lg_spec_wide = m->p >= 8 && m->p <= 15 && kn->k <= PIPE_KMAX && K.specwide != 0 &&
                            ((kn->kind == FMCMC_KERNEL_ADAPT && !adapt_hist) || (kn->kind == FMCMC_KERNEL_RAM && !ram_bounded && !kn->constr));
  if (!force && K.pipe != 0 && K.speclogit != 0 && K.shard < 0 && m->family == FMCMC_FAM_LOGISTIC && !mirror && m->p >= 1 && (m->p <= 7 || lg_lat_wide || lg_spec_wide) &&
      kn->k == m->p + (m->intercept ? 1 : 0) && ((kf == kn->k && kz == kn->k) || single_lat || (lg_lat_fixed && kf >= 1)) &&
      (((kn->kind == FMCMC_KERNEL_NORMAL || kn->kind == FMCMC_KERNEL_NORMAL_REFLECTIVE) && (kn->scheme == FMCMC_SCHEME_JOINT || single_lat)) ||
       (kn->kind == FMCMC_KERNEL_ADAPT && (!adapt_hist || adapt_ring)) || (kn->kind == FMCMC_KERNEL_RAM && !kn->constr && (!ram_bounded || K.specbnd != 0))) &&
      (unsigned long long)run->nsteps * (unsigned long long)kz * 8ull < (1ull << 32) && run->nsteps < (1ll << 28) &&
      (unsigned long long)kn->k * (unsigned long long)ldS * 8ull < (1ull << 32)) {
    if ((kn->scheme != FMCMC_SCHEME_JOINT || lg_lat_fixed || lg_lat_wide) && kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE) {
      // single-parameter schemes: the latency form's candidate wave, one to four chains per workgroup (as for the linear model above)
      // (a fixed parameter: at most 12 slots)
      if (per_cu <= 4 && (m->p <= 7 || lg_lat_wide) && nsl2 <= (lg_lat_fixed && fmh::reg_slots(m->p) > 12 ? 12 : fmh::reg_slots(m->p))) {
        pipe_opt = (int)nsl2; spec_logit = true; lat_normal = true;
        spec_cw = lat_forced ? K.lat : (int)per_cu;
      }
    } else
    if (nsl2 <= fmh::k_spec_optmax(m->p, kn->kind)) {
      pipe_opt = (int)nsl2;
      spec_logit = true;
      spec_cw = lat_forced ? K.lat : ((K.lat != 0 && per_cu <= 3) ? (int)per_cu : 4);
      // the normal / uniform kernels with fewer than four chains per CU: the latency form (mh_sweep_lat<.., LOGISTIC>: replicated decision)
      // (measured, tools/bench_small_logit.py and the pair of forms at 256 / 512 / 768 chains: the replicated decision wins up to ~3,000
      //  observations at any count -- 0.85 / 1.18 / 1.59 us against 1.25 / 1.34 / 1.78 at n = 1000 -- and up to ~6,000 with one chain
      //  per workgroup, 1.66 against 2.15 at n = 5000; beyond, the lookups' LDS time is the step and the owners' overlap pays:
      //  n = 10,000: 6.4 against 4.8 at 512 chains.  Knob speclogit=2: never.)
      if (spec_cw < 4 && K.speclogit != 2 && kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE && fmh::k_lat_logit(m->p, kn->kind) &&
          nsl2 <= (spec_cw == 1 ? 12 : 6)) lat_normal = true;
    }
  }
  // ---- the commit check: a register form is kept only where its instantiation exists and holds the slot count (a launch with a
  // slot count it does not hold would run no loop and hand back zeros -- round 5's soak found one such route); else the form below
  R.ring = adapt_ring;
  if (pipe_opt && !mfma_ng) {
    const Form f = lat_normal ? (spec_logit ? Form::LAT_LOGIT : Form::LAT) : (spec_logit ? Form::SPEC_LOGIT : Form::SPEC);
    const void* h = (f == Form::LAT) ? fmh::k_lat(m->p, kn->kind) : (f == Form::LAT_LOGIT) ? fmh::k_lat_logit(m->p, kn->kind)
                  : (f == Form::SPEC) ? (R.ring ? fmh::k_spec_ring(m->p, 0) : fmh::k_spec(m->p, kn->kind))
                  : (R.ring ? fmh::k_spec_ring(m->p, 1) : fmh::k_spec_logit(m->p, kn->kind));
    if (!h || pipe_opt > fmh::reg_slots(m->p) || (pipe_opt & 1)) {
      if (K.mode) fprintf(stderr, "fmcmc_amd: slot count %d beyond the register kernels' %d at p = %d: general kernel\n", pipe_opt, h ? fmh::reg_slots(m->p) : 0, m->p);
      pipe_opt = 0; lat_normal = false; spec_logit = false; spec_cw = 4;
    } else {
      R.form = f;
      R.kfn = h;
    }
  }
  R.pipe_opt = pipe_opt; R.spec_cw = spec_cw; R.mfma_ng = mfma_ng; R.mfma_ext = mfma_ext; R.mfma_ad = mfma_ad;
  if (mfma_ng) {
    R.form = mfma_ad ? Form::MFMA_ADAPTIVE : (mfma_ext ? Form::MFMA_STREAMED : Form::MFMA);
    if (mfma_ad) {
      // kernel_adapt / kernel_ram / mirror kernels: the adaptive owners between the barriers of the streamed evaluation (mh_mfma_ad.hpp)
      R.kx = (mfma_ad == 3) ? -2 : (mfma_ad == 2) ? -1 : ((kf != kn->k) ? 0 : (mfma_ng == 1 ? (kn->k == 5 ? 5 : 0) : (kn->k == 9 ? 9 : 0)));
      const bool bnd = mfma_ad == 1 && kn->kind == FMCMC_KERNEL_RAM && ram_bounded;
      R.kfn = fmh::k_mfma_ad(kn->kind, mfma_ng, R.kx, bnd ? 1 : 0, mfma_ext == 1 ? 1 : 0);   // (mfma_ext == 1, short data: one resident slot)
    }
  }
  const bool fast = pipe_opt || mfma_ng;
  if (fast) {   // step windows: the normal / uniform and adaptive kernels with the library's own stream
    const bool windowed = run->rng_mode == FMCMC_RNG_PHILOX && !mirror &&
                          (kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE || kn->kind == FMCMC_KERNEL_ADAPT || kn->kind == FMCMC_KERNEL_RAM);
    R.win = windowed ? step_window(run, kz, K) : 0;
  }

  // ---- the LONG-DATA form (mh_common.hpp, shard_long): few chains on long data.  Up to four chains are one workgroup of the
  // chain-sharded kernels, i.e. ONE compute unit walks the whole data set per step (n = 1e5, p = 3: 34 us per step, 255 CUs idle);
  // here all 256 workgroups evaluate their 1/256 of the observations for every chain and the canonical lane sums cross the chip as
  // in the other observation-sharded forms.  plan_long(kernel, its LDS bytes without the term block, what the call costs otherwise)
  // takes it when the cost model -- or knob shard=1 -- says so; us per step, fitted on `tools/dispatch_audit.py --only=long`
  // (profiles/r04_dispatch_audit.md): ~8 us of hand-overs, the walk of a lane's slots (1.6e-5 us per observation; sums of the
  // logistic terms 1.0e-5) once per group of chains whose terms fit the LDS, and per chain its terms and its share of the exchange.
  auto plan_long = [&](const void* kfn, size_t lds_base, double est_now, bool logistic) {
    if (force || K.shard == 0 || cw != 1 || ncu != 256 || run->nchains > 64 || m->n < 8 * NT || m->n >= (1ll << 31) || run->nsteps >= 30000000 ||
        (kn->kind == FMCMC_KERNEL_RAM && ram_bounded) || kn->kind < FMCMC_KERNEL_NORMAL || kn->kind > FMCMC_KERNEL_RAM) return;
    const long long room = ((long long)150 * 1024 - (long long)lds_base) / 8 - 2;
    const long long lrow = 2ll * shard_long_row((int)nsl) + SHL_BS;     // LDS doubles per chain of a group
    long long lcg = room / lrow;
    if (lcg > run->nchains) lcg = run->nchains;
    if (lcg < 1) return;
    const double pn = (double)m->n;
    const double groups = (double)((run->nchains + lcg - 1) / lcg);
    const double est_long = 8.3 + groups * (logistic ? 1.0e-5 : 1.6e-5) * pn + (logistic ? 2.0e-6 : 0.5e-6) * pn * (double)(m->p + 1) +
                            (double)run->nchains * (0.17 + 0.028 * (double)m->p + (logistic ? 3.0e-6 : 1.2e-6) * pn) +
                            (kn->kind >= FMCMC_KERNEL_ADAPT ? 3.5 : 0.0);
    if (!(K.shard == 1 || est_long < 0.9 * est_now)) return;
    R.kfn_long = kfn; R.lcg = lcg; R.lrow = lrow;
    R.lds_long = lds_base + sizeof(double) * (size_t)(lcg * lrow + 2);
  };
  // (wide linear models, p >= 16: where the matrix-core slices end -- 96 observations per workgroup, n = 24,576 -- the chain-sharded
  //  kernel is what is left: 4 + n p 8 / 65000 us per step)
  if (m->family == FMCMC_FAM_GAUSSIAN_LINREG && (m->p <= 15 || (m->p <= 62 && m->n > (long long)NT * 2 * SHM_T))) {
    const double pn = (double)m->n;
    const double now_rate = (m->p <= 3) ? (pn <= 2e5 ? 3.3e-4 : 5.1e-4) : (m->p <= 7 ? 4.9e-4 /* (round 5 audit: n = 2e4, p = 7, one chain: 9.75 us on the streamed MFMA kernel, the long-data form 10.6) */ : (m->p <= 11 ? 8.5e-4 : 1.17e-3));
    const double est_now = (m->p >= 16) ? 4.0 + pn * (double)m->p * 8.0 / 65000.0
                         : (m->n <= (long long)NT * fmh::mfma_reg_slots(m->p) ? 2.2 : now_rate * pn) + (kn->kind >= FMCMC_KERNEL_ADAPT ? 2.0 : 0.0);
    plan_long(fmh::k_wide(1, 2, kn->kind), R.lds, est_now, false);       // (the long-data form: one chain per workgroup, every proposal kernel)
  }

  // ---- the chain-sharded forms: what runs a call no fast form takes, and what a fast one steps down to
  R.nslots = (int)nsl;
  if (resident) { R.base = Form::RESIDENT; R.kfn_base = fmh::k_resident(R.res_p, kn->kind); }
  else if (!force && m->family == FMCMC_FAM_LOGISTIC && cw <= 4 && R.lds + sizeof(double) * (LG_LDS_DOUBLES + LG_LDS_TAIL) <= 160 * 1024 &&
           (kn->kind == FMCMC_KERNEL_NORMAL || kn->kind == FMCMC_KERNEL_NORMAL_REFLECTIVE || kn->kind == FMCMC_KERNEL_ADAPT ||
            kn->kind == FMCMC_KERNEL_RAM)) {
    // (round 4: kernel_adapt / kernel_ram too -- the workflow vignette's own model is a logistic regression under kernel_adapt;
    //  tools/option_audit.py found them on the all-family kernel at 3.9x the time per step of the normal kernels)
    // logistic-only instantiations: the g table in LDS; up to 28 / cw - 1 covariates their number is a compile-time constant
    // of the evaluation loop and the coefficients of the CW chains live in SGPRs (mh_common.hpp, logit_partials), beyond that
    // the run-time loop (logit_partials_any) -- still with the table in LDS, which is what the all-family kernel lacks
    const int lkv = kn->kind, lcw = cw <= 2 ? cw : 4;   // 1 .. 4
    R.base = Form::LOGISTIC;
    R.kfn_base = fmh::k_logit(lcw, 0, lkv);
    R.lds += sizeof(double) * (LG_LDS_DOUBLES + LG_LDS_TAIL);   // the table staged behind the chain blocks (16-byte aligned), logit_shard's control words
    // few chains: the long-data form (shard_long<LOGISTIC>) -- the sharded loop below keeps ONE thread per chain busy with its whole
    // slice (n = 1e5, 1 .. 64 chains: 31 .. 36 us per step), the chain-sharded one walks the data set in one workgroup
    if (!fast && m->p >= 1 && m->p <= 16) {
      const double w1 = (double)m->n * (double)(m->p + 12), stream1 = (double)m->n * (double)(m->p + 1) * 8.0 / 9.0e4;
      const double chain1 = 4.5 + ((w1 * 1.35e-5 > stream1) ? w1 * 1.35e-5 : stream1);
      const double shard1 = 10.3 + 1.78e-5 * (double)m->n * ((double)m->p + 10.3);
      plan_long(fmh::k_logit(1, 1, lkv), R.lds, (chain1 < shard1 || m->p > 16) ? chain1 : shard1, true);
    }
    // Observation-sharded form (mh_common.hpp, logit_shard): 256 workgroups of two canonical lanes each evaluate ALL chains
    // of the launch, up to 256 x cw of them; more chains run as consecutive launches.  Cost model (us per step): the
    // chain-sharded loop costs ~(p + 12) instructions per observation and chain, 4.5 + n cw (p + 12) 1.35e-5 with the
    // coefficients in SGPRs (p <= 28 / cw - 1; 2.8e-5 on the run-time loop beyond that) -- its lookups scatter over the table:
    // LDS-bound -- but never less than one pass of the workgroup over the data set at ~90 GB/s; the sharded form ~10 us of
    // hand-overs + n (p + 10.3) 1.78e-5 per 512 chains of a launch.  Knob shard=1 forces it for every eligible shape (tests),
    // shard=0 disables it.
    R.nb_launch = 256;
    R.ch_launch = (R.nblk > R.nb_launch) ? R.nb_launch * cw : (long long)run->nchains;
    bool lshard = false;
    // (round 5: the issue-priority turns of logit_shard, and for the normal / uniform kernels mh_sweep_logit2 -- four chains per
    //  workgroup whatever cw says --: 5 .. 15 % off every row of profiles/r05_dispatch_audit_logistic.md)
    const bool shadow_ok = K.shadow != 0 && kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE && kn->scheme == FMCMC_SCHEME_JOINT && kf == kn->k;
    // (not the bounded kernel_ram: its second evaluation of a step runs only in the workgroups where a proposal was reflected
    //  -- the grid-wide evaluation needs every workgroup in every hand-over)
    if (K.shard != 0 && m->p >= 1 && m->p <= 16 && ncu == 256 && m->n >= 2 * NT && m->n < (1ll << 28) &&
        !(kn->kind == FMCMC_KERNEL_RAM && ram_bounded)) {
      // (refitted to tools/dispatch_audit.py, profiles/r04_dispatch_audit.md: n = 2e3 .. 1e5, p = 2, 5, 8, 64 .. 4096 chains)
      const long long nb_launch = R.nb_launch, ch_launch = R.ch_launch;
      const double w = (double)m->n * (double)(m->p + 12);
      const double stream_us = (double)m->n * ((double)m->p + 0.5) * 8.0 / 9.0e4;      // a workgroup's pass over the data set (X only: the term does not read y) at ~90 GB/s
      const double loop_us = w * cw * ((m->p <= 28 / cw - 1) ? 1.35e-5 : 2.8e-5);
      const double rounds = (double)((R.nblk + ncu - 1) / ncu), launches = (double)((run->nchains + ch_launch - 1) / ch_launch);
      const double est_chain = (4.5 + (loop_us > stream_us ? loop_us : stream_us)) * rounds;
      const double passes = (double)((ch_launch + NT - 1) / NT);                       // chains per thread of the sharded loop
      const double launches_s = shadow_ok ? (double)((run->nchains + 4 * nb_launch - 1) / (4 * nb_launch)) : launches;
      const double passes_s = shadow_ok ? (double)(((run->nchains < 4 * nb_launch ? run->nchains : 4 * nb_launch) + NT - 1) / NT) : passes;
      const double est_shard = ((shadow_ok ? 8.5 : 10.0) + 2.2 * (passes_s - 1.0) +
                                (shadow_ok ? 1.62e-5 : 1.72e-5) * (double)m->n * ((double)m->p + 10.3) * passes_s) * launches_s;
      lshard = K.shard == 1 || est_shard < 0.95 * est_chain;
    }
    if (lshard && !fast) {
      R.form = Form::LOGISTIC_SHARDED;
      R.kfn = fmh::k_logit(lcw, 1, lkv);
      R.lds_run = R.lds;
      // (variates from a stream, the library's or the caller's: the instantiation without the generators in its body)
      R.kfn_fed = fmh::k_logit(lcw, 2, lkv);
      // (mh_sweep_logit2 holds four chains per workgroup whatever cw says)
      R.ch_shadow = (run->nchains < 4 * R.nb_launch) ? (long long)run->nchains : 4 * R.nb_launch;
      // the normal / uniform proposal kernels, joint scheme, no fixed parameter: mh_sweep_logit2 (mh_logit2.hpp) -- four chains per
      // workgroup whatever cw says, the owners' work in the shadow of the hand-overs (knob shadow=0: off)
      // (kernel_adapt / kernel_ram with up to eight parameters, none fixed, no window / constraint / bound: the same sweep with the
      //  register owner of mh_spec.hpp, mh_sweep_logit2a)
      const bool adaptive3 = (kn->kind == FMCMC_KERNEL_ADAPT && !adapt_hist) || (kn->kind == FMCMC_KERNEL_RAM && !kn->constr && !ram_bounded);
      R.kfn_shadow = (K.shadow == 0 || kf != kn->k || kz != kn->k) ? nullptr
                   : (kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE ? (kn->scheme == FMCMC_SCHEME_JOINT ? fmh::k_logit2(lkv) : nullptr)
                      : ((adaptive3 && kn->k <= SPEC_KA && kn->k <= PIPE_KMAX) ? fmh::k_logit2a(lkv) : nullptr));
      if (R.kfn_shadow) R.lds_shadow = (kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE) ? fmh::k_logit2_lds(kn->k) : fmh::k_logit2a_lds();
    }
  }
  else if (m->family == FMCMC_FAM_GAUSSIAN_LINREG && m->p >= 16 && cw <= 2 &&
           (kn->kind == FMCMC_KERNEL_RAM || kn->kind == FMCMC_KERNEL_NORMAL || kn->kind == FMCMC_KERNEL_NORMAL_REFLECTIVE)) {
    // wide linear models (config C4: k = 50): one family and one proposal kernel compiled in, which leaves the streamed
    // evaluation the registers for 4 observations x 8 columns in flight per thread (mh_common.hpp)
    const int kv = kn->kind, nslots = (int)nsl;   // 1, 2 or 4
    R.base = Form::WIDE;
    R.kfn_base = fmh::k_wide(cw, 0, kv);
    // Observation-sharded evaluation: one cooperative launch when the call has 128 or 256 workgroups, consecutive launches
    // of 256 workgroups when it has a multiple of that (more than 512 chains per GPU at two chains per workgroup)
    // (a launch may hold workgroups WITHOUT chains -- they own canonical lanes like the others -- so any chain count works:
    //  up to 512 chains run as one launch of 256 workgroups, exactly 128 workgroups keep 4 lanes each when n allows)
    R.nb_launch = (R.nblk == 128 && 4 * nslots <= SH_MAXO) ? 128 : 256;
    R.ch_launch = (R.nblk > R.nb_launch) ? R.nb_launch * cw : (long long)run->nchains;
    Knobs Kw = K;
    if (R.wide_switched && K.shard != 0) Kw.shard = 1;
    const int lpw = wide_sharded_lanes(Kw, m, kn, run, ram_bounded, ncu, R.nb_launch, cw);
    bool shard = lpw > 0;
    if (K.mode & 256) fprintf(stderr, "fmcmc_amd: wide path nblk=%lld lpw=%d nslots=%d p=%d bounded=%d shard=%d\n", R.nblk, lpw, nslots, m->p, (int)ram_bounded, (int)shard);
    // the slice product on the matrix cores (shard_columns_mfma): the slice lives in LDS behind the chain blocks
    const int mf_spg = shard ? (nslots + 4 / lpw - 1) / (4 / lpw) : 0, nmt = (mf_spg + 3) / 4;
    const int mblk = shm_hdr(nmt) + nmt * ((m->p + 3) / 4) * 64;
    // (three M-tiles of which the third holds values 8, 9 only, at the width with a compile-time K-block count -- config C4:
    //  its 8 rows go through two 4x4x4 MFMAs per K-block instead of a 16x16x4 that is half padding; knob t10=0: off)
    //  (the form reads values 0 .. SHM_T10_FULL - 1 of every lane group without a mask: slots spg h + t <= nslots - 2 are full)
    const bool t10_full = shard && mf_spg * (4 / lpw - 1) + (SHM_T10_FULL - 1) <= nslots - 2;
    R.t10 = (nmt == 3 && mf_spg <= 10 && (m->p + 3) / 4 == 12 && t10_full && K.t10 != 0) ? 1 : 0;
    R.mfma_form = shard && shard_mfma_enabled(K) && m->p <= 4 * SHM_KBMAX && mf_spg <= SHM_T &&
                  R.lds + sizeof(double) * (size_t)(mblk + 1) <= 160 * 1024;
    if (shard && !R.mfma_form && lpw * nslots > SH_MAXO) shard = false;      // (more than 40 observations per slice: the matrix-core form or none)
    // the dataflow form (mh_wide2.hpp): owner and evaluator waves decoupled, two chain groups half a step out of phase.
    // It pays where the owners have real work to hide -- kernel_ram: 35.8 -> 27.9 us per step at C4 -- and costs the normal
    // kernels 6 % (26.2 against 24.6: their owner phase is short and two of eight waves no longer evaluate).
    // Knob wide2=0 keeps the sequential form everywhere, wide2=1 takes the dataflow form for every eligible call (tests).
    const bool w2on = K.wide2 == 1 || (K.wide2 != 0 && kn->kind == FMCMC_KERNEL_RAM);
    R.wide2 = shard && R.mfma_form && w2on && lpw == 2 && cw == 2 && R.nb_launch == 256 && ncu == 256 &&
              !(kn->kind == FMCMC_KERNEL_RAM && kn->constr) && (kn->kind == FMCMC_KERNEL_RAM || kn->scheme == FMCMC_SCHEME_JOINT) &&
              nmt >= 1 && nmt <= 3 && run->nsteps < 100000000 &&
              sizeof(double) * wide2_lds_doubles(kn->k, kf, kn->kind, kz, mblk) <= 160 * 1024;
    R.lpw = lpw; R.nmt = nmt; R.mblk = mblk;
    if (fast) {
    } else if (R.wide2) {
      R.form = Form::WIDE_DATAFLOW;
      R.kfn = fmh::k_wide2(kv, nmt);
      R.lds_run = sizeof(double) * wide2_lds_doubles(kn->k, kf, kn->kind, kz, mblk);
      R.ngrp = (K.groups == 4) ? 4 : 2;
      R.tiles = (K.tiles == 0 || R.ngrp == 4) ? 0 : 1;
    } else if (shard) {
      // the sharded evaluation is its own instantiation (OPT = lanes per workgroup): sharing one with the streamed loop
      // cost 200-300 spilled registers in BOTH paths
      R.form = R.mfma_form ? Form::WIDE_SHARDED_MFMA : Form::WIDE_SHARDED;
      R.kfn = fmh::k_wide(cw, lpw, kv);
      R.lds_run = R.lds + (R.mfma_form ? sizeof(double) * (size_t)(mblk + 1) : 0);
    }
  }
  else { R.base = Form::GENERAL; R.kfn_base = fmh::k_general(cw); }
  if (!fast && R.form == Form::GENERAL) { R.form = R.base; R.kfn = R.kfn_base; }   // (no fast or sharded form)
  return R;
}
