// mh_engine.hip — gfx950 (MI355X) many-chain Metropolis-Hastings engine: the C-ABI (include/fmcmc_amd.h), validation, the
// launcher (launch_sweep: executes the plan of mh_route.hpp's plan_route, one function per form), the callback sweeps (run_fun; run_user)
// and the sweep of one model on many datasets (run_batch).
// Two headers belong to this unit alone: mh_prep.hpp (the data-preparation kernels launch_sweep enqueues) and mh_host.hpp (the
// staging of the host-pointer entry points).  The sweep kernels are instantiated in the k_*.hip translation units (compiled in
// parallel, fmcmc_amd/build.py) and reached through the look-ups of mh_kernels.hpp; their source is in the headers:
//   mh_common.hpp  shared device helpers      mh_streamed.hpp  general kernel (all families / kernels / schemes)
//   mh_rng.hpp     RNG stream kernel          mh_mfma.hpp      fp64-MFMA kernel, owner waves (headline)
//   mh_spec.hpp    wave-specialised kernel (kernel_adapt / kernel_ram; the latency form for few chains)
//   mh_wide2.hpp   wide models: observation-sharded dataflow kernel (owner / evaluator waves, two chain groups)
//   mh_mfma_ad.hpp adaptive owners on the MFMA evaluation   mh_bigk.hpp  more than 64 parameters
//
// Replaces, for ALL chains of a call at once, the per-chain loop of the reference
//   R/mcmc.R:720-838 (loop, accept, burn-in/thin)  x  R/kernel_normal.R / R/kernel_adapt.R /
//   R/kernel_ram.R / R/recursive.R / R/kernel.R:450-493 (proposal kernels).
//
// Execution model (DESIGN.md has the full picture):
//   * one 512-thread workgroup (8 wavefronts) owns CW chains; its 512 threads ARE the 512
//     "canonical lanes" of the log-posterior reduction: observation i belongs to lane i mod 512,
//     each lane accumulates its observations in index order with fma, lanes are combined by an
//     xor-butterfly tree (levels 1..32 inside a wavefront, 64..256 across the 8 wavefronts).
//     The CPU oracle mirrors exactly this tree, so accept decisions are bit-identical.
//   * every data value loaded by a thread is applied to all CW chains of the workgroup
//     (register/L2 traffic amortised over chains);
//   * per-chain "scalar" work (proposal, adaptation, accept) is done by the chain's owner
//     wavefront, lanes = parameters (one lane per row of Sigma / S);
//   * RNG = Philox4x32-10 counter stream (include/fmh_philox.h) or host-fed variates.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (explicit fma only).
#define FMH_WITH_RNG_FILL
#include "mh_tu.hpp"
#include <vector>
// (host-side shape helpers of the kernel families -- LDS sizes, slot counts; their kernels are instantiated in the k_*.hip files)
#include "mh_streamed.hpp"
#include "mh_mfma.hpp"
#include "mh_spec.hpp"
#include "mh_lat.hpp"
#include "mh_wide2.hpp"
#include "mh_mfma_ad.hpp"
#include "mh_bigk.hpp"
#include "mh_route.hpp"   // (kernel selection: plan_route)
#include "mh_fun.hpp"     // (the callback path: FunArgs, its LDS size; mh_fun_step is instantiated in k_fun.hip)
#include "mh_user.hpp"    // (a caller-defined transition kernel: UserArgs, EvalArgs; the kernels are instantiated in k_fun.hip)
#include "mh_batch.hpp"   // (one model on many datasets: BatchArgs, the LDS rule; mh_sweep_batch is instantiated in k_fun.hip)
#include "mh_prep.hpp"    // (the data-preparation kernels the launcher enqueues in front of a sweep)

static thread_local const char* g_kernel = "";

static int count_free(const fmcmc_kernel* kn, const uint8_t* fixed_host) {
  int kf = 0;
  for (int j = 0; j < kn->k; j++)
    if (!fixed_host[j]) kf++;
  return kf;
}
// is any free parameter bounded? (host copies of the kernel's arrays)
static int any_bounded(const uint8_t* fixed, const double* lb, const double* ub, int k) {
  for (int j = 0; j < k; j++)
    if (!fixed[j] && (lb[j] > -DBL_MAX || ub[j] < DBL_MAX)) return 1;
  return 0;
}
static bool is_simple_kind(int kind) {
  return kind == FMCMC_KERNEL_NORMAL || kind == FMCMC_KERNEL_NORMAL_REFLECTIVE || kind == FMCMC_KERNEL_UNIF ||
         kind == FMCMC_KERNEL_UNIF_REFLECTIVE || kind == FMCMC_KERNEL_NMIRROR || kind == FMCMC_KERNEL_UMIRROR;
}
static int variates_per_step(const fmcmc_kernel* kn, int kf) {  // single-parameter schemes draw one variate per step
  return (is_simple_kind(kn->kind) && kn->scheme != FMCMC_SCHEME_JOINT) ? 1 : kf;
}

// ==============================================================================================
// C-ABI
// ==============================================================================================
extern "C" {

int fmcmc_abi_version(void) { return FMCMC_ABI_VERSION; }
const char* fmcmc_last_error(void) { return g_err; }
// (not part of the C-ABI: the other translation units of the library leave their texts in the same thread-local buffer)
__attribute__((visibility("hidden"))) void fmcmc_set_error_text_(const char* text) { set_err("%s", text); }
const char* fmcmc_last_kernel(void) { return g_kernel; }

int fmcmc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int64_t fmcmc_kept_rows(int64_t nsteps, int64_t burnin, int64_t thin) {
  if (thin < 1 || burnin >= nsteps) return 0;
  return (nsteps - burnin) / thin;
}

// Argument checks with the reference's own messages (R/mcmc.R:501-520, R/kernel.R:9,129-132,
// R/kernel_normal.R:134-135). Pointers inside `kernel` must be HOST pointers here.
// the run arguments and the parameter count (R/mcmc.R:501-520), the checks fmcmc_validate and fmcmc_validate_fun share first
static int validate_run(const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (run->nchains < 1) { set_err("`nchains` must be an integer greater than 1."); return FMCMC_ERR_ARG; }
  if (run->burnin >= run->nsteps) {
    set_err("-burnin- (%lld) cannot be >= than -nsteps- (%lld).", (long long)run->burnin, (long long)run->nsteps);
    return FMCMC_ERR_ARG;
  }
  if (run->thin >= run->nsteps) {
    set_err("-thin- (%lld) cannot be > than -nsteps- (%lld).", (long long)run->thin, (long long)run->nsteps);
    return FMCMC_ERR_ARG;
  }
  if (run->thin < 1) { set_err("-thin- should be >= 1."); return FMCMC_ERR_ARG; }
  if (kn->k < 1 || kn->k > FMCMC_MAX_K) {
    set_err("number of parameters k=%d outside [1, %d]", kn->k, FMCMC_MAX_K);
    return FMCMC_ERR_UNSUPPORTED;
  }
  return FMCMC_OK;
}

// the kernel's own arguments (R/kernel.R:9,129-132, R/kernel_normal.R:134-135, ...) and the fed stream, shared as well
static int validate_kernel(const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (kn->kind < FMCMC_KERNEL_NORMAL || kn->kind > FMCMC_KERNEL_UMIRROR) {
    set_err("unknown kernel kind %d", kn->kind);
    return FMCMC_ERR_ARG;
  }
  const bool simple = is_simple_kind(kn->kind);
  if (kn->kind == FMCMC_KERNEL_RAM) {
    if (kn->ram_qfun < FMCMC_RAM_QFUN_T_K || kn->ram_qfun > FMCMC_RAM_QFUN_T_DF) {
      set_err("kernel_ram: unknown -qfun- family %d (0 = rt(k, k), 1 = rnorm(k), 2 = rt(k, df)).", kn->ram_qfun);
      return FMCMC_ERR_ARG;
    }
    if (kn->ram_qfun == FMCMC_RAM_QFUN_T_DF && !(kn->ram_df > 0.0 && kn->ram_df <= DBL_MAX)) {
      set_err("kernel_ram: -qfun- = rt(k, df) needs a finite df > 0.");
      return FMCMC_ERR_ARG;
    }
    if (!(kn->ram_eta_exp >= 0.0 && kn->ram_eta_exp <= DBL_MAX)) {
      set_err("kernel_ram: the exponent of -eta- must be finite and positive (0 selects the default 2/3).");
      return FMCMC_ERR_ARG;
    }
  }
  if (simple && (kn->scheme < FMCMC_SCHEME_JOINT || kn->scheme > FMCMC_SCHEME_EXPLICIT)) {
    set_err("-scheme- update must be either an integer sequence, 'joint', 'ordered', or 'random'.");
    return FMCMC_ERR_ARG;
  }
  if (kn->fixed && kn->lb && kn->ub) {
    int kf = count_free(kn, kn->fixed);
    if (kf == 0) {
      set_err("The number of parameters to update, i.e. not fixed, cannot be zero. "
              "Check the value -fixed- in the kernel initialization.");
      return FMCMC_ERR_ARG;
    }
    if (kn->kind != FMCMC_KERNEL_NORMAL && kn->kind != FMCMC_KERNEL_UNIF)
      for (int j = 0; j < kn->k; j++)
        if (!(kn->ub[j] > kn->lb[j])) { set_err("-ub- cannot be <= than -lb-."); return FMCMC_ERR_ARG; }
    if ((kn->kind == FMCMC_KERNEL_UNIF || kn->kind == FMCMC_KERNEL_UNIF_REFLECTIVE) && kn->scale)
      for (int j = 0; j < kn->k; j++)   // scale = max. - min. (R/kernel_unif.R:55-56, :123-124)
        if (!(kn->scale[j] > 0.0)) { set_err("-max.- cannot be <= than -min.-."); return FMCMC_ERR_ARG; }
    if (simple && kn->scheme == FMCMC_SCHEME_EXPLICIT) {  // R/kernel.R:72-90
      if (!kn->scheme_seq || kn->scheme_len != kf) {
        set_err("When setting the update scheme, it should have the same length as the number of variables that will "
                "not be fixed. Right now length(scheme) = %d while sum(!fixed) = %d.", kn->scheme_seq ? kn->scheme_len : 0, kf);
        return FMCMC_ERR_ARG;
      }
      for (int j = 0; j < kn->k; j++) {
        if (kn->fixed[j]) continue;
        bool found = false;
        for (int a = 0; a < kn->scheme_len; a++) found = found || (kn->scheme_seq[a] == j);
        if (!found) {
          set_err("One or more variables was not included in the ordering sequence. Only variables that are not fixed "
                  "can be included in this list.");
          return FMCMC_ERR_ARG;
        }
      }
    }
  }
  if (kn->kind == FMCMC_KERNEL_ADAPT && (kn->freq < 1 || kn->bw < 0)) {
    set_err("-freq- must be >= 1 and -bw- >= 0 (got freq=%d, bw=%d)", kn->freq, kn->bw);
    return FMCMC_ERR_ARG;
  }
  if (kn->kind == FMCMC_KERNEL_RAM && kn->freq < 1) { set_err("-freq- must be >= 1."); return FMCMC_ERR_ARG; }
  if (kn->kind == FMCMC_KERNEL_ADAPT && kn->bw > 0 && kn->bw > kn->warmup) {
    set_err("The `warmup` parameter must be greater than `bw`.");
    return FMCMC_ERR_ARG;
  }
  if (run->rng_mode == FMCMC_RNG_FED && (!run->fed_logu || !run->fed_z)) {
    set_err("rng_mode = FED needs fed_logu and fed_z");
    return FMCMC_ERR_ARG;
  }
  return FMCMC_OK;
}

int fmcmc_validate(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (!m || !kn || !run) { set_err("null argument"); return FMCMC_ERR_ARG; }
  const int rr = validate_run(kn, run);
  if (rr != FMCMC_OK) return rr;
  if (kn->k > FMCMC_MAX_K_WAVE) {   // one workgroup per chain (mh_sweep_bigk): what it implements
    const bool simple_joint = (kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE || kn->kind == FMCMC_KERNEL_UNIF || kn->kind == FMCMC_KERNEL_UNIF_REFLECTIVE) &&
                              kn->scheme == FMCMC_SCHEME_JOINT;
    const bool adapt_plain = kn->kind == FMCMC_KERNEL_ADAPT && kn->bw == 0 && kn->freq <= 1;
    if (!(simple_joint || adapt_plain || kn->kind == FMCMC_KERNEL_RAM)) {
      set_err("k = %d > %d parameters: supported are kernel_normal(_reflective) / kernel_unif(_reflective) with scheme = 'joint', "
              "kernel_adapt(bw = 0, freq = 1) and kernel_ram", kn->k, FMCMC_MAX_K_WAVE);
      return FMCMC_ERR_UNSUPPORTED;
    }
  }
  const int kexp = eval_params(m->family, m->p, m->intercept);
  if (kexp < 0) { set_err("unknown log-posterior family %d", m->family); return FMCMC_ERR_ARG; }
  if (kexp != kn->k) {
    set_err("Incorrect length of -initial-: the model has %d parameters, the kernel %d.", kexp, kn->k);
    return FMCMC_ERR_ARG;
  }
  if (m->n < 1) { set_err("the model needs at least one observation"); return FMCMC_ERR_ARG; }
  return validate_kernel(kn, run);
}

}  // extern "C"

// ---- the launcher: what executes a plan (mh_route.hpp).  kernel->fixed etc. are DEVICE pointers from here on.
// The same sweep for the chains [off, off + cnt) of a call: every per-chain array advanced, RNG ids continued.
static SweepArgs chain_window(const SweepArgs& A, long long off, long long cnt, int kf) {
  SweepArgs W = A;
  const long long k = A.k, S = A.ldS, ns = A.nsteps, words = (A.nsteps + 31) >> 5;
  W.nchains = cnt; W.chain_base = A.chain_base + off;
#define ADV(f, stride) if (W.f) W.f += off * (stride)
  ADV(scheme_cols, ns); ADV(mirror_mu, k); ADV(mirror_scale, k); ADV(obs_arate, k);
  ADV(hist, (long long)A.hist_rows * kf);
  ADV(fed_logu, ns); ADV(fed_z, ns * A.kz);
  ADV(win_sum, kf); ADV(theta0, k); ADV(f0, 1); ADV(abs_iter, 1); ADV(Sigma, (long long)kf * kf); ADV(mean_prev, kf); ADV(have_mean, 1); ADV(nerrors, 1);
  ADV(samples, k * S); ADV(logpost, S); ADV(draws, k * S); ADV(accept_count, 1); ADV(accept_bits, words);
  ADV(status, 1); ADV(status_step, 1); ADV(status_theta, k);
#undef ADV
  return W;
}

// the stream-ordered scratch blocks of a call: all of them released on EVERY way out of launch_sweep / run_fun
struct ScratchList {
  hipStream_t s = nullptr;
  void* blk[8];
  int n = 0;
  explicit ScratchList(hipStream_t stream) : s(stream) {}
  ScratchList(const ScratchList&) = delete;
  ~ScratchList() { while (n > 0) (void)hipFreeAsync(blk[--n], s); }
  // `field`: the address of the pointer that receives the block; `what` names it in the message of a refusal (nullptr: the
  // caller steps down instead, no error is left behind)
  int grab(void* field, size_t bytes, const char* what) {
    void* q = nullptr;
    const hipError_t e = (n < 8) ? hipMallocAsync(&q, bytes, s) : hipErrorOutOfMemory;
    if (e != hipSuccess) {
      if (what) set_err("hipMallocAsync(%s) failed: %s", what, hipGetErrorString(e));
      else (void)hipGetLastError();
      return FMCMC_ERR_DEVICE;
    }
    blk[n++] = q;
    *(void**)field = q;
    return FMCMC_OK;
  }
};

// what every step of launch_sweep works on: the NORMALISED call, the device, the stream and the call's scratch
struct SweepCtx {
  fmcmc_model m;
  fmcmc_kernel kn;
  const fmcmc_run* run;
  int kf;
  Knobs K;
  int dev = 0, ncu = 256;
  hipStream_t stream;
  ScratchList scratch;
  hipError_t e = hipSuccess;   // the first launch that failed (the tail of launch_sweep reports it)
  SweepCtx(const fmcmc_model* m_in, const fmcmc_kernel* kn_in, const fmcmc_run* r, int kf_, hipStream_t s)
      : m(*m_in), kn(*kn_in), run(r), kf(kf_), K(read_knobs()), stream(s), scratch(s) {}
};

// the code object is gfx950 only, and the hand-overs of the wide kernels rest on ITS cache behaviour (mh_common.hpp).  One
// query per device of the process: a second device of another architecture is refused as well.
static int require_gfx950(int dev) {
  static signed char known[64];   // by device index -- 0: not asked yet, 1: gfx950, -1: another architecture
  signed char beyond = 0, &ok = (dev >= 0 && dev < 64) ? known[dev] : beyond;
  if (!ok) {
    hipDeviceProp_t prop;
    ok = (hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ? 1 : -1;
  }
  if (ok < 0) { set_err("this library is built for gfx950 (MI355X); the current device is another architecture"); return FMCMC_ERR_DEVICE; }
  return FMCMC_OK;
}

// The run / state / out fields that SweepArgs, FunArgs and UserArgs all have (they name them alike), and the row stride
template <class Args>
static int fill_run_args(Args& A, int k, const fmcmc_run* run, const fmcmc_state* st, const fmcmc_out* out) {
  A.k = k;
  A.nchains = run->nchains; A.nsteps = run->nsteps; A.burnin = run->burnin; A.thin = run->thin;
  const long long S = fmcmc_kept_rows(run->nsteps, run->burnin, run->thin);
  A.ldS = out->ld_rows > 0 ? out->ld_rows : S;
  if (A.ldS < S) { set_err("fmcmc_out.ld_rows (%lld) is smaller than the %lld kept rows of this call", (long long)out->ld_rows, S); return FMCMC_ERR_ARG; }
  A.chain_base = run->chain_base; A.step_base = run->step_base; A.seed = run->seed;
  A.rng_mode = run->rng_mode; A.fed_logu = run->fed_logu;
  A.theta0 = st->theta0; A.f0 = st->f0;
  A.samples = out->samples; A.logpost = out->logpost; A.draws = out->draws;
  A.accept_count = (long long*)out->accept_count; A.accept_bits = out->accept_bits;
  A.status = out->status; A.status_step = (long long*)out->status_step; A.status_theta = out->status_theta;
  return FMCMC_OK;
}

// On top of them, the kernel fields and the adaptive state that SweepArgs and FunArgs both have, and what is derived from them:
// kernel_ram's qfun / eta families, the variates per step.  `kn`: the kernel as the device code sees it.
template <class Args>
static int fill_call_args(Args& A, const fmcmc_kernel* kn, const fmcmc_run* run, const fmcmc_state* st, const fmcmc_out* out, int kf) {
  A.kind = kn->kind; A.scheme = kn->scheme; A.warmup = kn->warmup;
  A.freq = kn->freq < 1 ? 1 : kn->freq; A.scheme_seq = kn->scheme_seq; A.scheme_len = kn->scheme_len;
  A.constr = (kn->kind == FMCMC_KERNEL_RAM) ? kn->constr : nullptr;
  A.until = kn->until; A.eps = kn->eps; A.arate = kn->arate;
  // kernel_ram's qfun / eta families (R/kernel_ram.R:67-68): df of the t variates (0 = normal) and the exponent of eta
  A.ram_df = (kn->ram_qfun == FMCMC_RAM_QFUN_NORMAL) ? 0.0 : (kn->ram_qfun == FMCMC_RAM_QFUN_T_DF ? kn->ram_df : (double)kf);
  A.ram_neg_exp = (kn->ram_eta_exp != 0.0) ? -kn->ram_eta_exp : (-2.0 / 3.0);
  A.mu = kn->mu; A.scale = kn->scale; A.lb = kn->lb; A.ub = kn->ub;
  A.fresh = st->fresh;
  A.kz = variates_per_step(kn, kf);
  A.fed_z = run->fed_z;
  A.abs_iter = (long long*)st->abs_iter; A.Sigma = st->Sigma;
  A.mean_prev = st->mean_prev; A.have_mean = st->have_mean; A.nerrors = st->nerrors; A.scheme_cols = st->scheme_cols;
  return fill_run_args(A, kn->k, run, st, out);
}

// the logistic family's data-only sums of the linear part and the columns' largest |x| (logit_hs_kernel), into the call's scratch
static int enqueue_logit_sums(const fmcmc_model& m, ScratchList& scratch, hipStream_t stream, const double** hs_out) {
  double* hs = nullptr;
  const int rh = scratch.grab(&hs, sizeof(double) * (size_t)(2 * MAXK + 2), "logistic sums");
  if (rh != FMCMC_OK) return rh;
  hipLaunchKernelGGL(logit_hs_kernel, dim3(1), dim3(NT), 0, stream, m.X, m.y, (long long)m.n, m.p, m.intercept ? 1 : 0, hs);
  *hs_out = hs;
  return FMCMC_OK;
}

// ---- the two callback sweeps (run_fun, run_user): one step kernel launch per evaluation
// the caller's log-posterior at theta [C][k] -> f [C]; a non-zero return is the call's error, with the loop step in its text
static int call_logpost(fmcmc_logpost_fn fun, const double* theta, long long C, int k, double* f, hipStream_t stream, void* user, long long step) {
  const int rc = fun(theta, (int64_t)C, (int32_t)k, f, (void*)stream, user);
  if (rc == 0) return FMCMC_OK;
  set_err("the log-posterior callback returned %d at loop step i = %lld%s", rc, step, step == 1 ? " (row 1: the initial values)" : "");
  return FMCMC_ERR_FUN;
}
// the step kernel of loop step `step`, one workgroup of nth threads per chain
template <class Args>
static int launch_step(const void* kfn, long long C, int nth, size_t lds, hipStream_t stream, const Args& A, long long step) {
  void* kargs[] = {(void*)&A};
  hipError_t e = hipLaunchKernel(kfn, dim3((unsigned)C), dim3((unsigned)nth), kargs, lds, stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { set_err("HIP launch failed at loop step i = %lld: %s", step, hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
  return FMCMC_OK;
}

// the canonical stream of chains [chain_base, + nchains) x steps [step_base, + nsteps) into logu [C][rows], z [C][rows][kz]
static void fill_rng(unsigned long long seed, long long step_base, long long chain_base, long long nchains, long long nsteps, int kz, double df,
                     double* logu, double* z, hipStream_t s) {
  const size_t items = (size_t)nchains * (size_t)nsteps;
  hipLaunchKernelGGL(rng_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, seed, step_base, chain_base, nchains, nsteps, kz, df,
                     logu, z);
}
// the variates a kernel's own stream draws (rng_fill_kernel: t / U(0,1) / normal)
static double fill_df(const SweepArgs& A) { return (A.kind == FMCMC_KERNEL_RAM) ? A.ram_df : (A.variate == 1 ? -1.0 : 0.0); }

// launch of a kernel handle (mh_kernels.hpp): every sweep kernel takes the launch's SweepArgs by value
static hipError_t launch_k(const void* kfn, long long grid, int block, size_t lds, hipStream_t stream, const SweepArgs& A) {
  if (!kfn) return hipErrorInvalidDeviceFunction;
  if (lds > 48 * 1024) {
    const hipError_t ea = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return ea;
  }
  void* kargs[] = {(void*)&A};
  return hipLaunchKernel(kfn, dim3((unsigned)grid), dim3((unsigned)block), kargs, lds, stream);
}

// Can `nb` workgroups of kernel `kfn` with `lds` bytes of LDS be co-resident, i.e. may it run as ONE cooperative launch?
// `what`: the A.debug & 256 diagnostic of a refusal (nullptr: none).  A refusal leaves no error behind.
static bool coop_fits(const SweepCtx& cx, const void* kfn, size_t lds, long long nb, const char* what) {
  int coop = 0, perCU = 0;
  (void)hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, cx.dev);
  const hipError_t e = kfn ? hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipErrorInvalidDeviceFunction;
  if (e != hipSuccess || !coop || hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kfn, NT, lds) != hipSuccess || (long long)perCU * cx.ncu < nb) {
    if (what && (cx.K.mode & 256)) fprintf(stderr, "fmcmc_amd: %s not launched: err=%d coop=%d perCU=%d lds=%zu\n", what, (int)e, coop, perCU, lds);
    (void)hipGetLastError();
    return false;
  }
  return true;
}

// The chains of a call as consecutive cooperative launches of `nb` workgroups, `per` chains each (the observation-sharded forms:
// the slices and tables serve every launch; the grid barrier words `bar` are cleared in front of each).
enum CoopRun { COOP_OK, COOP_NOTHING_RAN, COOP_LATER_FAILED };
static CoopRun coop_chain_windows(const void* kfn, long long nb, size_t lds, const SweepArgs& A, long long nchains, long long per, int kf,
                                  unsigned* bar, size_t nbar, hipStream_t stream) {
  hipError_t e = hipSuccess;
  long long done = 0;
  for (; done < nchains && e == hipSuccess; done += per) {
    SweepArgs W = chain_window(A, done, (nchains - done < per) ? nchains - done : per, kf);
    (void)hipMemsetAsync(bar, 0, sizeof(double) * nbar, stream);
    void* kargs[] = {(void*)&W};
    e = hipLaunchCooperativeKernel(kfn, dim3((unsigned)nb), dim3(NT), kargs, (unsigned int)lds, stream);
  }
  if (e == hipSuccess) return COOP_OK;
  (void)hipGetLastError();
  if (done <= per) return COOP_NOTHING_RAN;     // the runtime refused the first cooperative launch
  // a LATER window failed: the chains of the earlier windows have run
  set_err("HIP launch of chain window %lld failed (%s): the state of the first %lld chains is already advanced, the results of this call are invalid",
          (long long)(done / per), hipGetErrorString(e), (long long)(done - per));
  return COOP_LATER_FAILED;
}

// The tables of an observation-sharded form, carved out of ONE scratch block: p[i] begins n[0] + .. + n[i - 1] doubles behind
// the block's base -- the pieces in the order the caller lists them (long / logistic: theta | partials | barrier | slices;
// wide: xs | ys | theta | partials | barrier | mfma).
static int grab_carved(SweepCtx& cx, const size_t* n, int cnt, double** p) {
  size_t total = 0;
  for (int i = 0; i < cnt; i++) total += n[i];
  double* base = nullptr;
  const int rc = cx.scratch.grab(&base, sizeof(double) * total, "sharded evaluation");
  for (int i = 0; i < cnt && rc == FMCMC_OK; i++) { p[i] = base; base += n[i]; }
  return rc;
}
// their sizes in doubles for `ch` chains per launch: the proposals [k][ch + SH_PAD] (rounded so that the partials behind them stay
// 64-byte aligned), the lane partials [512 + SH_PAD][ch], the words of the 32-workgroup barrier counted in doubles
static size_t shard_theta_doubles(int k, long long ch) { return ((size_t)k * (ch + SH_PAD) + 7) & ~(size_t)7; }
static size_t shard_part_doubles(long long ch) { return (size_t)(NT + SH_PAD) * ch; }
constexpr size_t SHARD_BAR_DOUBLES = 32 * 20 / 2;

// The normalisation every call goes through before it is planned and launched.  Returns SweepArgs.variate (1: U(0,1) variates).
static int normalise_call(fmcmc_model& m, fmcmc_kernel& kn) {
  // iid Normal(mu, sigma) IS the Gaussian linear model with an intercept and no covariate -- the same canonical arithmetic in
  // every kernel and in the oracle (fmcmc_oracle.c: pp = 0, icc = 1) -- so it takes that model's fast paths instead of the
  // all-family kernel (tools/option_audit.py)
  if (m.family == FMCMC_FAM_IID_NORMAL) { m.family = FMCMC_FAM_GAUSSIAN_LINREG; m.p = 0; m.intercept = 1; }
  // the uniform kernels ARE the normal kernels with mu = min., scale = max. - min. and U(0,1) variates
  if (kn.kind == FMCMC_KERNEL_UNIF) { kn.kind = FMCMC_KERNEL_NORMAL; return 1; }
  if (kn.kind == FMCMC_KERNEL_UNIF_REFLECTIVE) { kn.kind = FMCMC_KERNEL_NORMAL_REFLECTIVE; return 1; }
  return kn.kind == FMCMC_KERNEL_UMIRROR ? 1 : 0;
}

// ---- step 1: the launch arguments of the normalised call (cx.m / cx.kn), the adapt history ring and the logistic sums
static int build_sweep_args(SweepCtx& cx, fmcmc_state* st, fmcmc_out* out, int ram_bounded, SweepArgs& A) {
  memset(&A, 0, sizeof(A));
  fmcmc_model& m = cx.m;
  fmcmc_kernel& kn = cx.kn;
  A.variate = normalise_call(m, kn);
  const bool mirror = (kn.kind == FMCMC_KERNEL_NMIRROR || kn.kind == FMCMC_KERNEL_UMIRROR);
  if (mirror && (!st->mirror_mu || !st->mirror_scale || !st->obs_arate || !st->abs_iter)) {
    set_err("mirror kernels need state->mirror_mu, mirror_scale, obs_arate and abs_iter");
    return FMCMC_ERR_ARG;
  }
  if ((kn.kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE || mirror) && kn.scheme == FMCMC_SCHEME_RANDOM && cx.run->rng_mode == FMCMC_RNG_FED &&
      !st->scheme_cols) {
    set_err("rng_mode = FED with scheme = 'random' needs state->scheme_cols");
    return FMCMC_ERR_ARG;
  }
  A.nadapt = kn.nadapt; A.mirror_mu = st->mirror_mu; A.mirror_scale = st->mirror_scale; A.obs_arate = st->obs_arate;
  A.bw = (kn.kind == FMCMC_KERNEL_ADAPT) ? kn.bw : 0; A.Sd = kn.Sd;
  if (kn.kind == FMCMC_KERNEL_ADAPT && (kn.bw > 0 || kn.freq > 1)) {   // ring of the last rows of every chain (the reference reads them from env$ans)
    A.hist_rows = (kn.bw - 1 > kn.freq) ? kn.bw - 1 : kn.freq;
    const int rh = cx.scratch.grab(&A.hist, sizeof(double) * (size_t)cx.run->nchains * (size_t)A.hist_rows * (size_t)cx.kf, "adapt history");
    if (rh != FMCMC_OK) return rh;
  }
  A.family = m.family; A.p = m.p; A.intercept = m.intercept ? 1 : 0; A.guard = m.guard ? 1 : 0;
  A.n = m.n; A.X = m.X; A.y = m.y; A.prior_div = m.prior_div;
  A.fixed = kn.fixed; A.ram_bounded = ram_bounded;
  A.S = fmcmc_kept_rows(cx.run->nsteps, cx.run->burnin, cx.run->thin);
  const int rf = fill_call_args(A, &kn, cx.run, st, out, cx.kf);
  if (rf != FMCMC_OK) return rf;
  A.debug = cx.K.mode;   // timing ablations only
  // logistic family: the data-only sums of the linear part and the columns' largest |x| (logit_hs_kernel), once per launch
  return (m.family == FMCMC_FAM_LOGISTIC) ? enqueue_logit_sums(m, cx.scratch, cx.stream, &A.lg_hs) : FMCMC_OK;
}

// ---- step 3, form by form.  Each returns an FMCMC_* code (a refusal with its own message) and leaves a failed launch in cx.e.
// more than 64 parameters: one workgroup per chain, nothing to prepare; it reports on its own (no knob changes what it computes)
static int launch_bigk(SweepCtx& cx, const Route& R, const SweepArgs& A) {
  g_kernel = kernel_name(R);
  hipError_t e = launch_k(R.kfn, cx.run->nchains, NT, R.lds, cx.stream, A);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { set_err("HIP launch failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
  return FMCMC_OK;
}

// the long-data form, where the plan has it: R.form = Form::LONG when it ran; a refused cooperative launch leaves the planned form
static int try_launch_long(SweepCtx& cx, Route& R, const SweepArgs& A) {
  if (!R.kfn_long || !coop_fits(cx, R.kfn_long, R.lds_long, 256, nullptr)) return FMCMC_OK;
  const long long nchains = cx.run->nchains;
  const int nobs = 2 * R.nslots;
  const size_t n[4] = {shard_theta_doubles(cx.kn.k, nchains), shard_part_doubles(nchains), SHARD_BAR_DOUBLES, (size_t)256 * (cx.m.p + 1) * nobs};
  double* p[4];   // theta | partials | barrier | slices
  const int rc = grab_carved(cx, n, 4, p);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(long_build_slices, dim3(256), dim3(256), 0, cx.stream, cx.m.X, cx.m.y, (long long)cx.m.n, cx.m.p, R.nslots, p[3]);
  SweepArgs W = A;
  W.shard = 2; W.sh_nslots = R.nslots; W.sh_xs = p[3]; W.sh_ys = nullptr; W.sh_th = p[0]; W.sh_part = p[1]; W.sh_bar = (unsigned*)p[2];
  W.sh_long = 1; W.sh_lcg = (int)R.lcg; W.sh_mblk = (int)(R.lcg * R.lrow);
  // (all chains in one launch: at most 64.  A refusal by the runtime: nothing ran, the block waits for the end of the call)
  if (coop_chain_windows(R.kfn_long, 256, R.lds_long, W, nchains, nchains, cx.kf, W.sh_bar, n[2], cx.stream) == COOP_OK) R.form = Form::LONG;
  return FMCMC_OK;
}

// the operand-order copy of the observation slots beyond the registers (EXT / adaptive MFMA forms): 4 ng doubles per streamed
// observation -- for p = 1 several times the size of X.  When the device cannot give that memory the call still runs: on
// the chain-sharded form beneath (for these shapes the resident or the general kernel), which needs none
static void attach_mfma_stream(SweepCtx& cx, Route& R, SweepArgs& A) {
  if (!R.mfma_ng || !R.mfma_ext) return;
  const int next = R.nslots - R.mfma_ext;
  double* mfs = nullptr;
  const size_t nd = (size_t)NW * (next > 0 ? next : 1) * R.mfma_ng * 64 * 4;   // (everything resident: one slot of stand-in, read and never used)
  if (cx.scratch.grab(&mfs, sizeof(double) * nd, nullptr) != FMCMC_OK) {
    R.form = R.base; R.kfn = R.kfn_base;
    R.mfma_ng = 0; R.mfma_ext = 0; R.mfma_ad = 0; R.pipe_opt = 0;
    return;
  }
  if (next > 0) hipLaunchKernelGGL(mfma_build_stream, dim3(512), dim3(256), 0, cx.stream, cx.m.X, cx.m.y, (long long)cx.m.n, cx.m.p, R.mfma_ng, R.mfma_ext, next, mfs);
  else (void)hipMemsetAsync(mfs, 0, sizeof(double) * nd, cx.stream);
  A.mf_stream = mfs; A.mf_next = next > 0 ? next : 0;
}

// the stream of launch W into `ws`, rows = W.nsteps
static void fill_window_stream(const SweepCtx& cx, SweepArgs& W, long long step_base_eff, double* ws) {
  const size_t items = (size_t)W.nchains * (size_t)W.nsteps;
  fill_rng(cx.run->seed, step_base_eff, cx.run->chain_base, W.nchains, W.nsteps, W.kz, fill_df(W), ws, ws + items, cx.stream);
  W.fed_logu = ws; W.fed_z = ws + items; W.rng_mode = FMCMC_RNG_FED;
}

// one launch of a stream-fed form: the whole call, or one step window of it
static hipError_t launch_fast(const SweepCtx& cx, const Route& R, const SweepArgs& W) {
  const fmcmc_kernel& kn = cx.kn;
  const long long pblk = (W.nchains + 3) / 4, sblk = (W.nchains + R.spec_cw - 1) / R.spec_cw;
  // (MFMA forms: offsets from the buffer bases stay 32 bits -- the cheaper form, see mh_sweep_mfma's BIG -- while the samples of
  //  all chains and the stream of this launch stay below 4 GiB)
  const bool big = (unsigned long long)W.nchains * kn.k * (unsigned long long)W.ldS * 8ull >= (1ull << 32) ||
                   (unsigned long long)W.nchains * (unsigned long long)W.nsteps * (unsigned long long)W.kz * 8ull >= (1ull << 32);
  const int kv = (kn.kind == FMCMC_KERNEL_NORMAL) ? 1 : 2;
  switch (R.form) {
    case Form::MFMA_ADAPTIVE: return launch_k(R.kfn, pblk, NT, mfma_ad_lds_bytes(R.mfma_ad == 2), cx.stream, W);
    case Form::MFMA_STREAMED: return launch_k(fmh::k_mfma_ext(kv, R.mfma_ng, R.mfma_ext, big ? 1 : 0), pblk, NT, mfma_lds_bytes(), cx.stream, W);
    case Form::MFMA: return launch_k(fmh::k_mfma(kv, R.mfma_ng, R.nslots, big ? 1 : 0), pblk, NT, mfma_lds_bytes(), cx.stream, W);
    // the latency form (mh_lat.hpp): 1 .. 3 chains per workgroup
    case Form::LAT_LOGIT: return launch_k(R.kfn, sblk, NT, fmh::k_lat_logit_lds(), cx.stream, W);
    case Form::LAT: return launch_k(R.kfn, sblk, NT, lat_lds_bytes(), cx.stream, W);
    // the wave-specialised kernel (mh_spec.hpp): spec_cw chains per workgroup
    case Form::SPEC_LOGIT: return launch_k(R.kfn, sblk, SPEC_NT, fmh::k_spec_logit_lds(kn.kind >= FMCMC_KERNEL_ADAPT ? 1 : 0), cx.stream, W);
    default: return launch_k(R.kfn, sblk, SPEC_NT, spec_lds_bytes(R.pipe_opt, kn.kind == FMCMC_KERNEL_ADAPT || kn.kind == FMCMC_KERNEL_RAM), cx.stream, W);
  }
}

// Step windows: the normal / uniform kernels with the library's own stream.  Window 0 is an ordinary launch of the call's
// first n0 steps; every later window is a launch of w + 1 steps whose step 1 re-evaluates the state the window starts
// from (bit for bit the f0 it replaces) and whose steps 2 .. w + 1 are the call's next w steps (SweepArgs.win_cont).
// The stream of a window (rows of w + 1 steps) is filled right in front of it into ONE reused buffer of <= ~256 MiB
// (it was nchains x nsteps x (kz + 1) doubles, and the reason for the 4 GiB limit; measured at C2's shape, 1.2e5 steps:
// windows of 320 / 1344 / 8192 steps 2.17 / 2.08 / 2.05 us per step -- a window costs ~40 us of launches, refill of the
// 80 operand registers and one extra evaluation, so the buffer is as large as is reasonable, not cache-sized).  The Philox counter
// is the ABSOLUTE step, so the variates, and with them every bit of the output, do not depend on the cut
// (windows begin behind a step = 1 mod 32: the accept bitmap's words then line up).
// Round 5: kernel_adapt / kernel_ram too (R/kernel_adapt.R:118-133, R/kernel_ram.R:129-152 are ONE loop of any length).  What
// depends on the step -- `i > 2`, the mean of this call's rows before the first adaptation, eta(i, k), `i %% freq` -- reads
// the call's step (SweepArgs.step_off + the window's), the running sum of the rows travels from window to window
// (SweepArgs.win_sum), everything else (Sigma / S, the running mean, abs_iter) is the state the windows hand on anyway.
static int launch_stream_fed(SweepCtx& cx, const Route& R, const SweepArgs& A) {
  const fmcmc_run* run = cx.run;
  const bool own_stream = A.rng_mode == FMCMC_RNG_PHILOX;
  const long long win = R.win ? R.win : run->nsteps;
  const long long n0 = (R.win && run->nsteps > win + 1) ? win + 1 : run->nsteps;   // steps of window 0
  double* ws = nullptr;
  if (own_stream) {
    // materialise the canonical stream: [C][rows] log u, then [C][rows][kz] z; rows = a window's steps (or the whole call)
    const long long rows = (n0 < run->nsteps) ? win + 1 : run->nsteps;
    const size_t items = (size_t)run->nchains * (size_t)rows;
    const int rc = cx.scratch.grab(&ws, sizeof(double) * items * (size_t)(A.kz + 1), "rng stream");
    if (rc != FMCMC_OK) return rc;
  }
  long long* wcount = nullptr;                                          // accept counts of one continuation window
  double* wsum = nullptr;
  if (n0 < run->nsteps) {   // (window counts, and behind them kernel_adapt's running sums of the call's rows)
    const size_t nsum = (cx.kn.kind == FMCMC_KERNEL_ADAPT) ? (size_t)run->nchains * (size_t)cx.kf : 0;
    const int rc = cx.scratch.grab(&wcount, sizeof(long long) * (size_t)run->nchains + sizeof(double) * nsum, "window counts");
    if (rc != FMCMC_OK) return rc;
    if (nsum) wsum = reinterpret_cast<double*>(wcount + run->nchains);
  }
  SweepArgs B = A;                                                      // what every window starts from
  B.bits_stride = (run->nsteps + 31) >> 5;
  B.win_sum = wsum;
  SweepArgs W = B;                                                      // window 0
  W.nsteps = n0;
  if (own_stream) fill_window_stream(cx, W, (long long)run->step_base, ws);
  cx.e = launch_fast(cx, R, W);
  for (long long s0 = n0; s0 < run->nsteps && cx.e == hipSuccess; ) {     // continuation windows
    const long long w = (run->nsteps - s0 < win) ? run->nsteps - s0 : win;
    const long long rows_done = fmcmc_kept_rows(s0, run->burnin, run->thin);
    W = B;
    W.nsteps = w + 1;
    W.win_cont = 1;
    W.fresh = 0;                 // (kernel state: what the window before wrote back)
    W.step_off = s0 - 1;
    W.burnin = (run->burnin - s0 + 1 > 1) ? run->burnin - s0 + 1 : 1;
    W.thin_ctr0 = (s0 > run->burnin) ? (int)((s0 - run->burnin) % run->thin) : 0;
    W.samples = A.samples + rows_done;
    if (A.logpost) W.logpost = A.logpost + rows_done;
    if (A.draws) W.draws = A.draws + rows_done;
    if (A.accept_bits) W.accept_bits = A.accept_bits + ((s0 - 1) >> 5);
    W.S = A.S - rows_done;
    W.accept_count = wcount;
    fill_window_stream(cx, W, (long long)run->step_base + s0 - 1, ws);
    cx.e = launch_fast(cx, R, W);
    hipLaunchKernelGGL(add_counts_kernel, dim3((unsigned)((run->nchains + 255) / 256)), dim3(256), 0, cx.stream, A.accept_count, wcount,
                       (long long)run->nchains);
    s0 += w;
  }
  return FMCMC_OK;
}

// the logistic-only instantiations: observation-sharded (logistic-sharded / -shadow) where the plan has it and the launch is
// resident, else chain-sharded
static int launch_logistic(SweepCtx& cx, Route& R, SweepArgs& A) {
  const fmcmc_run* run = cx.run;
  if (R.form == Form::LOGISTIC_SHARDED && !coop_fits(cx, R.kfn, R.lds_run, R.nb_launch, "sharded logistic evaluation")) R.form = Form::LOGISTIC;
  if (R.form == Form::LOGISTIC_SHARDED) {
    const long long nb_launch = R.nb_launch;
    const int nslots = R.nslots, p = cx.m.p;
    // (+ 8 observations behind the last slice: the pipelined loop's scalar loads run up to three passes ahead without a clamp)
    // (mh_sweep_logit2 holds four chains per workgroup whatever cw says: tables for the larger of the two launch widths)
    const long long ch_tab = (R.ch_shadow > R.ch_launch) ? R.ch_shadow : R.ch_launch;
    const size_t nsl = (size_t)nb_launch * nslots * 2 * p;
    const size_t n[4] = {shard_theta_doubles(cx.kn.k, ch_tab), shard_part_doubles(ch_tab), SHARD_BAR_DOUBLES, nsl + 8 * (size_t)p};
    double* t[4];   // theta | partials | barrier | slices
    const int rc = grab_carved(cx, n, 4, t);
    if (rc != FMCMC_OK) return rc;
    (void)hipMemsetAsync(t[3] + nsl, 0, sizeof(double) * 8 * (size_t)p, cx.stream);
    hipLaunchKernelGGL(logit_build_slices, dim3((unsigned)nb_launch), dim3(256), 0, cx.stream, cx.m.X, (long long)cx.m.n, p, nslots, t[3]);
    A.shard = 2; A.sh_nslots = nslots; A.sh_xs = t[3]; A.sh_ys = nullptr; A.sh_th = t[0]; A.sh_part = t[1]; A.sh_bar = (unsigned*)t[2];
    A.sh_t10 = (cx.K.turn >= 0) ? cx.K.turn : 1600700;   // (logit_shard's issue-priority turn: starts at 0.700 of the younger wave's passes, regulated towards a lead of 16 x 256 cycles; knob turn)
    // Round 5: the canonical stream of the call materialised in front of the sweep (rng_fill_kernel), where it fits 1 GiB, instead
    // of being drawn inside the cooperative kernel: there the draws of a tile of steps -- Philox, AS241 with its ~50 constants
    // reloaded from scratch -- sit between two grid-wide hand-overs with 255 workgroups waiting (C5: 1.4 us of a 66 us step,
    // tools/bench_c5_fed.py).  The same variates, the same bits.
    const SweepArgs A_own = A;                       // (the call on the library's own generators: what a refusal below falls back to)
    const unsigned long long stream_bytes = (unsigned long long)run->nchains * (unsigned long long)run->nsteps * (unsigned long long)(A.kz + 1) * 8ull;
    double* wsl = nullptr;
    if (A.rng_mode == FMCMC_RNG_PHILOX && stream_bytes <= (1ull << 30) &&
        (cx.kn.kind >= FMCMC_KERNEL_ADAPT || cx.kn.scheme == FMCMC_SCHEME_JOINT) &&
        cx.scratch.grab(&wsl, (size_t)stream_bytes, nullptr) == FMCMC_OK)
      fill_window_stream(cx, A, run->step_base, wsl);
    // (variates from a stream, the library's or the caller's: the instantiation without the generators in its body, and where the
    //  plan has one the shadow form)
    const void* kfr = R.kfn;
    size_t lds_run = R.lds_run;
    long long ch_run = R.ch_launch;
    if (A.rng_mode == FMCMC_RNG_FED) {
      if (R.kfn_fed && hipFuncSetAttribute(R.kfn_fed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.lds_run) == hipSuccess) kfr = R.kfn_fed;
      else (void)hipGetLastError();
      if (R.kfn_shadow && coop_fits(cx, R.kfn_shadow, R.lds_shadow, nb_launch, nullptr)) {
        kfr = R.kfn_shadow; lds_run = R.lds_shadow; ch_run = R.ch_shadow;
        R.form = Form::LOGISTIC_SHADOW;
      }
    }
    SweepArgs Ab = A;
    Ab.bits_stride = (run->nsteps + 31) >> 5;       // (the owners of mh_spec.hpp address the accept bitmap through it)
    const CoopRun cr = coop_chain_windows(kfr, nb_launch, lds_run, Ab, run->nchains, ch_run, cx.kf, A.sh_bar, n[2], cx.stream);
    if (cr == COOP_LATER_FAILED) return FMCMC_ERR_DEVICE;
    if (cr == COOP_NOTHING_RAN) {                  // the runtime refused the first cooperative launch: the chain-sharded kernel
      R.form = Form::LOGISTIC;
      A = A_own;
      A.shard = 0; A.sh_xs = nullptr; A.sh_th = nullptr; A.sh_part = nullptr; A.sh_bar = nullptr;
    }
  }
  if (R.form == Form::LOGISTIC) cx.e = launch_k(R.kfn_base, R.nblk, NT, R.lds, cx.stream, A);
  return FMCMC_OK;
}

// wide linear models: observation-sharded (sequential, matrix-core or dataflow form) where the plan has it and the launch is
// resident, else chain-sharded
static int launch_wide(SweepCtx& cx, Route& R, SweepArgs& A) {
  if (R.wide2) { A.sh_ngrp = R.ngrp; A.sh_tiles = R.tiles; }
  if (R.form != Form::WIDE && !coop_fits(cx, R.kfn, R.lds_run, R.nb_launch, "sharded evaluation")) R.form = Form::WIDE;
  if (R.form != Form::WIDE) {
    const long long nb_launch = R.nb_launch, ch_launch = R.ch_launch;
    const int p = cx.m.p;
    const bool mfma_form = R.mfma_form;
    const size_t n[6] = {mfma_form ? 0 : (size_t)nb_launch * p * SH_MAXO, mfma_form ? 0 : (size_t)nb_launch * SH_MAXO,
                         shard_theta_doubles(cx.kn.k, ch_launch), shard_part_doubles(ch_launch),
                         R.wide2 ? (size_t)(8 * W2_BARW / 2) : SHARD_BAR_DOUBLES,   // (barrier words counted in doubles)
                         mfma_form ? (size_t)nb_launch * R.mblk : 0};
    double* t[6];   // xs | ys | theta | partials | barrier | mfma
    const int rc = grab_carved(cx, n, 6, t);
    if (rc != FMCMC_OK) return rc;
    if (!mfma_form)
      hipLaunchKernelGGL(shard_build_slices, dim3((unsigned)nb_launch), dim3(256), 0, cx.stream, cx.m.X, cx.m.y, (long long)cx.m.n, p, R.lpw, R.nslots, t[0], t[1]);
    A.shard = R.lpw; A.sh_nslots = R.nslots; A.sh_xs = t[0]; A.sh_ys = t[1]; A.sh_th = t[2]; A.sh_part = t[3]; A.sh_bar = (unsigned*)t[4];
    if (mfma_form) {
      hipLaunchKernelGGL(shard_build_mfma, dim3((unsigned)nb_launch), dim3(256), 0, cx.stream, cx.m.X, cx.m.y, (long long)cx.m.n, p, R.lpw, R.nslots,
                         R.nmt, R.t10, t[5], R.mblk);
      A.sh_mfma = t[5]; A.sh_mblk = R.mblk; A.sh_nmt = R.nmt; A.sh_t10 = R.t10;
    }
    const CoopRun cr = coop_chain_windows(R.kfn, nb_launch, R.lds_run, A, cx.run->nchains, ch_launch, cx.kf, A.sh_bar, n[4], cx.stream);
    if (cr == COOP_LATER_FAILED) return FMCMC_ERR_DEVICE;
    if (cr == COOP_NOTHING_RAN) {                  // the runtime refused the first cooperative launch: the chain-sharded kernel
      R.form = Form::WIDE;
      A.shard = 0; A.sh_xs = nullptr; A.sh_ys = nullptr; A.sh_th = nullptr; A.sh_part = nullptr; A.sh_bar = nullptr;
      A.sh_mfma = nullptr; A.sh_mblk = 0; A.sh_nmt = 0; A.sh_t10 = 0;
    }
  }
  if (R.form == Form::WIDE) cx.e = launch_k(R.kfn_base, R.nblk, NT, R.lds, cx.stream, A);
  return FMCMC_OK;
}

// Executes one call: the arguments, the plan, the planned form's launcher, the report.
static int launch_sweep(const fmcmc_model* m_in, const fmcmc_kernel* kn_in, const fmcmc_run* run,
                        fmcmc_state* st, fmcmc_out* out, int kf, int ram_bounded, hipStream_t stream) {
  SweepCtx cx(m_in, kn_in, run, kf, stream);
  SweepArgs A;
  int rc = build_sweep_args(cx, st, out, ram_bounded, A);
  if (rc != FMCMC_OK) return rc;
  // ---- launch geometry and the plan
  (void)hipGetDevice(&cx.dev);
  (void)hipDeviceGetAttribute(&cx.ncu, hipDeviceAttributeMultiprocessorCount, cx.dev);
  if (cx.ncu <= 0) cx.ncu = 256;
  rc = require_gfx950(cx.dev);
  if (rc != FMCMC_OK) return rc;
  Route R = plan_route(&cx.m, &cx.kn, run, kf, ram_bounded, A.kz, A.ldS, cx.ncu, cx.K);
  if (R.lds_exceeded) { set_err("LDS budget exceeded (k=%d)", cx.kn.k); return FMCMC_ERR_UNSUPPORTED; }
  if (R.no_kernel) { set_err("no device kernel for the %s form (k=%d)", kernel_name(R), cx.kn.k); return FMCMC_ERR_DEVICE; }
  if (R.form == Form::BIGK || R.form == Form::BIGK_HBM) return launch_bigk(cx, R, A);
  A.tb = R.tb;
  A.spec_opt = R.pipe_opt;
  A.spec_cw = R.spec_cw;
  A.nsteps_call = run->nsteps;
  // ---- the planned form (the long-data form first, where the plan has it)
  rc = try_launch_long(cx, R, A);
  if (rc == FMCMC_OK && R.form != Form::LONG) {
    attach_mfma_stream(cx, R, A);
    if (stream_fed(R.form)) rc = launch_stream_fed(cx, R, A);
    else if (R.base == Form::LOGISTIC) rc = launch_logistic(cx, R, A);
    else if (R.base == Form::WIDE) rc = launch_wide(cx, R, A);
    else cx.e = launch_k(R.kfn, R.nblk, NT, R.lds, cx.stream, A);   // resident / general kernel
  }
  if (rc != FMCMC_OK) return rc;
  // ---- the report
  g_kernel = kernel_name(R);
  hipError_t e = cx.e;
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { set_err("HIP launch failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
  // timing ablations and stamps (knob mode=<bits>: 8 stamps in the draws buffer, 32 / 64 / 128 / 1024 parts of a step left out)
  // produce INVALID samples: a call made with one of them says so in fmcmc_last_kernel(), so that its results cannot pass for
  // a product run's
  if (cx.K.mode & (8 | 32 | 64 | 128 | 1024)) {
    static thread_local char kbuf[96];
    snprintf(kbuf, sizeof(kbuf), "invalid-results(mode=%d):%s", cx.K.mode, g_kernel);
    g_kernel = kbuf;
  }
  return FMCMC_OK;
}


// ==============================================================================================
// user-defined log-posteriors: the sweep around a batched callback (fmcmc_logpost_fn; mh_fun.hpp)
// ==============================================================================================
// The call: every pointer of kn / run / st / out is a DEVICE pointer (fx, lb, ub: host copies of the kernel's).  host_fun: `fun`
// takes host buffers (the theta1 of every chain is copied out and f(theta1) back in around each evaluation).
static int run_fun(const fmcmc_kernel* kn, const uint8_t* fx, const double* lb, const double* ub, const fmcmc_run* run,
                   fmcmc_state* st, fmcmc_out* out, fmcmc_logpost_fn fun, void* user, hipStream_t stream, bool host_fun) {
  if (!fun) { set_err("null log-posterior callback"); return FMCMC_ERR_ARG; }
  const int k = kn->k, kf = count_free(kn, fx);
  const long long C = run->nchains;
  const bool adapt = kn->kind == FMCMC_KERNEL_ADAPT, ram = kn->kind == FMCMC_KERNEL_RAM;
  if ((adapt || ram) && (!st->Sigma || !st->abs_iter || (adapt && (!st->mean_prev || !st->have_mean)))) {
    set_err("kernel_adapt / kernel_ram need state->Sigma and abs_iter (kernel_adapt: mean_prev and have_mean as well)");
    return FMCMC_ERR_ARG;
  }
  if (is_simple_kind(kn->kind) && kn->scheme == FMCMC_SCHEME_RANDOM && run->rng_mode == FMCMC_RNG_FED && !st->scheme_cols) {
    set_err("rng_mode = FED with scheme = 'random' needs state->scheme_cols");
    return FMCMC_ERR_ARG;
  }
  const int bounded = any_bounded(fx, lb, ub, k);
  FunArgs A;
  memset(&A, 0, sizeof(A));
  A.kf = kf; A.ram_bounded = ram ? bounded : 0;
  int rc = fill_call_args(A, kn, run, st, out, kf);
  if (rc != FMCMC_OK) return rc;
  int dev = 0;
  (void)hipGetDevice(&dev);
  rc = require_gfx950(dev);
  if (rc != FMCMC_OK) return rc;
  // scratch of the call: theta1 [C][k] and f(theta1) [C] (what `fun` reads and writes), kernel_adapt's running row sum [C][kf],
  // nerrors [C] when the caller keeps none, the free-parameter list [kf]
  const size_t n_th = (size_t)C * k, n_rs = adapt ? (size_t)C * kf : 0, n_ne = ((adapt || ram) && !st->nerrors) ? (size_t)C : 0;
  const size_t bytes = sizeof(double) * (n_th + (size_t)C + n_rs) + sizeof(int) * (n_ne + (size_t)kf);
  ScratchList scratch(stream);
  double* th1 = nullptr;
  if (scratch.grab(&th1, bytes, nullptr) != FMCMC_OK) {
    set_err("hipMallocAsync(%zu) for the callback sweep failed", bytes);
    return FMCMC_ERR_DEVICE;
  }
  double* f1 = th1 + n_th;
  A.rsum = adapt ? f1 + C : nullptr;
  int* ne = (int*)(f1 + C + n_rs);
  int* which = ne + n_ne;
  if (n_ne) { A.nerrors = ne; (void)hipMemsetAsync(ne, 0, sizeof(int) * n_ne, stream); }
  A.which = which; A.th1 = th1; A.f1 = f1;
  hipLaunchKernelGGL(fun_which_kernel, dim3(1), dim3(64), 0, stream, kn->fixed, k, which);
  (void)hipMemcpyAsync(th1, st->theta0, sizeof(double) * n_th, hipMemcpyDeviceToDevice, stream);   // row 1: f(initial)

  const int nth = (k <= FMCMC_MAX_K_WAVE) ? 64 : 256;
  const void* kfn = fmh::k_fun(nth);
  const size_t lds = sizeof(double) * fun_lds_doubles(k, kf, kn->kind, nth);
  if (!kfn) { set_err("no device kernel for the callback sweep (k=%d)", k); return FMCMC_ERR_DEVICE; }
  if (lds > 48 * 1024 && hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    set_err("LDS budget exceeded (k=%d)", k);
    return FMCMC_ERR_UNSUPPORTED;
  }
  g_kernel = (nth == 64) ? "fun" : "fun-wg";
  std::vector<double> h_th, h_f;
  if (host_fun) { h_th.resize(n_th); h_f.resize((size_t)C); }
  auto evaluate = [&](long long step) -> int {
    if (!host_fun) return call_logpost(fun, th1, C, k, f1, stream, user, step);
    if (hipMemcpyAsync(h_th.data(), th1, sizeof(double) * n_th, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
      set_err("cannot read the proposals of loop step i = %lld back from the device", step);
      return FMCMC_ERR_DEVICE;
    }
    const int rc = call_logpost(fun, h_th.data(), C, k, h_f.data(), stream, user, step);
    if (rc == FMCMC_OK && hipMemcpyAsync(f1, h_f.data(), sizeof(double) * (size_t)C, hipMemcpyHostToDevice, stream) != hipSuccess) {
      set_err("cannot copy the log-posterior of loop step i = %lld to the device", step);
      return FMCMC_ERR_DEVICE;
    }
    return rc;
  };
  auto launch = [&](long long step, int phase) -> int {
    A.step = step; A.phase = phase;
    return launch_step(kfn, C, nth, lds, stream, A, step);
  };
  const long long nsteps = run->nsteps;
  rc = evaluate(1);
  if (rc == FMCMC_OK) rc = launch(1, FPH_START | (nsteps >= 2 ? FPH_PROPOSE : FPH_FINISH));
  for (long long i = 2; i <= nsteps && rc == FMCMC_OK; i++) {
    const int tail = (i < nsteps ? FPH_PROPOSE : FPH_FINISH);
    rc = evaluate(i);
    if (rc != FMCMC_OK) break;
    if (ram && bounded) {   // f(un-reflected theta1) for the adaptation, then f(theta1) (R/kernel_ram.R:129-152)
      rc = launch(i, FPH_RAM);
      if (rc == FMCMC_OK) rc = evaluate(i);
      if (rc == FMCMC_OK) rc = launch(i, FPH_ACCEPT | tail);
    } else {
      rc = launch(i, (ram ? FPH_RAM : 0) | FPH_ACCEPT | tail);
    }
  }
  return rc;
}


// ==============================================================================================
// user-defined transition kernels: the step cut at the proposal as well (fmcmc_proposal_fn / fmcmc_logratio_fn; mh_user.hpp)
// ==============================================================================================
// the model of an evaluation: its family, its shape and the pointers logpost_eval_kernel reads
static int check_eval_model(const fmcmc_model* m) {
  const int k = eval_params(m->family, m->p, m->intercept);
  if (k < 0) { set_err("unknown log-posterior family %d", m->family); return FMCMC_ERR_ARG; }
  if (m->p < 0 || k < 1 || k > FMCMC_MAX_K) { set_err("number of parameters k=%d outside [1, %d]", k, FMCMC_MAX_K); return FMCMC_ERR_UNSUPPORTED; }
  if (m->n < 1) { set_err("the model needs at least one observation"); return FMCMC_ERR_ARG; }
  if (!m->y || (m->p > 0 && m->family != FMCMC_FAM_IID_NORMAL && !m->X)) { set_err("the model's data pointers are null"); return FMCMC_ERR_ARG; }
  return FMCMC_OK;
}

// The families' evaluator at caller-given points: prepare() once per call of an entry point (the logistic sums, into the call's
// scratch), enqueue() per batch of C parameter vectors.
struct EvalCall {
  EvalArgs E;
  const void* kfn = nullptr;
  int prepare(const fmcmc_model* m, ScratchList& scratch, hipStream_t stream) {
    memset(&E, 0, sizeof(E));
    E.family = m->family; E.p = m->p; E.intercept = m->intercept ? 1 : 0; E.guard = m->guard ? 1 : 0;
    E.n = m->n; E.prior_div = m->prior_div; E.X = m->X; E.y = m->y;
    kfn = fmh::k_logpost_eval();
    if (!kfn) { set_err("no device kernel for the batched evaluation"); return FMCMC_ERR_DEVICE; }
    return (m->family == FMCMC_FAM_LOGISTIC) ? enqueue_logit_sums(*m, scratch, stream, &E.hs) : FMCMC_OK;
  }
  hipError_t enqueue(const double* theta, long long C, double* out, hipStream_t stream) {
    E.theta = theta; E.nchains = C; E.out = out;
    void* kargs[] = {(void*)&E};
    hipError_t e = hipLaunchKernel(kfn, dim3((unsigned)C), dim3(NT), kargs, 0, stream);
    return e == hipSuccess ? hipGetLastError() : e;
  }
};

// run_fun's loop with the proposal outside (R/mcmc.R:737-783).  Every pointer of run / st / out is a DEVICE pointer.
static int run_user(const fmcmc_model* m, fmcmc_logpost_fn fun, fmcmc_proposal_fn proposal, fmcmc_logratio_fn logratio, void* user,
                    int k, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out, hipStream_t stream) {
  const long long C = run->nchains, nsteps = run->nsteps;
  UserArgs A;
  memset(&A, 0, sizeof(A));
  int rc = fill_run_args(A, k, run, st, out);
  if (rc != FMCMC_OK) return rc;
  int dev = 0;
  (void)hipGetDevice(&dev);
  rc = require_gfx950(dev);
  if (rc != FMCMC_OK) return rc;
  // scratch of the call: two theta1 [C][k] (the proposal callback reads the last proposal while it writes the new one),
  // f(theta1) [C], the caller's log-ratio [C]
  const size_t n_th = (size_t)C * k, bytes = sizeof(double) * (2 * n_th + (size_t)C * (logratio ? 2 : 1));
  ScratchList scratch(stream);
  double* thb[2] = {nullptr, nullptr};
  if (scratch.grab(&thb[0], bytes, nullptr) != FMCMC_OK) {
    set_err("hipMallocAsync(%zu) for the user-kernel sweep failed", bytes);
    return FMCMC_ERR_DEVICE;
  }
  thb[1] = thb[0] + n_th;
  double* f1 = thb[1] + n_th;
  double* lr = logratio ? f1 + C : nullptr;
  EvalCall ev;
  if (m) {
    rc = ev.prepare(m, scratch, stream);
    if (rc != FMCMC_OK) return rc;
  }
  const int nth = (k <= FMCMC_MAX_K_WAVE) ? 64 : 256;
  const void* kfn = fmh::k_user(nth);
  if (!kfn) { set_err("no device kernel for the user-kernel sweep (k=%d)", k); return FMCMC_ERR_DEVICE; }
  g_kernel = (nth == 64) ? "user" : "user-wg";
  auto evaluate = [&](const double* th, long long step) -> int {
    if (m) {
      const hipError_t e = ev.enqueue(th, C, f1, stream);
      if (e != hipSuccess) { set_err("HIP launch failed at loop step i = %lld: %s", step, hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
      return FMCMC_OK;
    }
    return call_logpost(fun, th, C, k, f1, stream, user, step);
  };
  auto launch = [&](const double* th, long long step, int phase) -> int {
    A.th1 = th; A.f1 = f1; A.logratio = (phase == UPH_ACCEPT) ? lr : nullptr; A.step = step; A.phase = phase;
    return launch_step(kfn, C, nth, 0, stream, A, step);
  };
  // row 1: f0 = f(initial), theta1 = theta0 and f1 = f0, as the reference initialises them
  (void)hipMemcpyAsync(thb[0], st->theta0, sizeof(double) * n_th, hipMemcpyDeviceToDevice, stream);
  rc = evaluate(thb[0], 1);
  if (rc == FMCMC_OK) rc = launch(thb[0], 1, UPH_START);
  fmcmc_step_env env;
  memset(&env, 0, sizeof(env));
  env.nsteps = nsteps; env.nchains = C; env.chain_base = run->chain_base; env.step_base = run->step_base; env.k = k;
  env.theta0 = st->theta0; env.f0 = st->f0; env.f1 = f1; env.status = out->status;
  int cur = 0;   // the buffer that holds the last proposal
  for (long long i = 2; i <= nsteps && rc == FMCMC_OK; i++) {
    double* next = thb[cur ^ 1];
    env.i = i; env.theta1 = thb[cur];
    int rp = proposal(&env, next, (void*)stream, user);
    if (rp != 0) { set_err("the proposal callback returned %d at loop step i = %lld", rp, i); return FMCMC_ERR_FUN; }
    cur ^= 1;
    env.theta1 = next;
    rc = evaluate(next, i);
    if (rc != FMCMC_OK) break;
    if (logratio) {
      rp = logratio(&env, lr, (void*)stream, user);
      if (rp != 0) { set_err("the logratio callback returned %d at loop step i = %lld", rp, i); return FMCMC_ERR_FUN; }
    }
    rc = launch(next, i, UPH_ACCEPT);
  }
  return rc;
}


// ==============================================================================================
// one model on many datasets: the callback sweep with the family's evaluation fused in, one launch (mh_batch.hpp)
// ==============================================================================================
// strides of a batch, checked before any device call (fmcmc_validate_batch has no strides to check)
static int check_batch_strides(const fmcmc_model* m, int64_t x_stride, int64_t y_stride) {
  const long long need_x = (m->family == FMCMC_FAM_IID_NORMAL || m->p < 1) ? 0 : (long long)m->p * m->n;
  if (x_stride < need_x || y_stride < m->n) {
    set_err("the strides of the batch (x_stride = %lld, y_stride = %lld doubles) are smaller than a dataset (p n = %lld, n = %lld)",
            (long long)x_stride, (long long)y_stride, need_x, (long long)m->n);
    return FMCMC_ERR_ARG;
  }
  if (!m->y || (need_x > 0 && !m->X)) { set_err("the model's data pointers are null"); return FMCMC_ERR_ARG; }
  return FMCMC_OK;
}

// The call: every pointer of m / kn / run / st / out is a DEVICE pointer (fx, lb, ub: host copies of the kernel's); active: the
// device mask [D] of the datasets that run, or NULL for all of them
static int run_batch(const fmcmc_model* m, long long D, long long x_stride, long long y_stride, const fmcmc_kernel* kn, const uint8_t* fx,
                     const double* lb, const double* ub, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out, const int32_t* active,
                     uint32_t flags, hipStream_t stream) {
  const int k = kn->k, kf = count_free(kn, fx);
  const long long C = run->nchains;
  const bool adapt = kn->kind == FMCMC_KERNEL_ADAPT, ram = kn->kind == FMCMC_KERNEL_RAM, logit = m->family == FMCMC_FAM_LOGISTIC;
  if (!st->theta0 || !st->f0) { set_err("a batch needs state->theta0 and f0"); return FMCMC_ERR_ARG; }
  if ((adapt || ram) && (!st->Sigma || !st->abs_iter || (adapt && (!st->mean_prev || !st->have_mean)))) {
    set_err("kernel_adapt / kernel_ram need state->Sigma and abs_iter (kernel_adapt: mean_prev and have_mean as well)");
    return FMCMC_ERR_ARG;
  }
  if (is_simple_kind(kn->kind) && kn->scheme == FMCMC_SCHEME_RANDOM && run->rng_mode == FMCMC_RNG_FED && !st->scheme_cols) {
    set_err("rng_mode = FED with scheme = 'random' needs state->scheme_cols");
    return FMCMC_ERR_ARG;
  }
  BatchArgs B;
  memset(&B, 0, sizeof(B));
  B.F.kf = kf; B.F.ram_bounded = ram ? any_bounded(fx, lb, ub, k) : 0;
  int rc = fill_call_args(B.F, kn, run, st, out, kf);
  if (rc != FMCMC_OK) return rc;
  B.family = m->family; B.p = m->p; B.intercept = m->intercept ? 1 : 0; B.guard = m->guard ? 1 : 0;
  B.n = m->n; B.prior_div = m->prior_div; B.X = m->X; B.y = m->y;
  B.x_stride = x_stride; B.y_stride = y_stride; B.hs_stride = 2 * MAXK + 2; B.chains_per_model = C / D;
  B.active = active;
  int dev = 0;
  (void)hipGetDevice(&dev);
  rc = require_gfx950(dev);
  if (rc != FMCMC_OK) return rc;
  // scratch of the call: the logistic sums [D][2 MAXK + 2], nerrors [C] when the caller keeps none, the free-parameter list [kf]
  const size_t n_hs = logit ? (size_t)D * (size_t)B.hs_stride : 0, n_ne = ((adapt || ram) && !st->nerrors) ? (size_t)C : 0;
  ScratchList scratch(stream);
  double* hs = nullptr;
  rc = scratch.grab(&hs, sizeof(double) * n_hs + sizeof(int) * (n_ne + (size_t)kf), "the batch's scratch");
  if (rc != FMCMC_OK) return rc;
  int* ne = (int*)(hs + n_hs);
  int* which = ne + n_ne;
  if (n_ne) { B.F.nerrors = ne; (void)hipMemsetAsync(ne, 0, sizeof(int) * n_ne, stream); }
  B.F.which = which;
  hipLaunchKernelGGL(fun_which_kernel, dim3(1), dim3(64), 0, stream, kn->fixed, k, which);
  if (logit) {
    B.hs = hs;
    hipLaunchKernelGGL(logit_hs_batch_kernel, dim3((unsigned)D), dim3(NT), 0, stream, m->X, m->y, (long long)m->n, m->p, B.intercept, hs,
                       x_stride, y_stride, B.hs_stride);
  }
  const bool lds_data = !(flags & FMCMC_BATCH_STREAM_DATA) && batch_data_in_lds(m->family, m->n, m->p, kf, kn->kind);
  const void* kfn = fmh::k_batch(lds_data, active != nullptr);
  if (!kfn) { set_err("no device kernel for the batch sweep"); return FMCMC_ERR_DEVICE; }
  const size_t lds = sizeof(double) * (batch_step_doubles(k, kf, kn->kind) + (lds_data ? batch_data_doubles(m->family, m->n, m->p) : 0));
  if (lds > 48 * 1024 && hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    set_err("LDS budget exceeded (k=%d, n=%lld, p=%d)", k, (long long)m->n, m->p);
    return FMCMC_ERR_UNSUPPORTED;
  }
  g_kernel = lds_data ? "batch-lds" : "batch-stream";
  void* kargs[] = {(void*)&B};
  hipError_t e = hipLaunchKernel(kfn, dim3((unsigned)C), dim3(NT), kargs, lds, stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { set_err("HIP launch of the batch sweep failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
  return FMCMC_OK;
}


#include "mh_host.hpp"   // (the staging of the *_host entry points)

extern "C" {

int fmcmc_rng_stream_dev(uint64_t seed, int64_t step_base, int64_t chain_base, int64_t nchains, int64_t nsteps,
                         int32_t kz, double student_df, double* logu, double* z, void* hip_stream) {
  if (!logu || !z || nchains < 1 || nsteps < 1 || kz < 1) { set_err("fmcmc_rng_stream_dev: bad argument"); return FMCMC_ERR_ARG; }
  fill_rng(seed, step_base, chain_base, nchains, nsteps, kz, student_df, logu, z, (hipStream_t)hip_stream);
  return hipGetLastError() == hipSuccess ? FMCMC_OK : FMCMC_ERR_DEVICE;
}

int fmcmc_detmath_dev(int which, const double* x, double* out, int64_t n, uint64_t seed, void* hip_stream) {
  if (n <= 0) return FMCMC_OK;
  hipLaunchKernelGGL(detmath_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                     which, x, out, (long long)n, (unsigned long long)seed);
  return hipGetLastError() == hipSuccess ? FMCMC_OK : FMCMC_ERR_DEVICE;
}

// The host build of the same text, for the codes whose host twin is not in the CPU oracle (11, 12: fmh_pnorm_both).
int fmcmc_detmath_host(int which, const double* x, double* out, int64_t n) {
  if (which != 11 && which != 12) { set_err("fmcmc_detmath_host: which = %d; 11 (Phi) or 12 (1 - Phi)", which); return FMCMC_ERR_ARG; }
  if (n > 0 && (!x || !out)) { set_err("fmcmc_detmath_host: null argument"); return FMCMC_ERR_ARG; }
  for (int64_t i = 0; i < n; i++) {
    double lo, up;
    fmh_pnorm_both(x[i], &lo, &up);
    out[i] = which == 11 ? lo : up;
  }
  return FMCMC_OK;
}

// The kernel arrays the host side needs (fixed, lb, ub; scale of the uniform kernels; scheme_seq) and a copy of the kernel
// pointing at them.  `fixed`, `lb`, `ub` (and scale / scheme_seq where they are checked) live on the device.  A caller that
// passes their host copies (fmcmc_kernel.h_*) gets a call that only enqueues work; otherwise the few bytes are read back,
// which synchronises `stream` (fmcmc_mcmc_run_dev's rule).
struct KernelHostView {
  uint8_t fx[MAXK];
  double lb[MAXK], ub[MAXK], sc[MAXK];
  int32_t seq[MAXK];
  fmcmc_kernel kh;
};
static int kernel_host_view(const fmcmc_kernel* kn, hipStream_t stream, KernelHostView* v) {
  if (kn->k < 1 || kn->k > MAXK) { set_err("k=%d outside [1,%d]", kn->k, MAXK); return FMCMC_ERR_UNSUPPORTED; }
  const bool unif = (kn->kind == FMCMC_KERNEL_UNIF || kn->kind == FMCMC_KERNEL_UNIF_REFLECTIVE);
  const bool expl = (is_simple_kind(kn->kind) && kn->scheme == FMCMC_SCHEME_EXPLICIT && kn->scheme_seq &&
                     kn->scheme_len >= 1 && kn->scheme_len <= MAXK);
  const bool mirrored = kn->h_fixed && kn->h_lb && kn->h_ub && (!unif || kn->h_scale) && (!expl || kn->h_scheme_seq);
  if (mirrored) {
    memcpy(v->fx, kn->h_fixed, (size_t)kn->k);
    memcpy(v->lb, kn->h_lb, sizeof(double) * (size_t)kn->k);
    memcpy(v->ub, kn->h_ub, sizeof(double) * (size_t)kn->k);
    if (unif) memcpy(v->sc, kn->h_scale, sizeof(double) * (size_t)kn->k);
    if (expl) memcpy(v->seq, kn->h_scheme_seq, sizeof(int32_t) * (size_t)kn->scheme_len);
  } else if (hipMemcpyAsync(v->fx, kn->fixed, kn->k, hipMemcpyDeviceToHost, stream) != hipSuccess ||
             hipMemcpyAsync(v->lb, kn->lb, kn->k * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
             hipMemcpyAsync(v->ub, kn->ub, kn->k * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
             (unif && hipMemcpyAsync(v->sc, kn->scale, kn->k * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
             (expl && hipMemcpyAsync(v->seq, kn->scheme_seq, kn->scheme_len * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
             hipStreamSynchronize(stream) != hipSuccess) {
    set_err("cannot read kernel parameters from device memory");
    return FMCMC_ERR_DEVICE;
  }
  v->kh = *kn;
  v->kh.fixed = v->fx; v->kh.lb = v->lb; v->kh.ub = v->ub;
  v->kh.scale = unif ? v->sc : nullptr;
  v->kh.scheme_seq = expl ? v->seq : nullptr;
  return FMCMC_OK;
}

int fmcmc_mcmc_run_dev(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run,
                       fmcmc_state* st, fmcmc_out* out, void* hip_stream) {
  if (!m || !kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  hipStream_t stream = (hipStream_t)hip_stream;
  KernelHostView v;
  int rc = kernel_host_view(kn, stream, &v);
  if (rc != FMCMC_OK) return rc;
  rc = fmcmc_validate(m, &v.kh, run);
  if (rc != FMCMC_OK) return rc;
  return launch_sweep(m, kn, run, st, out, count_free(kn, v.fx), any_bounded(v.fx, v.lb, v.ub, kn->k), stream);
}

int fmcmc_mcmc_run_host(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run,
                        fmcmc_state* st, fmcmc_out* out, int device) {
  if (!m || !kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  const int rv = fmcmc_validate(m, kn, run);
  if (rv != FMCMC_OK) return rv;
  if (fmcmc_device_count() < 1) { set_err("no HIP device: the engine has no CPU fallback"); return FMCMC_ERR_DEVICE; }
  HostStage H(kn, run, st, out);
  if (out->ld_rows != 0 && out->ld_rows != (int64_t)H.S) { set_err("fmcmc_out.ld_rows is honoured by fmcmc_mcmc_run_dev only (host buffers are dense)"); return FMCMC_ERR_ARG; }
  H.open(device);
  fmcmc_model dm = *m;
  if (m->p > 0) H.up(&dm.X, m->X, sizeof(double) * (size_t)m->p * m->n);
  H.up(&dm.y, m->y, sizeof(double) * (size_t)m->n);
  stage_call(H, kn, run, st, out);
  if (H.rc == FMCMC_OK) H.rc = launch_sweep(&dm, &H.dk, &H.dr, &H.ds, &H.dout, H.kf, any_bounded(kn->fixed, kn->lb, kn->ub, H.k), H.stream);
  return fetch_call(H, kn, run, st, out);
}

// Diagnostic, no device call and no allocation: the route plan_route gives a call, as one line of key=value fields of Route.
// `kn` holds HOST pointers, as for fmcmc_mcmc_run_host; ncu: the compute units to plan for.
int fmcmc_plan_route(const fmcmc_model* m_in, const fmcmc_kernel* kn_in, const fmcmc_run* run, int64_t ld_rows, int32_t ncu,
                     char* text, size_t text_len) {
  if (!text || text_len < 1) { set_err("null argument"); return FMCMC_ERR_ARG; }
  text[0] = 0;
  const int rv = fmcmc_validate(m_in, kn_in, run);
  if (rv != FMCMC_OK) return rv;
  if (!kn_in->fixed || !kn_in->lb || !kn_in->ub) { set_err("kernel arrays lb, ub and fixed are required"); return FMCMC_ERR_ARG; }
  const int kf = count_free(kn_in, kn_in->fixed), bounded = any_bounded(kn_in->fixed, kn_in->lb, kn_in->ub, kn_in->k);
  fmcmc_model m = *m_in;
  fmcmc_kernel kn = *kn_in;
  normalise_call(m, kn);
  const long long S = fmcmc_kept_rows(run->nsteps, run->burnin, run->thin);
  const Route R = plan_route(&m, &kn, run, kf, bounded, variates_per_step(&kn, kf), ld_rows > 0 ? ld_rows : S, ncu > 0 ? ncu : 256, read_knobs());
  Route B = R; B.form = R.base;
  const int len = snprintf(text, text_len,
      "form=%s base=%s kfn=%d kfn_base=%d lds=%zu lds_run=%zu lds_exceeded=%d no_kernel=%d cw=%d tb=%d res_p=%d nblk=%lld wide_switched=%d "
      "pipe_opt=%d spec_cw=%d mfma_ng=%d mfma_ext=%d mfma_ad=%d kx=%d ring=%d win=%lld nb_launch=%lld ch_launch=%lld nslots=%d "
      "kfn_fed=%d kfn_shadow=%d lds_shadow=%zu ch_shadow=%lld lpw=%d nmt=%d t10=%d mblk=%d ngrp=%d tiles=%d mfma_form=%d wide2=%d "
      "kfn_long=%d lds_long=%zu lcg=%lld lrow=%lld",
      kernel_name(R), kernel_name(B), R.kfn != nullptr, R.kfn_base != nullptr, R.lds, R.lds_run, (int)R.lds_exceeded, (int)R.no_kernel, R.cw, R.tb,
      R.res_p, R.nblk, (int)R.wide_switched, R.pipe_opt, R.spec_cw, R.mfma_ng, R.mfma_ext, R.mfma_ad, R.kx, (int)R.ring, R.win, R.nb_launch,
      R.ch_launch, R.nslots, R.kfn_fed != nullptr, R.kfn_shadow != nullptr, R.lds_shadow, R.ch_shadow, R.lpw, R.nmt, R.t10, R.mblk, R.ngrp,
      R.tiles, (int)R.mfma_form, (int)R.wide2, R.kfn_long != nullptr, R.lds_long, R.lcg, R.lrow);
  if (len < 0 || (size_t)len >= text_len) { set_err("fmcmc_plan_route: the text buffer holds %zu bytes, the route needs %d", text_len, len + 1); return FMCMC_ERR_ARG; }
  return FMCMC_OK;
}

int fmcmc_validate_fun(const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (!kn || !run) { set_err("null argument"); return FMCMC_ERR_ARG; }
  const int rr = validate_run(kn, run);
  if (rr != FMCMC_OK) return rr;
  if (kn->kind == FMCMC_KERNEL_NMIRROR || kn->kind == FMCMC_KERNEL_UMIRROR) {
    set_err("a user-defined -fun- runs with kernel_normal(_reflective), kernel_unif(_reflective), kernel_adapt(bw = 0, freq = 1) "
            "and kernel_ram; the mirror kernels are not supported on this path");
    return FMCMC_ERR_UNSUPPORTED;
  }
  if (kn->kind == FMCMC_KERNEL_ADAPT && (kn->bw > 0 || kn->freq > 1)) {
    set_err("a user-defined -fun- runs kernel_adapt with bw = 0 and freq = 1 only (got bw=%d, freq=%d): the windowed and the "
            "strided adaptation are not supported on this path", kn->bw, kn->freq);
    return FMCMC_ERR_UNSUPPORTED;
  }
  return validate_kernel(kn, run);
}

int fmcmc_mcmc_run_fun_dev(const fmcmc_kernel* kn, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out,
                           fmcmc_logpost_fn fun, void* user, void* hip_stream) {
  if (!kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  hipStream_t stream = (hipStream_t)hip_stream;
  KernelHostView v;
  int rc = kernel_host_view(kn, stream, &v);
  if (rc != FMCMC_OK) return rc;
  rc = fmcmc_validate_fun(&v.kh, run);
  if (rc != FMCMC_OK) return rc;
  return run_fun(kn, v.fx, v.lb, v.ub, run, st, out, fun, user, stream, false);
}

int fmcmc_mcmc_run_fun_host(const fmcmc_kernel* kn, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out,
                            fmcmc_logpost_fn fun, void* user, int device) {
  if (!kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  const int rv = fmcmc_validate_fun(kn, run);
  if (rv != FMCMC_OK) return rv;
  if (!kn->fixed || !kn->lb || !kn->ub || !kn->mu || !kn->scale) { set_err("kernel arrays mu, scale, lb, ub and fixed are required"); return FMCMC_ERR_ARG; }
  if (fmcmc_device_count() < 1) { set_err("no HIP device: the engine has no CPU fallback"); return FMCMC_ERR_DEVICE; }
  HostStage H(kn, run, st, out);
  if (H.adaptive && (!st->Sigma || !st->abs_iter || !st->mean_prev || !st->have_mean)) {
    set_err("kernel_adapt / kernel_ram need state->Sigma, abs_iter, mean_prev and have_mean");
    return FMCMC_ERR_ARG;
  }
  if (out->ld_rows != 0 && out->ld_rows != (int64_t)H.S) { set_err("fmcmc_out.ld_rows is honoured by fmcmc_mcmc_run_fun_dev only (host buffers are dense)"); return FMCMC_ERR_ARG; }
  H.open(device);
  stage_call(H, kn, run, st, out);
  if (H.rc == FMCMC_OK) H.rc = run_fun(&H.dk, kn->fixed, kn->lb, kn->ub, &H.dr, &H.ds, &H.dout, fun, user, H.stream, true);
  return fetch_call(H, kn, run, st, out);
}

int fmcmc_logpost_dev(const fmcmc_model* m, const double* theta, int64_t nchains, double* out, void* hip_stream) {
  if (!m || !theta || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  if (nchains < 1) { set_err("`nchains` must be an integer greater than 1."); return FMCMC_ERR_ARG; }
  int rc = check_eval_model(m);
  if (rc != FMCMC_OK) return rc;
  int dev = 0;
  (void)hipGetDevice(&dev);
  rc = require_gfx950(dev);
  if (rc != FMCMC_OK) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  ScratchList scratch(stream);
  EvalCall ev;
  rc = ev.prepare(m, scratch, stream);
  if (rc != FMCMC_OK) return rc;
  const hipError_t e = ev.enqueue(theta, nchains, out, stream);
  if (e != hipSuccess) { set_err("HIP launch failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
  return FMCMC_OK;
}

int fmcmc_validate_user(const fmcmc_run* run, int32_t k) {
  if (!run) { set_err("null argument"); return FMCMC_ERR_ARG; }
  fmcmc_kernel kn;
  memset(&kn, 0, sizeof(kn));
  kn.k = k;
  const int rr = validate_run(&kn, run);
  if (rr != FMCMC_OK) return rr;
  if (run->rng_mode == FMCMC_RNG_FED && !run->fed_logu) { set_err("rng_mode = FED needs fed_logu"); return FMCMC_ERR_ARG; }
  return FMCMC_OK;
}

int fmcmc_mcmc_run_user_dev(const fmcmc_model* m, fmcmc_logpost_fn fun, fmcmc_proposal_fn proposal, fmcmc_logratio_fn logratio,
                            void* user, int32_t k, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out, void* hip_stream) {
  if (!run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  if (!proposal) { set_err("null proposal callback"); return FMCMC_ERR_ARG; }
  if (!m && !fun) { set_err("null log-posterior callback"); return FMCMC_ERR_ARG; }
  if (!st->theta0 || !st->f0) { set_err("a user-defined kernel needs state->theta0 and f0"); return FMCMC_ERR_ARG; }
  int rc = fmcmc_validate_user(run, k);
  if (rc != FMCMC_OK) return rc;
  if (m) {
    rc = check_eval_model(m);
    if (rc != FMCMC_OK) return rc;
    const int kexp = eval_params(m->family, m->p, m->intercept);
    if (kexp != k) { set_err("Incorrect length of -initial-: the model has %d parameters, the kernel %d.", kexp, k); return FMCMC_ERR_ARG; }
  }
  return run_user(m, fun, proposal, logratio, user, k, run, st, out, (hipStream_t)hip_stream);
}

int fmcmc_validate_batch(const fmcmc_model* m, int64_t nmodels, const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (!m || !kn || !run) { set_err("null argument"); return FMCMC_ERR_ARG; }
  const int rr = validate_run(kn, run);
  if (rr != FMCMC_OK) return rr;
  if (kn->k > FMCMC_MAX_K_WAVE) {
    set_err("k = %d parameters: a batch of datasets runs up to FMCMC_MAX_K_WAVE = %d parameters per chain", kn->k, FMCMC_MAX_K_WAVE);
    return FMCMC_ERR_UNSUPPORTED;
  }
  if (kn->kind == FMCMC_KERNEL_NMIRROR || kn->kind == FMCMC_KERNEL_UMIRROR) {
    set_err("a batch of datasets runs with kernel_normal(_reflective), kernel_unif(_reflective), kernel_adapt(bw = 0, freq = 1) "
            "and kernel_ram; the mirror kernels are not supported on this path");
    return FMCMC_ERR_UNSUPPORTED;
  }
  if (kn->kind == FMCMC_KERNEL_ADAPT && (kn->bw > 0 || kn->freq > 1)) {
    set_err("a batch of datasets runs kernel_adapt with bw = 0 and freq = 1 only (got bw=%d, freq=%d): the windowed and the "
            "strided adaptation are not supported on this path", kn->bw, kn->freq);
    return FMCMC_ERR_UNSUPPORTED;
  }
  if (nmodels < 1) { set_err("`nmodels` must be at least 1 (got %lld).", (long long)nmodels); return FMCMC_ERR_ARG; }
  if (run->nchains % nmodels != 0) {
    set_err("`nchains` (%lld) must be a multiple of `nmodels` (%lld): every dataset gets the same number of chains.",
            (long long)run->nchains, (long long)nmodels);
    return FMCMC_ERR_ARG;
  }
  const int kexp = eval_params(m->family, m->p, m->intercept);
  if (kexp < 0) { set_err("unknown log-posterior family %d", m->family); return FMCMC_ERR_ARG; }
  if (kexp != kn->k) {
    set_err("Incorrect length of -initial-: the model has %d parameters, the kernel %d.", kexp, kn->k);
    return FMCMC_ERR_ARG;
  }
  if (m->n < 1) { set_err("the model needs at least one observation"); return FMCMC_ERR_ARG; }
  return validate_kernel(kn, run);
}

int fmcmc_mcmc_run_batch_dev(const fmcmc_model* m, int64_t nmodels, int64_t x_stride, int64_t y_stride, const fmcmc_kernel* kn,
                             const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out, uint32_t flags, void* hip_stream) {
  return fmcmc_mcmc_run_batch_sel_dev(m, nmodels, x_stride, y_stride, kn, run, st, out, nullptr, flags, hip_stream);
}

int fmcmc_mcmc_run_batch_sel_dev(const fmcmc_model* m, int64_t nmodels, int64_t x_stride, int64_t y_stride, const fmcmc_kernel* kn,
                                 const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out, const int32_t* active, uint32_t flags,
                                 void* hip_stream) {
  if (!m || !kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  int rc = check_batch_strides(m, x_stride, y_stride);
  if (rc != FMCMC_OK) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  KernelHostView v;
  rc = kernel_host_view(kn, stream, &v);
  if (rc != FMCMC_OK) return rc;
  rc = fmcmc_validate_batch(m, nmodels, &v.kh, run);
  if (rc != FMCMC_OK) return rc;
  return run_batch(m, nmodels, x_stride, y_stride, kn, v.fx, v.lb, v.ub, run, st, out, active, flags, stream);
}

int fmcmc_mcmc_run_batch_host(const fmcmc_model* m, int64_t nmodels, int64_t x_stride, int64_t y_stride, const fmcmc_kernel* kn,
                              const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out, uint32_t flags, int device) {
  if (!m || !kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  int rv = check_batch_strides(m, x_stride, y_stride);
  if (rv != FMCMC_OK) return rv;
  rv = fmcmc_validate_batch(m, nmodels, kn, run);
  if (rv != FMCMC_OK) return rv;
  if (!kn->fixed || !kn->lb || !kn->ub || !kn->mu || !kn->scale) { set_err("kernel arrays mu, scale, lb, ub and fixed are required"); return FMCMC_ERR_ARG; }
  if (fmcmc_device_count() < 1) { set_err("no HIP device: the engine has no CPU fallback"); return FMCMC_ERR_DEVICE; }
  HostStage H(kn, run, st, out);
  if (H.adaptive && (!st->Sigma || !st->abs_iter || !st->mean_prev || !st->have_mean)) {
    set_err("kernel_adapt / kernel_ram need state->Sigma, abs_iter, mean_prev and have_mean");
    return FMCMC_ERR_ARG;
  }
  if (out->ld_rows != 0 && out->ld_rows != (int64_t)H.S) { set_err("fmcmc_out.ld_rows is honoured by fmcmc_mcmc_run_batch_dev only (host buffers are dense)"); return FMCMC_ERR_ARG; }
  H.open(device);
  fmcmc_model dm = *m;
  const bool has_x = m->family != FMCMC_FAM_IID_NORMAL && m->p > 0;
  if (has_x) H.up(&dm.X, m->X, sizeof(double) * ((size_t)(nmodels - 1) * (size_t)x_stride + (size_t)m->p * m->n));
  H.up(&dm.y, m->y, sizeof(double) * ((size_t)(nmodels - 1) * (size_t)y_stride + (size_t)m->n));
  stage_call(H, kn, run, st, out);
  if (H.rc == FMCMC_OK) H.rc = run_batch(&dm, nmodels, x_stride, y_stride, &H.dk, kn->fixed, kn->lb, kn->ub, &H.dr, &H.ds, &H.dout, nullptr, flags, H.stream);
  return fetch_call(H, kn, run, st, out);
}

}  // extern "C"
