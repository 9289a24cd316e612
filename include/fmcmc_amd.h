/* fmcmc_amd.h — C-ABI of the MI355X-native many-chain Metropolis-Hastings engine.
 *
 * fmcmc (USCbiostats/fmcmc v0.6-0) is interpreted R and has NO FFI for its hot path:
 * the boundary is the R closure protocol of the per-chain loop,
 *     draws[i,] <- kernel$proposal(environment())   R/mcmc.R:752
 *     logpost[i] <- f(theta1)                        R/mcmc.R:754
 *     klogratio <- kernel$logratio(environment())    R/mcmc.R:768
 * which cannot cross to a GPU.  The drop-in therefore replaces the WHOLE loop body of
 * MCMC_without_conv_checker (R/mcmc.R:720-838) for all chains of a call at once; the
 * entry points below are what an R `.Call` shim binds (INTEGRATION.md shows the stub).
 * Every struct is plain-old-data: plain pointers, sizes and scalars, no torch types.
 *
 * Two pointer domains, same structs:
 *   *_host entry points: every pointer is HOST memory; the library stages to/from HBM.
 *   *_dev  entry points: every pointer is DEVICE memory (hipMalloc / a torch tensor's
 *                        data_ptr); the call only enqueues work on `stream` when the kernel's
 *                        host mirrors (fmcmc_kernel.h_*) are set, else it reads a few bytes back first.
 *
 * Layouts (chosen so that one chain's block is exactly an R column-major matrix):
 *   X        [p][n]       column-major n x p design matrix (no intercept column)
 *   initial/theta0 [C][k] one row per chain (R: initial[c, ])
 *   samples  [C][k][S]    ans of chain c = column-major S x k matrix (R/mcmc.R:728,778)
 *   draws    [C][k][S]    proposals (R/mcmc.R:731,752)
 *   logpost  [C][S]       f(theta1) per kept row (R/mcmc.R:730,754)
 *   Sigma    [C][kf][kf]  row-major per chain; kernel_adapt: covariance (R/kernel_adapt.R:148),
 *                         kernel_ram: lower-triangular factor (R/kernel_ram.R:141)
 *   S = floor((nsteps - burnin) / thin) kept rows: 1-based rows r = burnin + j*thin
 *   (R/mcmc.R:786-813).
 */
#ifndef FMCMC_AMD_H
#define FMCMC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMCMC_ABI_VERSION 6
#define FMCMC_MAX_K 256 /* parameters per chain supported by the device kernels (R/kernel_ram.R:93-121, R/kernel_adapt.R:87-115: any k) */
/* Up to FMCMC_MAX_K_WAVE parameters a chain's rows live in the lanes of one wavefront and every kernel, scheme and option is
 * available; from there to FMCMC_MAX_K one workgroup serves a chain (mh_sweep_bigk): kernel_normal(_reflective) /
 * kernel_unif(_reflective) with scheme = "joint", kernel_adapt(bw = 0, freq = 1), kernel_ram -- anything else is refused above FMCMC_MAX_K_WAVE with FMCMC_ERR_UNSUPPORTED;
 * its matrices live in LDS while they fit and in the chain's own Sigma buffer beyond (kernel_adapt from 134, kernel_ram from 184
 * free parameters).  Raised from 128 to 256 under the same FMCMC_ABI_VERSION: no struct, signature or buffer layout changed
 * (INTEGRATION.md); 256 and not more because the host oracle's stack frame grows as k^2;
 * fmcmc_gelman_partial_dev and fmcmc_gelman_finish take any p <= FMCMC_MAX_K columns (the window reduction tiles its output
 * above FMCMC_MAX_K_WAVE: one workgroup per chain and pair of 64-column blocks; widened from FMCMC_MAX_K_WAVE under the same
 * FMCMC_ABI_VERSION, no layout changed). */
#define FMCMC_MAX_K_WAVE 64

/* ---- log-posterior families: the `fun` argument of MCMC() (R/mcmc.R:327) ---------- */
enum {
  /* sum(dnorm(y - (b0 + X b), sd = sigma, log = TRUE)); theta = (b0?, b[p], sigma).
   * README.md:128-139 (guard=1: non-finite -> -Inf) and :356-361 (guard=0). */
  FMCMC_FAM_GAUSSIAN_LINREG = 1,
  /* sum(logp[y==1]) + sum(logq[y==0]) - sum(beta^2)/prior_div; theta = (b0?, b[p]).
   * vignettes/workflow-with-fmcmc.Rmd:35-41. */
  FMCMC_FAM_LOGISTIC = 2,
  /* sum(log(dnorm(D, mu, sigma))); theta = (mu, sigma); D passed as y, p = 0.
   * R/mcmc.R:141-144. */
  FMCMC_FAM_IID_NORMAL = 3
};

typedef struct fmcmc_model {
  int32_t family;     /* FMCMC_FAM_* */
  int32_t p;          /* covariate columns in X (0 allowed) */
  int64_t n;          /* observations */
  const double* X;    /* [p][n] column-major, may be NULL when p == 0 */
  const double* y;    /* [n] response / 0-1 outcome / data vector */
  int32_t intercept;  /* 1: theta[0] is an intercept (implicit column of ones) */
  int32_t guard;      /* 1: non-finite log-posterior is returned as -Inf (README.md:133-136) */
  double prior_div;   /* logistic: prior -sum(beta^2)/prior_div; 0 = flat */
} fmcmc_model;

/* ---- transition kernels: the `kernel` argument (R/kernel_*.R) --------------------- */
enum {
  FMCMC_KERNEL_NORMAL = 1,            /* R/kernel_normal.R:26-82   */
  FMCMC_KERNEL_NORMAL_REFLECTIVE = 2, /* R/kernel_normal.R:96-177  */
  FMCMC_KERNEL_ADAPT = 3,             /* R/kernel_adapt.R:54-202   */
  FMCMC_KERNEL_RAM = 4,               /* R/kernel_ram.R:65-181     */
  /* theta1[w] = theta0[w] + runif(min.[w], max.[w]) (R/kernel_unif.R:42-91, :96-170): the same proposal code as
   * the normal kernels with mu := min., scale := max. - min. and U(0,1) variates instead of N(0,1). */
  FMCMC_KERNEL_UNIF = 5,
  FMCMC_KERNEL_UNIF_REFLECTIVE = 6,
  /* mirror kernels (R/kernel_mirror.R:3-138, :140-283): theta1[w] ~ N(2 mu[w] - theta0[w], scale[w]^2) resp.
   * U(2 mu - theta0[w] -+ sqrt(3) scale); mu follows the running mean of the chain during warm-up and scale is rescaled
   * once, when abs_iter == nadapt, by tan(pi/2 obs_arate) / tan(pi/2 arate).  (The closure reads its ARGUMENT nadapt,
   * not the floor(seq(...)) vector stored next to it, so there is exactly one adaptation; the element-wise indexing of
   * kernel_umirror -- mu[a], scale[a] of the a-th updated parameter -- is kept as it is in the reference.) */
  FMCMC_KERNEL_NMIRROR = 7,
  FMCMC_KERNEL_UMIRROR = 8
};
/* Update schemes of the normal / uniform kernels, plan_update_sequence (R/kernel.R:66-133).  Row i of the plan is used
 * by loop step i (R/kernel_normal.R:67); the plan is built once per kernel object for the nsteps of its first call. */
enum {
  FMCMC_SCHEME_JOINT = 0,    /* all free parameters every step (:94-99) */
  FMCMC_SCHEME_ORDERED = 1,  /* one parameter per step, which(!fixed)[(i-1) mod kf] (:101-104) */
  FMCMC_SCHEME_RANDOM = 2,   /* one parameter per step, sample(which(!fixed), nsteps, TRUE)[i] (:106-113) */
  FMCMC_SCHEME_EXPLICIT = 3  /* one parameter per step, scheme_seq[(i-1) mod scheme_len] (:69-92) */
};

enum {
  FMCMC_RAM_QFUN_T_K = 0,    /* stats::rt(k, k), the default (R/kernel_ram.R:68) */
  FMCMC_RAM_QFUN_NORMAL = 1, /* stats::rnorm(k): the Gaussian proposal of Vihola (2012) */
  FMCMC_RAM_QFUN_T_DF = 2    /* stats::rt(k, ram_df) */
};

typedef struct fmcmc_kernel {
  int32_t kind;         /* FMCMC_KERNEL_* */
  int32_t k;            /* number of parameters (length of theta) */
  const double* mu;     /* [k] proposal mean (already recycled: R/kernel.R:3-17); unif kernels: min. */
  const double* scale;  /* [k] proposal sd (normal kernels); unif kernels: max. - min. */
  const double* lb;     /* [k] lower bounds, -DBL_MAX when unbounded (R/kernel.R:25-41) */
  const double* ub;     /* [k] upper bounds */
  const uint8_t* fixed; /* [k] 1 = parameter never updated */
  int32_t scheme;       /* FMCMC_SCHEME_* (normal / unif kernels) */
  int32_t freq;         /* adapt/ram: adaptation frequency (adapt every freq-th loop step, `!(env$i %% freq)`) */
  int32_t warmup;       /* adapt/ram */
  int32_t bw;           /* adapt: > 0 = windowed AM, Sigma = Sd * (cov(last bw - 1 rows) + eps * I) (R/kernel_adapt.R:123-125) */
  double until;         /* adapt/ram: stop adapting when abs_iter >= until (Inf allowed) */
  double eps;           /* adapt/ram: initial Sigma = eps * I */
  double arate;         /* ram: target acceptance rate */
  double Sd;            /* adapt: scaling of the windowed variant (the recursive path does not apply it, as in R) */
  const int32_t* scheme_seq; /* [scheme_len] FMCMC_SCHEME_EXPLICIT: 0-based parameter indices, a permutation of the
                              * free parameters (R/kernel.R:72-90); NULL otherwise */
  int32_t scheme_len;
  int32_t nadapt;       /* mirror kernels: abs_iter at which the scale is adapted (R/kernel_mirror.R:103,121) */
  const double* constr; /* ram: [kf][kf] mask multiplied element-wise into the updated factor
                         * (constr[which., which.], R/kernel_ram.R:149-150); NULL = none */
  /* v3, fmcmc_mcmc_run_dev only: HOST copies of the device arrays above that the launch geometry and the argument checks
   * need (fixed, lb, ub; scale for the uniform kernels; scheme_seq).  With all of them set the entry point only enqueues
   * work; with NULLs it reads the few bytes back from the device and synchronises the stream first. */
  const uint8_t* h_fixed;
  const double* h_lb;
  const double* h_ub;
  const double* h_scale;
  const int32_t* h_scheme_seq;
  /* ram: built-in alternatives to the defaults of R/kernel_ram.R:67-68 (user closures cannot cross a C boundary; these
   * are the families the arguments are used for).  All zero = the defaults. */
  int32_t ram_qfun;     /* FMCMC_RAM_QFUN_*: the variates U = qfun(k) of R/kernel_ram.R:124 */
  int32_t reserved;
  double ram_df;        /* FMCMC_RAM_QFUN_T_DF: degrees of freedom (> 0) */
  double ram_eta_exp;   /* eta(i, k) = min(1, k * i^(-ram_eta_exp)); 0 = the default 2/3 (R/kernel_ram.R:67) */
} fmcmc_kernel;

/* ---- one call of MCMC_without_conv_checker over all chains ------------------------ */
enum { FMCMC_RNG_PHILOX = 0, FMCMC_RNG_FED = 1 };

typedef struct fmcmc_run {
  int64_t nchains;      /* chains in THIS call (the shard) */
  int64_t nsteps;       /* R's nsteps: rows of ans before burn-in/thinning; loop runs i = 2..nsteps */
  int64_t burnin;
  int64_t thin;
  uint64_t seed;        /* Philox key */
  int64_t chain_base;   /* global id of local chain 0 (sharding never changes results) */
  int64_t step_base;    /* MH iterations already done by these chains in earlier calls/bulks */
  int32_t rng_mode;     /* FMCMC_RNG_* */
  int32_t reserved;
  /* FMCMC_RNG_FED: host-generated variates in R's own draw order (bit-exact fmcmc replay):
   * fed_logu [C][nsteps] (entry i-1 is R[i]); fed_z [C][nsteps][kz] proposal variates of step i
   * (kz = free parameters; normal/adapt: N(0,1); ram: Student-t).  NULL in PHILOX mode. */
  const double* fed_logu;
  const double* fed_z;
} fmcmc_run;

/* Per-chain state carried from call to call: chain restart by value (R/mcmc.R:344-422) plus
 * the kernel environments that persist across bulks (R/kernel.R:218-237). In/out. */
typedef struct fmcmc_state {
  double* theta0;      /* [C][k]  in: initial; out: last row of ans */
  double* f0;          /* [C]     out: log-posterior of theta0 */
  int64_t* abs_iter;   /* [C]     adapt/ram: kernel's abs_iter (0 for a fresh kernel) */
  double* Sigma;       /* [C][kf][kf] adapt/ram (kf = number of non-fixed parameters); NULL otherwise */
  double* mean_prev;   /* [C][kf] adapt: Mean_t_prev */
  int32_t* have_mean;  /* [C]     adapt: 0 while Mean_t_prev is NULL (R/kernel_adapt.R:130) */
  int32_t* nerrors;    /* [C]     ram: failed factor updates (R/kernel_ram.R:143) */
  int32_t fresh;       /* 1: kernel state is uninitialised; the engine sets Sigma = eps*I etc. */
  int32_t reserved;
  /* FMCMC_SCHEME_RANDOM: the plan of the kernel object, entry [c][i-1] = 0-based parameter updated by loop step i.
   * PHILOX mode: a pure function of (seed, global chain, i) -- identical in every call, as the reference reuses
   * the plan of the kernel's first call -- written here when non-NULL.  FED mode: read from here (the caller
   * replays R's sample()).  [C][nsteps] int32, or NULL. */
  int32_t* scheme_cols;
  /* mirror kernels: the adapted mean and scale of every chain, [C][k] each, and obs_arate, [C][k] (ABI 6; was [C]): NaN before
   * the one-off adaptation, the observed acceptance rate it used in all k entries after it, then -- through the rest of the
   * warm-up -- R's element-wise running mean of (ans[i-1, ] != ans[i-2, ]) (R/kernel_mirror.R:108-118,:246-253: the closure's
   * scalar turns into a k-vector there).  fresh == 1: mu / scale initialised from kernel->mu / kernel->scale. */
  double* mirror_mu;
  double* mirror_scale;
  double* obs_arate;
} fmcmc_state;

enum {
  FMCMC_CHAIN_OK = 0,
  FMCMC_CHAIN_NAN_LOGPOST = 1, /* fun(par) is undefined: R/mcmc.R:758-765 */
  FMCMC_CHAIN_NAN_RATIO = 2,   /* f1 - f0 is NaN (e.g. -Inf - -Inf): R's `if (NA)` error */
  FMCMC_CHAIN_NOT_PD = 3,      /* proposal covariance not positive definite (MASS::mvrnorm error) */
  /* kernel_adapt with bw > 0 or freq > 1: the rows ans[(i-bw+1):(i-1), ] / ans[(i-freq):(i-1), ] reach before the first row
   * of this call (R: "subscript out of bounds" / mixed subscripts, R/kernel_adapt.R:119-125,139-156) */
  FMCMC_CHAIN_BAD_WINDOW = 4,
  FMCMC_CHAIN_SYNC_TIMEOUT = 5 /* engine-internal: a grid-wide hand-over of the observation-sharded evaluation timed out */
};

typedef struct fmcmc_out {
  double* samples;        /* [C][k][S] */
  double* logpost;        /* [C][S] or NULL */
  double* draws;          /* [C][k][S] or NULL */
  int64_t* accept_count;  /* [C] accepted proposals in this call */
  uint32_t* accept_bits;  /* [C][ceil(nsteps/32)] bit (i-1) set iff loop step i accepted; or NULL */
  int32_t* status;        /* [C] FMCMC_CHAIN_* */
  int64_t* status_step;   /* [C] loop index i at which status was raised */
  double* status_theta;   /* [C][k] theta1 at that step */
  int64_t ld_rows;        /* v3, fmcmc_mcmc_run_dev only: row stride of samples / draws columns and of logpost rows; 0 = S.
                           * With ld_rows > S the kept rows of consecutive calls (the bulks of MCMC_with_conv_checker,
                           * R/mcmc.R:926-947) land in ONE preallocated [C][k][ld_rows] history: pass samples + rows so far. */
} fmcmc_out;

/* Return codes */
enum {
  FMCMC_OK = 0,
  FMCMC_ERR_ARG = 1,     /* invalid argument; message mirrors the reference's stop() text */
  FMCMC_ERR_DEVICE = 2,  /* HIP runtime failure / no device */
  FMCMC_ERR_CHAIN = 3,   /* at least one chain raised a FMCMC_CHAIN_* status */
  FMCMC_ERR_UNSUPPORTED = 4,
  FMCMC_ERR_FUN = 5      /* the caller's log-posterior callback (fmcmc_logpost_fn) returned non-zero; the call was abandoned */
};

int fmcmc_abi_version(void);
const char* fmcmc_last_error(void);
/* Diagnostic: which kernel variant the calling thread's last fmcmc_mcmc_run_* chose ("mfma", "spec", "resident",
 * "streamed", "streamed-logistic", "streamed-wide", "streamed-wide-sharded", ...).  Results never depend on it. */
const char* fmcmc_last_kernel(void);
int fmcmc_device_count(void);
int64_t fmcmc_kept_rows(int64_t nsteps, int64_t burnin, int64_t thin);

/* Validates a call exactly like R/mcmc.R:501-520 and the kernel initialisers
 * (R/kernel_normal.R:134-135, R/kernel.R:9,129-132); no GPU needed. */
int fmcmc_validate(const fmcmc_model* model, const fmcmc_kernel* kernel, const fmcmc_run* run);

/* Diagnostic: the route the library plans for a call -- which kernel form would run it and in which shape -- without a device
 * call or an allocation, so it works on a machine without a GPU.  `kernel` holds HOST pointers (lb, ub and fixed are required;
 * the data pointers of `model` and the fed streams of `run` are never read, only tested for null by fmcmc_validate).  ld_rows:
 * fmcmc_out.ld_rows of the call (0: its kept rows); ncu: the compute units of the device to plan for (MI355X: 256).  Reads
 * FMCMC_AMD_DEBUG as a run does.  Writes one line of space-separated key=value fields into `text`: `form` and `base` as
 * fmcmc_last_kernel() names them, every number and flag of the plan, and its five kernel handles as 0 (none) or 1.  A run may
 * still step down from `form` to `base` (a refused cooperative launch), and a fed logistic call may take "logistic-shadow".
 * Returns fmcmc_validate's code and message for a call it refuses; FMCMC_ERR_ARG when `text` is too short (1024 bytes do). */
int fmcmc_plan_route(const fmcmc_model* model, const fmcmc_kernel* kernel, const fmcmc_run* run, int64_t ld_rows, int32_t ncu,
                     char* text, size_t text_len);

/* The hot path. Replaces R/mcmc.R:720-838 x R/kernel_*.R for all chains of the call. */
int fmcmc_mcmc_run_dev(const fmcmc_model* model, const fmcmc_kernel* kernel,
                       const fmcmc_run* run, fmcmc_state* state, fmcmc_out* out,
                       void* hip_stream);
int fmcmc_mcmc_run_host(const fmcmc_model* model, const fmcmc_kernel* kernel,
                        const fmcmc_run* run, fmcmc_state* state, fmcmc_out* out,
                        int device);

/* ---- user-defined log-posteriors: the `fun` of MCMC() as a batched callback (R/mcmc.R:754) ---------------------------------
 * Batched log-posterior: out[c] = log f(theta[c][0..k-1]) for c < nchains.  Called on the calling host thread.  Work is
 * enqueued on hip_stream, or the function synchronises before returning.  0 = ok; anything else aborts the call. */
typedef int (*fmcmc_logpost_fn)(const double* theta, int64_t nchains, int32_t k, double* out, void* hip_stream, void* user);

/* The semantics of fmcmc_mcmc_run_* with the family replaced by `fun`: the same run / state / out layouts (ld_rows, FED mode,
 * chain_base, step_base, carried kernel state), chain statuses and outputs.  `fun` is called once for row 1 (f0), then once per
 * loop step; bounded kernel_ram calls it twice per step, on the un-reflected proposal and on the reflected one
 * (R/kernel_ram.R:129-152).  A non-zero return of `fun` ends the call with FMCMC_ERR_FUN (fmcmc_last_error() names the step and
 * the code); the chain state of such a call is undefined.  Kernels: kernel_normal(_reflective) / kernel_unif(_reflective) with
 * every scheme, kernel_adapt(bw = 0, freq = 1), kernel_ram with every option, 1 <= k <= FMCMC_MAX_K; the mirror kernels and the
 * windowed / strided kernel_adapt are refused with FMCMC_ERR_UNSUPPORTED.  fmcmc_last_kernel(): "fun" (k <= FMCMC_MAX_K_WAVE,
 * one wavefront per chain) or "fun-wg" (one workgroup per chain).  Pointers inside `kernel` follow the domain of the entry
 * point, as for fmcmc_mcmc_run_dev / _host. */
int fmcmc_validate_fun(const fmcmc_kernel* kernel, const fmcmc_run* run);
int fmcmc_mcmc_run_fun_dev(const fmcmc_kernel* kernel, const fmcmc_run* run, fmcmc_state* state, fmcmc_out* out,
                           fmcmc_logpost_fn fun, void* user, void* hip_stream);   /* theta/out of `fun`: device pointers */
int fmcmc_mcmc_run_fun_host(const fmcmc_kernel* kernel, const fmcmc_run* run, fmcmc_state* state, fmcmc_out* out,
                            fmcmc_logpost_fn fun, void* user, int device);      /* theta/out of `fun`: host pointers */

/* ---- the families' log-posterior at caller-given points -------------------------------------------------------------------
 * out[c] = f(theta[c][0..k-1]) for c < nchains, k the family's parameter count: the canonical form the sweeps evaluate (the 512
 * canonical lanes, their xor tree, the closed form), bit for bit.  One workgroup per parameter vector; theta and out are device
 * pointers, the work is enqueued on hip_stream.  Any n >= 1 and any k <= FMCMC_MAX_K. */
int fmcmc_logpost_dev(const fmcmc_model* model, const double* theta /* [C][k], device */, int64_t nchains,
                      double* out /* [C], device */, void* hip_stream);

/* ---- user-defined transition kernels: kernel_new(proposal, logratio) as batched callbacks (R/kernel.R:136-317) --------------
 * What R/kernel.R:169-184 lists, for all chains of the call; device pointers, read-only.  `proposal` sees in theta1 / f1 the LAST
 * proposal and its value, `logratio` the new ones.  env$ans is not offered (kept rows are not R's rows). */
typedef struct {
  int64_t i;               /* R's 1-based loop index, 2 .. nsteps */
  int64_t nsteps, nchains, chain_base, step_base;
  int32_t k;
  const double* theta0;    /* [C][k] */
  const double* theta1;    /* [C][k] */
  const double* f0;        /* [C] */
  const double* f1;        /* [C] */
  const int32_t* status;   /* [C] FMCMC_CHAIN_*: a chain whose status is not OK no longer moves */
} fmcmc_step_env;
/* Called on the calling host thread, once per loop step each.  Work is enqueued on hip_stream, or the function synchronises
 * before returning.  0 = ok; anything else aborts the call. */
typedef int (*fmcmc_proposal_fn)(const fmcmc_step_env* env, double* theta1_out /* [C][k] */, void* hip_stream, void* user);
typedef int (*fmcmc_logratio_fn)(const fmcmc_step_env* env, double* logratio_out /* [C] */, void* hip_stream, void* user);

/* The loop of fmcmc_mcmc_run_fun_dev with the proposal outside (R/mcmc.R:737-783).  Row 1: f0 = f(initial), theta1 = theta0,
 * f1 = f0.  Then for i = 2 .. nsteps: proposal(env) writes theta1; f1 = f(theta1), through `fun` or, when `model` is given,
 * through the evaluator of fmcmc_logpost_dev; logratio(env) when given (NULL: f1 - f0, the decision of the built-in kernels);
 * one launch of the accept / store step: NaN f1 -> FMCMC_CHAIN_NAN_LOGPOST, NaN ratio -> FMCMC_CHAIN_NAN_RATIO, accept iff
 * log u < ratio with the engine's accept uniform of (seed, step_base + i, chain_base + c) (FED mode: run->fed_logu; fed_z is
 * not read).  The same run / out layouts, statuses and outputs as fmcmc_mcmc_run_fun_dev; of `state` theta0 and f0 only.
 * Everything is enqueued on hip_stream, no host synchronisation.  A non-zero return of a callback ends the call with
 * FMCMC_ERR_FUN (fmcmc_last_error() names the callback, the step and the code).  1 <= k <= FMCMC_MAX_K; fmcmc_last_kernel():
 * "user" (k <= FMCMC_MAX_K_WAVE) or "user-wg".  fmcmc_validate_user: the run checks of fmcmc_validate with their messages. */
int fmcmc_validate_user(const fmcmc_run* run, int32_t k);
int fmcmc_mcmc_run_user_dev(const fmcmc_model* model /* or NULL */, fmcmc_logpost_fn fun /* used when model is NULL */,
                            fmcmc_proposal_fn proposal, fmcmc_logratio_fn logratio /* NULL: f1 - f0 */, void* user,
                            int32_t k, const fmcmc_run* run, fmcmc_state* state, fmcmc_out* out, void* hip_stream);

/* ---- one model fitted to many datasets in one call (a simulation study, a bootstrap, one regression per subject) ------------
 * `model` gives the family and the shape every dataset shares (p, n, intercept, guard, prior_div) and the X / y of dataset 0;
 * dataset d lies x_stride / y_stride doubles behind it (x_stride >= p n, y_stride >= n; X is [p][n] per dataset).  run->nchains
 * is the total, nmodels x chains_per_model: local chain c samples dataset c / chains_per_model with the stream of global chain
 * run->chain_base + c, so a caller may shard by whole datasets (X / y of its first one, chain_base advanced).  Everything else
 * -- kernel, run, state, out with their layouts, ld_rows, FED mode, step_base, the carried kernel state, chain statuses -- is
 * fmcmc_mcmc_run_dev's, and every output is bit for bit what that entry gives dataset d's chains on their own.
 * One launch runs every step of every chain (one workgroup per chain; fmcmc_last_kernel(): "batch-lds" -- each workgroup holds
 * its dataset in LDS -- or "batch-stream" -- it reads it from global memory every step; the library picks by size,
 * FMCMC_BATCH_STREAM_DATA in `flags` forces the second).  Kernels: those of fmcmc_validate_fun (kernel_normal(_reflective) /
 * kernel_unif(_reflective) with every scheme, kernel_adapt(bw = 0, freq = 1), kernel_ram with every option) up to
 * FMCMC_MAX_K_WAVE parameters; refused with FMCMC_ERR_UNSUPPORTED / FMCMC_ERR_ARG: k > FMCMC_MAX_K_WAVE, the mirror kernels,
 * the windowed / strided kernel_adapt, nmodels < 1, nchains not a multiple of nmodels, strides smaller than a dataset.
 * fmcmc_validate_batch needs no device and applies fmcmc_validate's model and run checks with their messages (strides are
 * checked by the run entries, before any device call). */
enum { FMCMC_BATCH_STREAM_DATA = 1 };
int fmcmc_validate_batch(const fmcmc_model* model, int64_t nmodels, const fmcmc_kernel* kernel, const fmcmc_run* run);
int fmcmc_mcmc_run_batch_dev(const fmcmc_model* model /* shape; X, y: dataset 0 */, int64_t nmodels,
                             int64_t x_stride, int64_t y_stride /* doubles between datasets */,
                             const fmcmc_kernel* kernel, const fmcmc_run* run, fmcmc_state* state, fmcmc_out* out,
                             uint32_t flags, void* hip_stream);
/* fmcmc_mcmc_run_batch_dev with a dataset mask: active[nmodels] (device int32, NULL = every dataset).  The chains of a dataset
 * whose entry is 0 do not run: their theta0, f0, Sigma, abs_iter, mean_prev, have_mean, nerrors, their output rows, status,
 * status_step, status_theta, accept count and bitmap are left exactly as they were; every other chain's outputs are bit for
 * bit those of fmcmc_mcmc_run_batch_dev (which is this entry with NULL).  fmcmc_run.step_base is one number: chains that sat
 * out a call are behind the others in their variate streams, so a later call runs them with the others only when the caller
 * accepts that (MCMC_batch(stop_each = ...) never runs them again).  No host-pointer variant: a stop loop over host pointers
 * would stage the data again for every call. */
int fmcmc_mcmc_run_batch_sel_dev(const fmcmc_model* model, int64_t nmodels, int64_t x_stride, int64_t y_stride,
                                 const fmcmc_kernel* kernel, const fmcmc_run* run, fmcmc_state* state, fmcmc_out* out,
                                 const int32_t* active, uint32_t flags, void* hip_stream);
int fmcmc_mcmc_run_batch_host(const fmcmc_model* model, int64_t nmodels, int64_t x_stride, int64_t y_stride,
                              const fmcmc_kernel* kernel, const fmcmc_run* run, fmcmc_state* state, fmcmc_out* out,
                              uint32_t flags, int device);   /* every pointer a host pointer */

/* Gelman-Rubin partial sums over local chains (R/convergence.R:191-246 -> coda::gelman.diag).
 * Window = kept rows [row0, row0+N) of each chain. partial has fmcmc_gelman_partial_len(p)
 * doubles: {m, sum xbar[p], sum xbar xbar^T[p*p], sum S_c[p*p], sum s2[p], sum s2^2[p],
 * sum s2*xbar[p], sum s2*xbar^2[p]}.  Partials of different GPUs add (one all-reduce). */
int64_t fmcmc_gelman_partial_len(int32_t p);
/* doubles of scratch (device) the partial kernel needs: per chain xbar[p] and S_c[p][p] */
int64_t fmcmc_gelman_work_len(int64_t nchains, int32_t p);
/* cols[p]: parameter indices to test (the free parameters, R/mcmc.R:950-968), device int32; 1 <= p <= FMCMC_MAX_K.
 * work: fmcmc_gelman_work_len doubles, left as work[c] = {xbar[p] - center, S_c[p][p] (both triangles)} per chain.
 * center[p] (device, may be NULL): xbar sums are accumulated relative to it (all ranks must
 * pass the same vector); it only limits cancellation, R-hat is shift-invariant. */
int fmcmc_gelman_partial_dev(const double* samples, int64_t nchains, int32_t k, int64_t S,
                             int64_t row0, int64_t N, const int32_t* cols, int32_t p,
                             const double* center, double* work, double* partial,
                             void* hip_stream);
/* The same reduction for ngroups groups of chains_per_group consecutive chains (group g = chains g chains_per_group ..; one
 * model on many datasets: a group = the chains of a dataset) in two launches on the caller's stream.  partials is
 * [ngroups][fmcmc_gelman_partial_len(p) + 2] (device): the head of row g is bit for bit the partial that
 * fmcmc_gelman_partial_dev gives for the chains of group g alone with center = the window's first row (row0) of the group's
 * first chain at the columns cols; the two doubles behind it are the sum and the sum of squares of every entry of the group's
 * window, formed from the chains' means and variances in a fixed order (rm_invariant's test, R/convergence.R:171-173).
 * active[ngroups] (device int32, NULL = all): the row of a group whose entry is 0 is not written.  work:
 * fmcmc_gelman_groups_work_len doubles, left as work[c] = {xbar[p] (NOT centred), S_c[p][p]} per chain.
 * 1 <= p <= FMCMC_MAX_K_WAVE (FMCMC_ERR_UNSUPPORTED beyond); the finish is fmcmc_gelman_finish per row, on the host. */
int64_t fmcmc_gelman_groups_work_len(int64_t ngroups, int64_t chains_per_group, int32_t p);
int fmcmc_gelman_groups_dev(const double* samples, int64_t ngroups, int64_t chains_per_group, int32_t k, int64_t S,
                            int64_t row0, int64_t N, const int32_t* cols, int32_t p, const int32_t* active,
                            double* work, double* partials, void* hip_stream);
/* Host finish on the (all-reduced) partial: psrf[p] point estimates, *mpsrf (NaN if p == 1).
 * Returns FMCMC_ERR_CHAIN when W is not positive definite (gelman.diag would fail); psrf[p] is complete then too. */
int fmcmc_gelman_finish(const double* partial, int32_t p, int64_t N, double* psrf,
                        double* mpsrf);

/* ---- posterior summary of the kept rows, computed on the device (coda::summary.mcmc(.list), coda::effectiveSize) -----------
 * Window = kept rows [row0, row0 + N) of each of the `nchains` local chains, columns cols[p] (device int32, each < k); S is the
 * row stride of `samples` (fmcmc_out.ld_rows), as for fmcmc_gelman_partial_dev.  Per chain c and column j:
 *   mean, variance (divisor N - 1), spec0 = coda::spectrum0.ar (autocovariances with divisor N of the series centred on its
 *   mean up to lag M = min(N - 1, floor(10 log10 N)), Levinson-Durbin, aic_m = N log(v_m) + 2 m + 2 at its first minimum o,
 *   var.pred = v_o N / (N - (o + 1)), spec0 = var.pred / (1 - sum ar)^2; 0 for a constant or exactly linear series), order o.
 * chain_stats (device, may be NULL): [nchains][p][4] = {mean, variance, spec0, order}.
 * pooled (device, fmcmc_summary_pooled_len(p, nprobs) doubles): [p][5] = {mean and variance (divisor nchains N - 1) of the
 *   pooled rows, mean over the chains of spec0, effective size = sum_c (spec0 == 0 ? 0 : N var_c / spec0), count of non-finite
 *   values}, then [p][nprobs][2] = the order statistics x_(lo), x_(hi) of the nchains N pooled values of the column, with
 *   index = 1 + (nchains N - 1) probs[q], lo = floor(index), hi = ceil(index) (R's quantile type 7 interpolates between them:
 *   q = x_(lo) + (index - lo) (x_(hi) - x_(lo))).  They are exact (a radix select on the values' bits, no sort, no sketch).
 * probs: HOST array of nprobs <= 16 probabilities in [0, 1], read during the call; nprobs = 0 skips the order statistics.
 * work: device scratch of fmcmc_summary_work_len(nchains, p, nprobs) doubles.  The call only enqueues kernels on hip_stream and
 * reads `samples` only.  N >= 3; N < 3162278 (AR orders up to 64), FMCMC_ERR_UNSUPPORTED beyond.  Argument errors are found
 * before any device call (no GPU needed) and leave their text in fmcmc_last_error().  Every sum has a fixed order: the
 * results are the same bits on every call.  With non-finite values in the window the moments are NaN and the count says so. */
int64_t fmcmc_summary_work_len(int64_t nchains, int32_t p, int32_t nprobs);
int64_t fmcmc_summary_pooled_len(int32_t p, int32_t nprobs);
int fmcmc_summary_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                      const int32_t* cols, int32_t p, const double* probs, int32_t nprobs, double* work,
                      double* chain_stats, double* pooled, void* hip_stream);
/* The same summary for ngroups groups of chains_per_group consecutive chains, each group on its own (group g = chains
 * g chains_per_group ..; one model on many datasets: a group = the chains of a dataset), enqueued once on the caller's stream.
 * pooled is [ngroups][fmcmc_summary_pooled_len(p, nprobs)] (device): row g is bit for bit the `pooled` that fmcmc_summary_dev
 * writes for the chains of group g alone (divisors and ranks over chains_per_group N values).  chain_stats (device, may be NULL):
 * [ngroups chains_per_group][p][4], and work, fmcmc_summary_groups_work_len = ngroups chains_per_group p (72 + 4) doubles whose
 * head is [series][72] (r_0 .. r_64, mean at 65, residual sd at 66, non-finite count at 67): both bit for bit those of the single
 * call.  active[ngroups] (device int32, NULL = all): for a group whose entry is 0 no row of pooled, chain_stats or work is
 * written.  probs as for fmcmc_summary_dev.  The order statistics of a (group, column) are selected by ONE workgroup that keeps
 * the group's chains_per_group N keys in LDS while they are at most 19456 and re-reads them every pass beyond: correct at any
 * size below 2^32 values per group (FMCMC_ERR_UNSUPPORTED from there), slow for a few large groups -- fmcmc_summary_dev per
 * group is the form for those. */
int64_t fmcmc_summary_groups_work_len(int64_t ngroups, int64_t chains_per_group, int32_t p, int32_t nprobs);
int fmcmc_summary_groups_dev(const double* samples, int64_t ngroups, int64_t chains_per_group, int32_t k, int64_t S,
                             int64_t row0, int64_t N, const int32_t* cols, int32_t p, const int32_t* active,
                             const double* probs, int32_t nprobs, double* work, double* chain_stats, double* pooled,
                             void* hip_stream);

/* ---- Heidelberger-Welch diagnostic of every chain (coda::heidel.diag), the device part ---------------------------------------
 * Window, samples, S, cols as for fmcmc_summary_dev.  Rows are counted from row0: half_row is the first row of the window the
 * spectral density S0 of the stationarity test comes from (coda: window(Y, start = end / 2)); cand_rows is a HOST array, read
 * during the call, of ncand >= 1 ascending first rows of the candidate tails [cand_rows[s], N) (ncand is not capped);
 * half_row >= cand_rows[0], so that the longest tail contains every row the call reads.
 * out (device, fmcmc_heidel_out_len doubles): [1 + ncand][nchains][p][4] = {mean, variance, spec0, order} as fmcmc_summary_dev
 *   defines them, entry 0 for [half_row, N), entry 1 + s for the tail of candidate s; then [ncand][nchains][p] = Q, the sum
 *   over the rows t of the tail of B_t^2, B_t = sum_{u <= t} (y_u - mean): the tail is centred on the mean reported for it
 *   before it is scanned.  The Cramer-von Mises statistic is Q / (n^2 S0), n = N - cand_rows[s].
 * work: device scratch of fmcmc_heidel_work_len doubles; on return its first nchains p 72 doubles are the series work of the
 *   tail of cand_rows[0] (per series 72 doubles, the 68th the count of non-finite values among the rows of that tail, which
 *   are all the rows the call reads).  The `start` coda reports for candidate s is the iteration label of row cand_rows[s].
 * Every window needs 3 rows (FMCMC_ERR_ARG); N < 3162278 (FMCMC_ERR_UNSUPPORTED).  Argument errors are found before any device
 * call and leave their text in fmcmc_last_error().  The call only enqueues kernels on hip_stream, reads `samples` only, and
 * every sum has a fixed shape that depends on the length of its window alone: a series gives the same bits wherever it sits. */
int64_t fmcmc_heidel_work_len(int64_t nchains, int32_t p, int64_t ncand);
int64_t fmcmc_heidel_out_len(int64_t nchains, int32_t p, int64_t ncand);
int fmcmc_heidel_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                     const int32_t* cols, int32_t p, int64_t half_row, const int64_t* cand_rows, int64_t ncand, double* work,
                     double* out, void* hip_stream);

/* ---- order statistics of every chain on its own ------------------------------------------------------------------------------
 * Window, samples, S, cols as for fmcmc_summary_dev, and its row limits (3 <= N < 3162278).  ranks is a HOST array, read during
 * the call, of 1 <= nranks <= 32 0-based ranks in [0, N), the same for every series (repeats allowed).
 * out (device, nchains p nranks doubles): [nchains][p][nranks], out[c][j][t] = the value with ranks[t] values of the N rows of
 *   chain c, column cols[j] before it in ascending order (-0.0 before +0.0).  They are exact: a radix select on the values' bits,
 *   one workgroup per series, the series held in LDS up to 19456 rows and re-read from global memory every pass beyond.
 * work (device, fmcmc_chain_order_work_len doubles): [nchains][p], left as the count of non-finite values of each series (a NaN
 *   sorts below -Inf or above +Inf by its sign bit).
 * Argument errors are found before any device call and leave their text in fmcmc_last_error().  The call only enqueues one
 * kernel on hip_stream and reads `samples` only; all counts are integers: a series gives the same bits wherever it sits. */
int64_t fmcmc_chain_order_work_len(int64_t nchains, int32_t p, int32_t nranks);
int fmcmc_chain_order_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                          const int32_t* cols, int32_t p, const int64_t* ranks, int32_t nranks, double* work, double* out,
                          void* hip_stream);

/* ---- Raftery-Lewis run-length diagnostic of every chain (coda::raftery.diag), the device part ---------------------------------
 * Window, samples, S, cols and row limits as for fmcmc_summary_dev.  Per series (chain c, column cols[j]):
 *   u = R's type-7 quantile of the N rows of the series at q (0 <= q <= 1): index = 1 + (N - 1) q, lo = floor(index),
 *   hi = ceil(index) (1-based), u = x_(lo) when index == lo or x_(hi) == x_(lo), else (1 - h) x_(lo) + h x_(hi) with h = index - lo
 *   (two rounded products, one rounded sum); Z_t = (x_t <= u), t = 0 .. N - 1.
 *   For each thinning j = j0 .. j0 + nj - 1 (j0 >= 1, 1 <= nj <= 32): rows 0, j, 2 j, ... (m = ceil(N / j) of them), the counts
 *   T[a][b][c] of the triples (Z_i, Z_{i+1}, Z_{i+2}) = (a, b, c), i = 0 .. m - 3, of the thinned series (all 0 when m < 3), and
 *   its last pair (Z_{m-2}, Z_{m-1}) (Z_{m-2} reported as 0 when m == 1).
 * out (device, fmcmc_raftery_out_len(nchains, p, nj) 8-byte words): [nchains][p][4] doubles = {u, x_(lo), x_(hi), count of
 *   non-finite values of the series}, then [nchains][p][nj][10] 64-bit INTEGERS = {T at 4 a + 2 b + c, Z_{m-2}, Z_{m-1}}.
 * work (device, fmcmc_raftery_work_len(nchains, p, N) doubles): [nchains][p][ceil(N / 64)] 64-bit words, left as the
 *   indicator, bit t % 64 of word t / 64 = Z_t.  A call does not depend on what an earlier call left there.
 * BIC, the first thinning that passes, alpha, beta, M, N and I follow from these integers on the host
 * (fmcmc_amd/summary.py: raftery_finish).  Argument errors are found before any device call and leave their text in
 * fmcmc_last_error().  The call only enqueues one kernel on hip_stream and reads `samples` only; everything but u is an
 * integer and u has a fixed arithmetic: a series gives the same bits wherever it sits. */
int64_t fmcmc_raftery_work_len(int64_t nchains, int32_t p, int64_t N);
int64_t fmcmc_raftery_out_len(int64_t nchains, int32_t p, int32_t nj);
int fmcmc_raftery_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                      const int32_t* cols, int32_t p, double q, int64_t j0, int32_t nj, double* work, double* out,
                      void* hip_stream);

/* ---- highest-posterior-density interval of every chain on its own (coda::HPDinterval), the device part ---------------------
 * Window, samples, S, cols and row limits as for fmcmc_summary_dev.  gap is the number of rows the interval spans, formed by the
 * caller (coda: max(1, min(N - 1, round(N prob))), R's round being half-to-even); 1 <= gap <= N - 1 (FMCMC_ERR_ARG).  Per series,
 * with x_(0) <= .. <= x_(N-1) its rows in ascending order (-0.0 before +0.0): i* = the FIRST index of the minimum over
 * i = 0 .. N - gap - 1 of x_(i+gap) - x_(i) (one float64 subtraction each; equal widths, infinite ones included, tie).
 * out (device, nchains p 4 doubles): [nchains][p][4] = {lower = x_(i*), upper = x_(i*+gap), i*, count of non-finite values of
 *   the series}.  coda's attribute Probability is gap / N.
 * work (device, fmcmc_hpd_work_len(nchains, p) doubles): [nchains][p][2], left as {x_(N-gap-1), x_(gap)}, the largest value of
 *   the low tail and the smallest of the high tail.
 * Only the T = N - gap smallest and the T largest rows enter; both tails are held and sorted in LDS, T <= 8192 rows each
 * (FMCMC_ERR_UNSUPPORTED beyond, before any device call: N <= 163840 rows per chain at prob = 0.95).  The call only enqueues one
 * kernel on hip_stream and reads `samples` only; everything is a comparison but the one subtraction per width: a series gives
 * the same bits wherever it sits, and the bits of a sort on the host. */
int64_t fmcmc_hpd_work_len(int64_t nchains, int32_t p);
int fmcmc_hpd_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* cols,
                  int32_t p, int64_t gap, double* work, double* out, void* hip_stream);

/* ---- autocovariances of every chain at freely chosen lags (coda::autocorr, stats::acf), the device part ----------------------
 * Window, samples, S, cols and row limits as for fmcmc_summary_dev (which keeps r_0 .. r_M up to the AR order only).  lags is a
 * HOST array, read during the call, of 1 <= nlags <= 32 distinct row lags in [0, N) (FMCMC_ERR_ARG otherwise), the same for
 * every series.
 * out (device, fmcmc_autocov_out_len(nchains, p, nlags) doubles): [nchains][p][3 + nlags] = {mean, c_0, count of non-finite
 *   values of the series, c_{lags[0]}, .., c_{lags[nlags-1]}}, c_h = (1 / N) sum_{t < N - h} (x_t - mean)(x_{t+h} - mean), the
 *   series centred on its own float64 mean (the bits fmcmc_summary_dev reports), the products summed with fma.  The
 *   autocorrelation is c_h / c_0 (NaN for a constant series, as acf has it).
 * work (device, nchains p doubles): [nchains][p], left as the count of non-finite values of each series.
 * The call only enqueues one kernel on hip_stream and reads `samples` only.  The sum of a lag has a fixed shape that depends on
 * (N, h) alone: not on the other lags of the call, nor on where the series sits. */
int64_t fmcmc_autocov_out_len(int64_t nchains, int32_t p, int32_t nlags);
int fmcmc_autocov_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* cols,
                      int32_t p, const int64_t* lags, int32_t nlags, double* work, double* out, void* hip_stream);

/* ---- pooled ranks of a column and the rank-normalised split R-hat (Vehtari et al. 2021), the device part ------------------------
 * Window, samples, S, cols as for fmcmc_summary_dev; N >= 4 (FMCMC_ERR_ARG), no upper limit from an AR order.  With
 * N' = floor(N / 2) the window of chain c is two split chains: 2 c = rows [0, N'), 2 c + 1 = rows [N - N', N) (an odd N drops
 * its middle row, which takes part in nothing).  The M = 2 nchains N' values of a column are pooled; M < 2^32
 * (FMCMC_ERR_UNSUPPORTED from there: the index of a value is a 32-bit word).  r = the 1-based average rank of a value among the
 * M (ties by numerical equality: -0.0 ties with +0.0), so 2 r = 2 #less + #equal + 1 is an integer;
 * z = fmh_qnorm((r - 0.375) / (M + 0.25)), the difference and the sum exact, one rounded division.
 * med = (x_(M/2 - 1) + x_(M/2)) / 2 of the pooled values in ascending order (0-based; -0.0 read as +0.0).
 *
 * fmcmc_rank_scores_dev: out (device, p M doubles) = [p][2 nchains][N']: z (what = 0) or 2 r (what = 1, exact integers) of the
 *   values x (fold = 0) or |x - med| (fold = 1).  info (device, 2 p doubles) = [p][2] = {count of non-finite values of the
 *   column's window (the dropped row not counted), med}.
 * fmcmc_rank_rhat_dev: out (device, fmcmc_rank_rhat_out_len(nchains, p) = p (8 nchains + 2) doubles), per column:
 *   [2 nchains][2] = {mean, variance (divisor N' - 1)} of the z of every split chain for x (bulk), the same [2 nchains][2] for
 *   |x - med| (tail), then the non-finite count and med.  R-hat follows on the host (fmcmc_amd/summary.py: rhat_finish).
 *   The sums of a split chain have a fixed order (csrc/diag_rank.hpp: split_stats_kernel).
 * work: device scratch of fmcmc_rank_work_len(nchains, p, N) doubles: 1280 + 3 M + 2 ceil(M / 2) + 128 T + 4 ceil(T / 2) with
 *   T = ceil(M / 4096) tiles (two buffers of 64-bit keys and 32-bit indices, the tile x digit table of a pass, the scores); it
 *   does not grow with p: the columns are processed one after another.  A call does not depend on what work held before.
 * The pairs (key, index) are sorted by a stable least-significant-digit radix sort through global memory, 8 passes of 8 bits; a
 * pass whose digit is the same in every key is skipped.  Per column and sort at most 31 kernels and one memset are enqueued
 * (rhat: two sorts and two reductions a column).  The calls only enqueue on hip_stream, take every temporary from work, never
 * synchronise and read `samples` only.  Every count is an integer: the same bits on every call, wherever the window sits.
 * Argument errors are found before any device call and leave their text in fmcmc_last_error(). */
int64_t fmcmc_rank_work_len(int64_t nchains, int32_t p, int64_t N);
int64_t fmcmc_rank_rhat_out_len(int64_t nchains, int32_t p);
int fmcmc_rank_scores_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                          const int32_t* cols, int32_t p, int32_t fold, int32_t what, double* work, double* out, double* info,
                          void* hip_stream);
int fmcmc_rank_rhat_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                        const int32_t* cols, int32_t p, double* work, double* out, void* hip_stream);
/* fmcmc_rank_rhat_dev for ngroups groups of chains_per_group consecutive chains, each group on its own (group g = chains
 * g chains_per_group ..; one model on many datasets: a group = the chains of a dataset), in ONE kernel on the caller's stream.
 * samples, S, row0, N, cols, active and the grouping as for fmcmc_gelman_groups_dev and fmcmc_summary_groups_dev; N >= 4.
 * One workgroup takes one (group, column): it keeps the M = 2 chains_per_group floor(N / 2) keys of the column in LDS, sorts them
 * there, looks every value's rank up in the sorted keys and reduces the scores of every split chain in the order of
 * fmcmc_rank_rhat_dev (csrc/diag_rank_groups.hpp).  M <= fmcmc_rank_groups_max_values() = 8192 (FMCMC_ERR_UNSUPPORTED beyond,
 * before any device call: fmcmc_rank_rhat_dev per group is the form for larger groups).
 * out (device, ngroups p (8 chains_per_group + 2) doubles) = [ngroups][p][8 chains_per_group + 2]: row g is bit for bit the
 *   `out` that fmcmc_rank_rhat_dev writes for the chains of group g alone: the moments, the non-finite count and med, a column
 *   index outside k (all of its values count as non-finite) and -0.0 read as +0.0 included.
 * scores (device, may be NULL): [ngroups][p][2][M], the bulk z then the tail z of every group and column, each in the element
 *   order of fmcmc_rank_scores_dev ([2 chains_per_group][N']) and bit for bit its values (fold = 0, then fold = 1).
 * active[ngroups] (device int32, NULL = all): for a group whose entry is 0 no element of out or scores is written.
 * work: device scratch of fmcmc_rank_rhat_groups_work_len doubles: 1, which the call does not touch (everything lives in LDS,
 *   with or without scores); the length is 0 for arguments the call refuses.  A call does not depend on what work held.
 * The call only enqueues on hip_stream, never synchronises and reads `samples` only.  Every count is an integer and every sum
 * has a fixed order: the same bits on every call, wherever a group sits in the launch and whatever other columns the call holds.
 * Argument errors are found before any device call and leave their text in fmcmc_last_error(). */
int64_t fmcmc_rank_groups_max_values(void);
int64_t fmcmc_rank_rhat_groups_work_len(int64_t ngroups, int64_t chains_per_group, int32_t p, int64_t N);
int fmcmc_rank_rhat_groups_dev(const double* samples, int64_t ngroups, int64_t chains_per_group, int32_t k, int64_t S,
                               int64_t row0, int64_t N, const int32_t* cols, int32_t p, const int32_t* active, double* work,
                               double* scores, double* out, void* hip_stream);

/* ---- rank-normalised bulk and tail effective sample size (Vehtari et al. 2021), the device part -------------------------------
 * Window, samples, S, cols, the split into m = 2 nchains chains of n = floor(N / 2) rows and M = m n < 2^32 as for
 * fmcmc_rank_rhat_dev; N >= 8 (FMCMC_ERR_ARG below).  Per column four series y [m][n] are reduced, in this order: bulk (the
 * scores z of fmcmc_rank_scores_dev), q05 and q95 (1.0 where x <= q, else 0.0; q = R's type-7 quantile at 0.05 / 0.95 of the M
 * pooled values in ascending order, -0.0 read as +0.0: x_lo, or (1 - h) x_lo + h x_hi, two rounded products and a rounded sum),
 * mean (the values).  Of every series: mean_s, var_s of every split chain (as fmcmc_rank_rhat_dev sums them),
 * c_s(t) = (1 / n) sum_{i < n - t} (y_{s,i} - mean_s)(y_{s,i+t} - mean_s) (a rounded difference a value; the products are summed
 * by v_mfma_f64_16x16x4 in an order that (n, t) fix: the same bits on every call, wherever the window sits and whatever other
 * columns the call holds; |error| <= gamma(n + 8) sum |u_i| |u_{i+t}| / n), S(t) = sum_s c_s(t) in the order s = 0, 1, ...
 * The lags come in rounds [0, 256), [256, 512), [512, 1024), ... up to the cap L_cap = n - 2 (lags 0 .. n - 3).  After every round
 * the device runs the pair test of the definition in float64, the same expressions in the same order as
 * fmcmc_amd/summary.py: geyer_tau; the rounds after the one that finds the cut K return at once.
 * out (device, fmcmc_rank_ess_out_len(nchains, p, N) = p (4 (2 m + 2 + L_cap) + 7) doubles), per column: for each of the four
 *   series {[m][2] = mean_s, var_s; L = the lags computed; K; S(0) .. S(L_cap - 1), written below L only}, then {count of
 *   non-finite values, q05, q95, pooled mean, pooled sd (divisor M - 1), least value, largest value}.
 * work: device scratch of fmcmc_rank_ess_work_len(nchains, p, N) doubles (= fmcmc_rank_work_len: the c_s(t) of a round live in
 *   the sort's key buffers, which are dead by then).
 * At most 30 + 4 (2 + 3 R) kernels and one memset a column for R rounds, R <= log2(n / 256) + 3, all on hip_stream; nothing is
 * synchronised and `samples` is only read.  Argument errors are found before any device call. */
int64_t fmcmc_rank_ess_work_len(int64_t nchains, int32_t p, int64_t N);
int64_t fmcmc_rank_ess_out_len(int64_t nchains, int32_t p, int64_t N);
int fmcmc_rank_ess_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                       const int32_t* cols, int32_t p, double* work, double* out, void* hip_stream);
/* fmcmc_rank_ess_dev for ngroups groups of chains_per_group consecutive chains, each group on its own, in ONE kernel on the
 * caller's stream, whatever the number of groups.  samples, S, row0, N, cols, active and the grouping as for
 * fmcmc_rank_rhat_groups_dev; N >= 8 (FMCMC_ERR_ARG below).  One workgroup takes one (group, column): it sorts the
 * M = 2 chains_per_group floor(N / 2) keys of the column in LDS, writes the column's info and scores, and takes the four series
 * through the stats, the rounds of lags on the fp64 matrix core and the pair test, leaving its loop when the cut is known
 * (csrc/diag_ess_groups.hpp).  M <= fmcmc_rank_groups_max_values() = 8192 (FMCMC_ERR_UNSUPPORTED beyond, before any device call:
 * fmcmc_rank_ess_dev per group is the form for larger groups); more than 2^31 - 1 (group, column) pairs are FMCMC_ERR_UNSUPPORTED.
 * out (device, fmcmc_rank_ess_groups_out_len = ngroups p (4 (2 m + 2 + L_cap) + 7) doubles, m = 2 chains_per_group,
 *   L_cap = floor(N / 2) - 2) = [ngroups][p][.]: row (g, j) has the layout of a column of fmcmc_rank_ess_dev's `out`, and every
 *   element that call writes for the chains of group g alone has the same bits here: the stats, L, K, S(t) below L, the info; NaN
 *   keys, -0.0 read as +0.0, a column index outside k and a constant column included.  S(t) at and above L is not written.
 * active[ngroups] (device int32, NULL = all): for a group whose entry is 0 no element of out or work is written.
 * work: device scratch of fmcmc_rank_ess_groups_work_len = ngroups p M doubles: the scores of every (group, column), written and
 *   read by its own workgroup.  A call does not depend on what work held.  Both lengths are 0 for arguments the call refuses.
 * The call only enqueues on hip_stream, never synchronises and reads `samples` only.  Every count is an integer and every sum
 * has a fixed order: the same bits on every call, wherever a group sits in the launch and whatever other columns the call holds.
 * Argument errors are found before any device call and leave their text in fmcmc_last_error(). */
int64_t fmcmc_rank_ess_groups_work_len(int64_t ngroups, int64_t chains_per_group, int32_t p, int64_t N);
int64_t fmcmc_rank_ess_groups_out_len(int64_t ngroups, int64_t chains_per_group, int32_t p, int64_t N);
int fmcmc_rank_ess_groups_dev(const double* samples, int64_t ngroups, int64_t chains_per_group, int32_t k, int64_t S,
                              int64_t row0, int64_t N, const int32_t* cols, int32_t p, const int32_t* active, double* work,
                              double* out, void* hip_stream);

/* ---- WAIC and the pointwise log-likelihood of the closed-form families (Watanabe 2010; loo::waic), the device part -------------
 * The draws are the rows [row0, row0 + N) of the nchains chains of `samples` ([C][k][S], S the row stride): S' = nchains N >= 2
 * draws, every one of the k parameters read; k must be the family's parameter count (FMCMC_ERR_ARG), at most FMCMC_MAX_K.  `m`
 * holds DEVICE pointers X [p][n], y [n] as for fmcmc_mcmc_run_dev.  Per draw s and observation i, l = log p(y_i | theta_s), the
 * likelihood alone (no prior_div term, no guard):
 *   gaussian_linreg  l = -(log sigma + ln sqrt(2 pi)) - 0.5 (y_i - b0 - x_i b)^2 / sigma^2; iid_normal the same with mu = theta_0,
 *                    sigma = theta_1; evaluated as fma(-w, r r, a), a = -(fmh_log(sigma) + ln sqrt(2 pi)), w = 0.5 / (sigma sigma),
 *                    r = the fma chain of v_mfma_f64_16x16x4 over (b0, b, 1) . (1, x_i, -y_i);
 *   logistic         t = eta where y_i != 0, else -eta; l = min(t, 0) - fmh_log1p(fmh_exp(-|t|)).
 * point (device, [n][4]) = {elpd_i, p_waic_i, lppd_i, mean_i}: lppd_i = log((1 / S') sum_s exp l), mean_i = (1 / S') sum_s l,
 *   p_waic_i = sum_s (l - mean_i)^2 / (S' - 1), elpd_i = lppd_i - p_waic_i.
 * total (device, [10]) = {elpd_waic, p_waic, lppd (the sums of the pointwise values), waic = -2 elpd_waic, se_elpd, se_p, se_lppd
 *   (sqrt(n var) of the pointwise values, divisor n - 1: NaN for n = 1), n_high (observations with p_waic_i > 0.4), bad_draws
 *   (draws with a parameter that is not finite or a sigma that is not > 0), bad_points (observations whose four numbers are not
 *   all finite)}; the counts are exact doubles.  A call with bad_draws > 0 is not repaired: its numbers mean nothing.
 * The split of the draws into parts, whose partial results {max, sum of exp, mean, M2} are merged in part order (log-sum-exp, and
 * Chan's update): with T = ceil(N / 16) tiles of 16 rows a chain, unit u = c T + t is tile t of chain c, U = nchains T; a part is
 * upp = max(fmcmc_waic_part_rows() / 16, ceil(U / cap)) consecutive units, cap = 256 while n <= 1024 and 64 beyond;
 * fmcmc_waic_parts(nchains, N, n) = ceil(U / upp) <= cap.  The rule reads (nchains, N, n) only -- never the device, the
 * occupancy or the number of groups --, no float atomics are used and every merge has a fixed order: the same bits on every
 * call and every gfx950, wherever the window sits in `samples`.
 * work: device scratch of fmcmc_waic_work_len(m, ngroups, chains_per_group, N) doubles (0 for arguments the call refuses): for
 *   the Gaussian families a and w of every draw (16 bytes a draw), the bad-draw count of every 256 draws, and the partials
 *   [ngroups][parts][n][4] (20 MB at n = 10^4 with 64 parts).  A call does not depend on what work held.
 * fmcmc_waic_groups_dev: ngroups groups of chains_per_group consecutive chains, group g on dataset g (X, y of m0 are those of
 *   dataset 0, dataset g lies x_stride / y_stride doubles behind: fmcmc_mcmc_run_batch_dev's layout); point [ngroups][n][4] and
 *   total [ngroups][10]; row g is bit for bit what fmcmc_waic_dev writes for the chains of group g and dataset g alone (it is the
 *   same code: fmcmc_waic_dev is the call with one group).  active[ngroups] (device int32, NULL = all) as for
 *   fmcmc_gelman_groups_dev: for a group whose entry is 0 no element of point, total or work is written.  At most 65535 groups.
 * Four kernels are enqueued on hip_stream; nothing is synchronised, `samples` and the model are only read, nothing is written
 * past the documented lengths.  Argument errors are found before any device call and leave their text in fmcmc_last_error(). */
int64_t fmcmc_waic_part_rows(void);
int64_t fmcmc_waic_parts(int64_t nchains, int64_t N, int64_t n);
int64_t fmcmc_waic_work_len(const fmcmc_model* m, int64_t ngroups, int64_t chains_per_group, int64_t N);
int fmcmc_waic_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                   double* work, double* point /* [n][4] */, double* total /* [10] */, void* hip_stream);
int fmcmc_waic_groups_dev(const fmcmc_model* m0, int64_t x_stride, int64_t y_stride, const double* samples, int64_t ngroups,
                          int64_t chains_per_group, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* active,
                          double* work, double* point /* [G][n][4] */, double* total /* [G][10] */, void* hip_stream);

/* ---- PSIS-LOO with Pareto-k diagnostics (Vehtari, Gelman, Gabry 2017; loo::loo with r_eff = 1), the device part ------------------
 * Draws, model, families and the evaluation of l as for fmcmc_waic_dev; the definition is INTEGRATION.md 2.2 (fmcmc_amd/summary.py:
 * loo_host is its executable form).  With r = -l: fmcmc_loo_tail_len(S') = M = ceil(min(0.2 S', 3 sqrt(S'))) (in integers; 0 for
 * S' < 1); the tail of an observation is its M largest r, the cutoff its (M + 1)-th largest, both EXACTLY what a full sort of the
 * device's own r gives, ties included.
 * point (device, [n][6]) = {elpd_loo_i, p_loo_i = lppd_i - elpd_loo_i, lppd_i, pareto_k_i (+Inf: not smoothed), n_eff_i = 1 / sum
 *   of the squared normalised weights, cutoff_i (the (M + 1)-th largest r, unshifted)}.
 * tail (device, [n][M], or NULL) = the M largest r of every observation, ascending, before the smoothing.
 * total (device, [12]) = {elpd_loo, p_loo, lppd, looic = -2 elpd_loo, se_elpd, se_p, se_lppd (as for WAIC), n_k_bad (pareto_k >
 *   min(1 - 1 / log10 S', 0.7)), n_k_very_bad (pareto_k > 1), max_k, bad_draws, bad_points (observations whose elpd, p_loo, lppd
 *   or n_eff is not finite or whose pareto_k is NaN)}; the counts are exact doubles.
 * fmcmc_loo_plan(chains_per_group, N, n, out): the plan, a function of its three arguments alone.  out[0] = M; the subsample is
 *   the units u = 0, out[1], 2 out[1], ... (a unit: WAIC's tile of 16 rows, u = c T + t), out[2] units with out[3] rows; the
 *   threshold of an observation is the out[4]-th largest r of its subsample, chosen so that out[5] draws are expected above it;
 *   out[6] = the capacity of an observation's buffer (the power of two >= 3 M).  An observation whose count of draws above the
 *   threshold is in [M + 1 - ties, out[6]] is served from its buffer; any other takes the exact fallback (a radix select over all
 *   draws).  With out[1] = 1 the subsample is every draw and the threshold is exact.  out[7] = the number of tail lengths at
 *   which a kernel or its launch changes form, out[8 ...] those M (5: the fit and the smoothing start; 8193: the finishing
 *   kernel's LDS passes 64 KB); the rest of the FMCMC_LOO_PLAN_LEN entries are 0.
 * work: device scratch of fmcmc_loo_work_len(...) doubles (0 for arguments the call refuses): WAIC's, then per observation the
 *   subsample (16 out[2] keys), the buffer (out[6] keys), 8 state words {threshold key, count above, count equal, 1 if the
 *   fallback served it, ...} at fmcmc_loo_state_offset(...) + 8 (g n + i) (8-byte integers; what a call leaves there may be read),
 *   and a 256-bin histogram.  A call does not depend on what work held.
 * Tails up to M = 16384 (S' <= 29826161); beyond: FMCMC_ERR_UNSUPPORTED.  fmcmc_loo_groups_dev, active, the streams, the checks
 * and the bit-for-bit equality of a group with its single call are those of fmcmc_waic_groups_dev. */
#define FMCMC_LOO_PLAN_LEN 16
int64_t fmcmc_loo_tail_len(int64_t S);
int fmcmc_loo_plan(int64_t chains_per_group, int64_t N, int64_t n, int64_t out[FMCMC_LOO_PLAN_LEN]);
int64_t fmcmc_loo_work_len(const fmcmc_model* m, int64_t ngroups, int64_t chains_per_group, int64_t N);
int64_t fmcmc_loo_state_offset(const fmcmc_model* m, int64_t ngroups, int64_t chains_per_group, int64_t N);
int fmcmc_loo_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                  double* work, double* point /* [n][6] */, double* tail /* [n][M] or NULL */, double* total /* [12] */,
                  void* hip_stream);
int fmcmc_loo_groups_dev(const fmcmc_model* m0, int64_t x_stride, int64_t y_stride, const double* samples, int64_t ngroups,
                         int64_t chains_per_group, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* active,
                         double* work, double* point /* [G][n][6] */, double* tail /* [G][n][M] or NULL */,
                         double* total /* [G][12] */, void* hip_stream);

/* ---- Leave-one-out predictive checks from the PSIS weights (loo::E_loo, bayesplot::ppc_loo_pit), the device part ------------------
 * The whole of fmcmc_loo_dev on the same arguments, then one more sweep of the draws; the definition is INTEGRATION.md 2.2
 * (fmcmc_amd/summary.py: loo_predictive_host is its executable form).  m: FMCMC_FAM_GAUSSIAN_LINREG or FMCMC_FAM_LOGISTIC;
 * FMCMC_FAM_IID_NORMAL: FMCMC_ERR_UNSUPPORTED.  With lambda_j = min(the smoothed log weight of tail rank j, 0), R the largest r and
 * c the cutoff, a draw whose r = v is below c weighs exp(v - R); above c, the mean of exp(lambda_j) over the tail ranks whose r
 * equals v; at c, [sum of exp(lambda_j) over the c_T tail ranks equal to c + (count(c) - c_T) exp(c - R)] / count(c).  "Equal"
 * is the equality of the device's own r.  E_loo[h] = sum_s omega_s h_s / sum_s omega_s.
 * point (device, [n][6]) = {mean_i, sd_i, pit_i, pareto_k_i, n_eff_i, elpd_loo_i}: gaussian_linreg, d = eta - y_i: mean_i = y_i +
 *   E_loo[d], sd_i = sqrt(E_loo[d^2 + sigma^2] - E_loo[d]^2), pit_i = E_loo[Phi(-d (1 / sigma))], Phi the lower tail of
 *   fmh_pnorm_both; logistic: mean_i = E_loo[expit(eta)], sd_i = sqrt(mean_i (1 - mean_i)), pit_i = NaN.  The last three are
 *   fmcmc_loo_dev's.  A row whose fmcmc_loo_dev row is NaN, or whose counts of draws above and at the cutoff are not those of the
 *   tail (the sweep found other r than the selection did), is NaN.
 * loo_point (device, [n][6], or NULL) and total[0 .. 12): bit for bit what fmcmc_loo_dev writes to point and total on the same
 *   arguments; total[12] = the rows of `point` whose mean or sd is not finite.  total has 13 entries.
 * work: device scratch of fmcmc_loo_predictive_work_len(m, nchains, N) doubles (0 for arguments the call refuses; needs no
 *   device): fmcmc_loo_work_len(m, 1, nchains, N), then the tail, its capped log weights and the run means [3][n][M], 8 n
 *   doubles, 1 / sigma and sigma^2 per draw (gaussian_linreg) and the partials [parts][n][10].  A call does not depend on what
 *   work held.
 * Every kernel is enqueued on hip_stream; nothing is synchronised, there are no floating-point atomics and every sum has a fixed
 * order: the same bits on every call, wherever the window sits in `samples`.  The checks, their texts and the status codes are
 * fmcmc_loo_dev's. */
int64_t fmcmc_loo_predictive_work_len(const fmcmc_model* m, int64_t nchains, int64_t N);
int fmcmc_loo_predictive_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0,
                             int64_t N, double* work, double* point /* [n][6] */, double* loo_point /* [n][6] or NULL */,
                             double* total /* [13] */, void* hip_stream);

/* ---- WAIC and PSIS-LOO of a user-defined model: the pointwise log-likelihood as a batched callback -----------------------------
 * Batched pointwise log-likelihood: ll[b][i] = log p(y_i | theta[b][0..k-1]) for b < B, i < n, the likelihood alone (no prior),
 * row-major.  The rules of fmcmc_logpost_fn: theta and ll are DEVICE pointers (theta is read-only), the function is called on
 * the calling host thread, its work is enqueued on hip_stream or it synchronises before returning; 0 = ok, anything else
 * abandons the call with FMCMC_ERR_FUN, and fmcmc_last_error() names the pass ("fold"; "sample", "collect", "histogram 0" ..
 * "histogram 7", "second collect"), the block (0-based within the pass) and the code. */
typedef int (*fmcmc_pointwise_fn)(const double* theta /* [B][k] */, int64_t B, int32_t k, int64_t n,
                                  double* ll /* [B][n], row-major */, void* hip_stream, void* user);

/* fmcmc_waic_dev / fmcmc_loo_dev with the family replaced by `fun` and its n >= 1 observations: the draws, the window, the plan of
 * parts (fmcmc_waic_parts, fmcmc_loo_plan) and the layouts and meanings of point, tail and total are theirs, with bad_draws = the
 * draws with a parameter that is not finite (no sigma is known here); an l that is NaN makes its observation a bad_point, an l
 * of -Inf is a draw of likelihood zero.  1 <= k <= FMCMC_MAX_K.
 * The S' x n matrix is never stored.  The draws are taken block after block: a block is a run of consecutive units (WAIC's tile
 * of 16 rows of one chain, u = c T + t, the last tile of a chain shorter), gathered into a row-major [B][k] buffer, handed to
 * `fun`, and the [B][n] block it fills is read once before the next one overwrites it.  block_rows bounds B: it is rounded up to
 * whole units; 0 is the library's choice, fmcmc_pointwise_block_rows(n, nchains, N, 0): b = 2^25 / (16 n) units (a block of
 * about 256 MiB), all U units where b >= U, else b rounded down to whole parts of the plan where a part fits, else max(1, b).
 * Every floating sum has an order that (nchains, N, n) alone decide: point, tail and total hold the same bits
 * for every block_rows, on every call, wherever the window sits in `samples`.
 * fmcmc_waic_fun_dev: one sweep of `fun` over the S' draws (pass "fold"); kernels and callbacks are enqueued on hip_stream and
 *   nothing is synchronised.
 * fmcmc_loo_fun_dev: `fun` on the rows of the plan's subsample only (pass "sample": out[3] rows of fmcmc_loo_plan), the threshold,
 *   one sweep over all draws ("collect"), the flags.  Then the call SYNCHRONISES hip_stream once, to read how many observations
 *   are flagged: with none (the common case) the finish follows; otherwise eight more sweeps ("histogram d") and a last one
 *   ("second collect"), which use the flagged observations' columns only.  That is the only synchronisation.
 * work: device scratch of fmcmc_*_fun_work_len(n, nchains, N, block_rows) doubles (0 for arguments the call refuses; the same
 *   block_rows as the call's): a count per unit, the partials [parts][n][4], the accumulators carried from block to block
 *   [2][4][6][n], the two buffers [B][FMCMC_MAX_K] and [B][n]; for LOO then the subsample, the buffers, the state words at
 *   fmcmc_loo_fun_state_offset(...) + 8 i (as for fmcmc_loo_state_offset; -1 for arguments the call refuses) and the histograms
 *   of fmcmc_loo_dev.  A call does not depend on what work held.
 * Argument errors are found before any device call and leave their text in fmcmc_last_error(); `samples` is only read; nothing
 * is written past the documented lengths.  After FMCMC_ERR_FUN point, tail and total hold nothing of meaning; the next call is
 * not affected. */
int64_t fmcmc_pointwise_block_rows(int64_t n, int64_t nchains, int64_t N, int64_t block_rows);
int64_t fmcmc_waic_fun_work_len(int64_t n, int64_t nchains, int64_t N, int64_t block_rows);
int fmcmc_waic_fun_dev(fmcmc_pointwise_fn fun, void* user, int64_t n, const double* samples, int64_t nchains, int32_t k,
                       int64_t S, int64_t row0, int64_t N, int64_t block_rows, double* work,
                       double* point /* [n][4] */, double* total /* [10] */, void* hip_stream);
int64_t fmcmc_loo_fun_work_len(int64_t n, int64_t nchains, int64_t N, int64_t block_rows);
int64_t fmcmc_loo_fun_state_offset(int64_t n, int64_t nchains, int64_t N, int64_t block_rows);
int fmcmc_loo_fun_dev(fmcmc_pointwise_fn fun, void* user, int64_t n, const double* samples, int64_t nchains, int32_t k,
                      int64_t S, int64_t row0, int64_t N, int64_t block_rows, double* work,
                      double* point /* [n][6] */, double* tail /* [n][M] or NULL */, double* total /* [12] */,
                      void* hip_stream);

/* ---- Fitted values, predictions at new covariates and their credible bands, the device part -------------------------------------
 * The definition is INTEGRATION.md 2.2 (fmcmc_amd/summary.py: predict_host is its executable form).  Draws and window as for
 * fmcmc_waic_dev; S' = nchains N >= 2 (at most 2^31 - 1).  m: FMCMC_FAM_GAUSSIAN_LINREG or FMCMC_FAM_LOGISTIC; m->X is the DEVICE
 * pointer to the new points Xn in the model's own layout [p][n] (n = m->n points), m->intercept applies, m->y is not read.
 * FMCMC_FAM_IID_NORMAL has no covariates: FMCMC_ERR_UNSUPPORTED.
 *   eta[s][i] = (b0_s) + sum_j Xn[i][j] beta_sj, the fma chain of v_mfma_f64_16x16x4 over (b0, beta) . (1, x_i);
 *   kind 0 (linpred): q = eta; kind 1 (epred): q = eta (Gaussian), q = 1 / (1 + exp(-eta)) (logistic; with e = fmh_exp(-|eta|):
 *   1 / (1 + e) for eta >= 0, e / (1 + e) below).
 * point (device, [n][4 + nprobs]) = {mean_i and sd_i of q over the draws (divisor S' - 1), sd_pred_i = sqrt(var_i(eta) + mean_s
 *   sigma_s^2) (the sd of the posterior predictive of a new y at x_i; NaN for the logistic family), the mean of eta, and the
 *   type-7 quantiles of q at probs[0 .. nprobs)}: the two neighbouring order statistics are EXACTLY what a full sort of the
 *   device's own eta gives, ties included; they are mapped to q first and then interpolated, (1 - h) lo + h hi in two rounded
 *   products and one rounded sum, lo itself where h = 0 or hi == lo.  probs is a HOST array, read during the call; nprobs <= 16.
 * total (device, [4]) = {S', bad_draws (a coefficient that is not finite, Gaussian: a sigma that is not > 0), the mean of
 *   sigma^2 (NaN for the logistic family), 0}.  A call with bad_draws > 0 is not repaired: its numbers mean nothing.
 * The draws are split into parts as for fmcmc_waic_dev with n := m->n (fmcmc_waic_parts); partial {count, mean, M2} are merged
 * by Chan's update in a fixed order and the order statistics are selected on integer keys (integer atomics only): the same bits
 * on every call and every gfx950, wherever the window sits in `samples`; the row of a point does not depend on the other points
 * of a call while both calls have n <= 1024 or both n > 1024.
 * work: device scratch of fmcmc_predict_work_len(m, nchains, N, nprobs) doubles (0 for arguments the call refuses; needs no
 *   device): two sums per 256 draws, the partials [min(256, ceil(U / 32))][n][4], two 8-byte state words per point and rank
 *   ([n][2 nprobs][2]) and the 256-bin histograms of min(2 nprobs, 8) ranks per point (the ranks are selected in batches of 8,
 *   each batch in eight passes over all draws).  Never smaller for a larger N, n or nprobs.  A call does not depend on what work held.
 * Every kernel is enqueued on hip_stream; nothing is synchronised, `samples` and the model are only read, nothing is written
 * past the documented lengths.  Argument errors are found before any device call and leave their text in fmcmc_last_error(). */
int64_t fmcmc_predict_work_len(const fmcmc_model* m, int64_t nchains, int64_t N, int32_t nprobs);
int fmcmc_predict_dev(const fmcmc_model* m /* X = Xn [p][m->n]; y not read */, const double* samples, int64_t nchains, int32_t k,
                      int64_t S, int64_t row0, int64_t N, int32_t kind, const double* probs /* host */, int32_t nprobs,
                      double* work, double* point /* [n][4 + nprobs] */, double* total /* [4] */, void* hip_stream);

/* ---- The posterior predictive distribution of a new observation y at a point: quantiles and PIT, the device part ----------------
 * The definition is INTEGRATION.md 2.2 (fmcmc_amd/summary.py: predictive_host is its executable form).  Draws, window and eta as
 * for fmcmc_predict_dev; S' = nchains N >= 2 (at most 2^31 - 1).  m: FMCMC_FAM_GAUSSIAN_LINREG only; m->X is the DEVICE pointer
 * to the points Xn [p][n], m->y the DEVICE pointer to the n values to take the PIT at, or NULL.  FMCMC_FAM_LOGISTIC (the
 * predictive distribution of its y is Bernoulli(mean of epred), which fmcmc_predict_dev returns) and FMCMC_FAM_IID_NORMAL:
 * FMCMC_ERR_UNSUPPORTED.
 *   F_i(t) = (1 / S') sum_s Phi((t - eta_si) / sigma_s), Phi = fmh_pnorm_both (include/fmh_detmath.h); u = (t - eta) (1 / sigma).
 *   The quantile at p is the root of g(t) = F_i(t) - p; for p > 1/2 the upper tails are summed and g = (1 - p) - (1 - F_i)(t).
 * point (device, [n][4 + 4 nprobs]) = {mean_i of eta, sd_pred_i = sqrt(var_i(eta) + mean_s sigma_s^2) (both as fmcmc_predict_dev
 *   defines them), pit_i = F_i(y_i), pit_upper_i = 1 - F_i(y_i) (two direct sums; NaN without m->y), then per prob: t (the
 *   quantile, or the last iterate), g at t, the width hi - lo of the bracket, the pass at which it finished (0: not yet)}.
 *   A (point, prob) is finished when |g| <= c 2^-52 min(p, 1 - p), c the rounding budget of the sum (csrc/diag_predictive.hpp:
 *   pdv_c; a function of the plan), or when the bracket is no wider than 2 ulp of its larger end.
 * total (device, [6]) = {S', bad_draws (as fmcmc_predict_dev), the mean of sigma^2, min sigma, max sigma, the count of (point,
 *   prob) not yet finished}.  A call with bad_draws > 0 is not repaired: its numbers mean nothing.
 * probs: a HOST array, read during the call; nprobs <= 16 (0: the PIT and the head alone), each strictly inside (0, 1).
 * npasses >= 1 evaluation passes are enqueued, each one sweep over all draws per batch of 8 probs (a workgroup whose points are all
 *   finished returns at once).  resume = 0 starts: the draw pass, the fold, the brackets, the PIT.  resume = 1 continues from
 *   the state that a previous call left in `work`: the caller passes the same arguments and the same `work`; two calls of 4 passes
 *   give the bits of one call of 8.
 * The draws are split into parts as for fmcmc_waic_dev with n := m->n; every sum has a fixed order, there are no floating-point
 * atomics: the same bits on every call and every gfx950, wherever the window sits in `samples`; the row of a point does not
 * depend on the other points of a call while both calls have n <= 1024 or both n > 1024.
 * work: device scratch of fmcmc_predictive_work_len(m, nchains, N, nprobs) doubles (0 for arguments the call refuses; needs no
 *   device): four values per 256 draws, 1 / sigma per draw, the fold's partials [parts][n][4], a head [n][4], the state
 *   [n][nprobs + 1][8], the evaluation's partials [parts][n][8][2] and the PIT's [parts][n][2].  A call with resume = 0 does not
 *   depend on what work held.
 * Every kernel is enqueued on hip_stream; nothing is synchronised, `samples` and the model are only read, nothing is written
 * past the documented lengths.  Argument errors are found before any device call and leave their text in fmcmc_last_error(). */
int64_t fmcmc_predictive_work_len(const fmcmc_model* m, int64_t nchains, int64_t N, int32_t nprobs);
int fmcmc_predictive_dev(const fmcmc_model* m /* X = Xn [p][m->n]; y [m->n] or NULL */, const double* samples, int64_t nchains,
                         int32_t k, int64_t S, int64_t row0, int64_t N, const double* probs /* host */, int32_t nprobs,
                         int32_t npasses, int32_t resume, double* work, double* point /* [n][4 + 4 nprobs] */,
                         double* total /* [6] */, void* hip_stream);

/* ---- Posterior predictive checks from replicated data (Gelman, Meng and Stern 1996; bayesplot::ppc_stat), the device part ---------
 * The definition is INTEGRATION.md 2.2 (fmcmc_amd/summary.py: ppc_host is its executable form).  Draws, window and eta as for
 * fmcmc_predict_dev at the model's own X; S' = nchains N >= 2.  m: FMCMC_FAM_GAUSSIAN_LINREG or FMCMC_FAM_LOGISTIC with the DEVICE
 * pointers X [p][n] and y [n]; FMCMC_FAM_IID_NORMAL: FMCMC_ERR_UNSUPPORTED.
 *   Draw s = row r of chain c of the window has the keys (seed, chain id = chain_base + c, id = id0 + id_step r); both ids must fit
 *   32 bits (else FMCMC_ERR_UNSUPPORTED).  The uniform of observation i is lane i & 1 of fmh_uniform2(seed, id, chain id, i >> 1,
 *   FMH_STREAM_PPC) (include/fmh_philox.h).  Gaussian: z = fmh_qnorm(u), y_rep = fmh_fma(sigma_s, z, eta_si).  Logistic: y_rep =
 *   1 if u < expit(eta_si), else 0, expit in the branch form of fmcmc_predict_dev.
 * stats (device, [nchains][6][N], the layout of `samples`) = per draw {mean, sd (divisor n - 1; NaN for n = 1), min, max of y_rep
 *   over the n observations, chisq_rep, chisq_obs}: Gaussian chisq_rep = sum z^2, chisq_obs = sum ((y_i - eta_si) (1 / sigma_s))^2;
 *   logistic each is sum fmh_exp(v ? -eta : eta), v = y_rep resp. y.  The fold over i = 0 .. n - 1 is a function of n alone: lane
 *   c = 0 .. 15 takes i = c, c + 16, ... in that order with its sums shifted by the first value; the 16 lanes are merged in lane
 *   order by Chan's update (sums: added; min, max: compared).  No floating-point atomics: a draw's six numbers depend on its theta,
 *   its two ids, the model and the seed alone, not on nchains, N, row0 or the other draws.
 * tobs (HOST, [4]) = T(y) for mean, sd, min, max.  total (device, [17]) = {S', bad_draws (as fmcmc_predict_dev), then for each of
 *   mean, sd, min, max, chisq the counts of draws with T_rep > T_obs, T_rep == T_obs, and a value that is not finite on either
 *   side (counted in neither of the first two)}; for chisq the comparison is chisq_rep against the draw's own chisq_obs.
 * work: device scratch of fmcmc_ppc_work_len(m, nchains, N) doubles (0 for arguments the call refuses; needs no device): two sums
 *   per 256 draws and 16 integer words.  A call does not depend on what work held.
 * fmcmc_ppc_yrep_dev writes the replicated data sets themselves, yrep (device, [nsel][n]), of nsel <= 65535 selected draws
 *   (sel_chain[i] in [0, nchains), sel_row[i] in [0, S): HOST arrays, read during the call; the id of row r is id0 + id_step r,
 *   so id0 belongs to row 0 of the buffer): the same text per element, bit for bit what the fold of fmcmc_ppc_dev consumed.  It
 *   needs nchains S >= 2 and does not read m->y.
 * Every kernel is enqueued on hip_stream; nothing is synchronised, `samples` and the model are only read, nothing is written
 * past the documented lengths.  Argument errors are found before any device call and leave their text in fmcmc_last_error().
 * fmcmc_ppc_elem_host: the host build of the same per-element text on host arrays (needs no device): given eta [n] of the draw
 *   with the keys (seed, chain_id, id) and its sigma (Gaussian), yrep [n] and variate [n] = z (Gaussian) or u (logistic), bit
 *   for bit the device's. */
int64_t fmcmc_ppc_work_len(const fmcmc_model* m, int64_t nchains, int64_t N);
int fmcmc_ppc_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                  uint64_t seed, int64_t chain_base, int64_t id0, int64_t id_step, const double* tobs /* host, [4] */,
                  double* work, double* stats /* [nchains][6][N] */, double* total /* [17] */, void* hip_stream);
int fmcmc_ppc_yrep_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, uint64_t seed,
                       int64_t chain_base, int64_t id0, int64_t id_step, const int64_t* sel_chain /* host */,
                       const int64_t* sel_row /* host */, int64_t nsel, double* yrep /* [nsel][n] */, void* hip_stream);
int fmcmc_ppc_elem_host(int32_t family, uint64_t seed, int64_t chain_id, int64_t id, int64_t n, const double* eta, double sigma,
                        double* yrep, double* variate);

/* Materialises the canonical Philox stream of a call in device memory, in the FED layout of fmcmc_run:
 * logu[C][nsteps] (entry i-1 = log accept-uniform of loop step i), z[C][nsteps][kz] (N(0,1) when student_df == 0;
 * Student-t with student_df degrees of freedom when student_df > 0 -- kernel_ram: kf for the default qfun rt(k, k),
 * fmcmc_kernel.ram_df for FMCMC_RAM_QFUN_T_DF, 0 for FMCMC_RAM_QFUN_NORMAL (R/kernel_ram.R:68) -- ; U(0,1) of the uniform
 * kernels when student_df == -1).  A double since ABI 4 (it was an int32 and could not carry a fractional df).  A sweep run with
 * rng_mode = FMCMC_RNG_FED on these buffers is bit-identical to rng_mode = FMCMC_RNG_PHILOX; callers that
 * launch many sweeps can reuse the buffers instead of letting the library allocate them per call. */
int fmcmc_rng_stream_dev(uint64_t seed, int64_t step_base, int64_t chain_base, int64_t nchains, int64_t nsteps,
                         int32_t kz, double student_df, double* logu, double* z, void* hip_stream);

/* Diagnostic: evaluate the canonical math / RNG primitives on the device, element-wise
 * (which: 0 log, 1 exp, 2 log1p, 3 qnorm, 4 log accept-u, 5 normal, 6 student-t(df=x), 7 sqrt,
 * 8 reciprocal, 9 fused log1p(exp(x)) for x <= 0, 10 uniform variate, 11 Phi(x) and 12 1 - Phi(x) of fmh_pnorm_both,
 * 13 tan on [0, pi/2]). Used by tests to prove host/device bit-equality of include/fmh_*.h.
 * fmcmc_detmath_host: the host build of the same text for which = 11 and 12 (x and out are host arrays; needs no device); the
 * other codes have their host twin in the CPU oracle. */
int fmcmc_detmath_dev(int which, const double* x, double* out, int64_t n, uint64_t seed,
                      void* hip_stream);
int fmcmc_detmath_host(int which, const double* x, double* out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* FMCMC_AMD_H */
