// mh_user.hpp -- the device half of a USER-DEFINED transition kernel (fmcmc_mcmc_run_user_dev; R/kernel.R:136-317, kernel_new):
//   mh_user_step<NTH>     the accept / store half of mh_fun_step (mh_fun.hpp) and nothing else: the carried values, row 1, the
//                         decision and the write-back ARE that kernel's, the pieces of mh_rowowner.hpp.  The callback path cuts the step
//                         at the evaluation; a user kernel cuts it once more, at the proposal: theta1 [C][k] comes from the
//                         caller's proposal callback, f1 [C] from the evaluation, the log-ratio [C] from the caller's logratio
//                         callback (none: f1 - f0 formed here, the decision of the built-in kernels bit for bit).
//                           [START]   row 1: f0 = f(initial), theta1 = theta0, the row stored, status / accept bits reset
//                           [ACCEPT]  step i: NaN checks, log u < ratio, theta0 / f0, the kept row, draws, logpost, accept bit
//                                     (R/mcmc.R:754-778)
//                         No proposal, no adaptation, no Sigma.  Layout of mh_fun_step: one workgroup per chain, thread r =
//                         parameter r; NTH = 64 (k <= 64, "user") or 256 ("user-wg").  Nothing is kept in LDS: a thread holds its
//                         parameter of theta0 / theta1, the chain's scalars are uniform.
//   logpost_eval_kernel   the three families' canonical log-posterior of C caller-given parameter vectors, out[c] = f(theta[c, ]):
//                         the oracle's logpost_canon (fmcmc_oracle.c) bit for bit.  One workgroup of NT = 512 threads per chain,
//                         thread = canonical lane: lane l accumulates the observations i = l, l + 512, .. in index order, the
//                         lanes combine by the xor butterfly (wave_xor_sum, then the eight waves' values pairwise), thread 0
//                         evaluates the closed form.  X column-major [p][n]: a wavefront reads 64 consecutive doubles of a
//                         column; the coefficients are broadcast from LDS.  Its body is logpost_canon_wg, a device function
//                         that mh_sweep_batch (mh_batch.hpp) calls as well, with the data wherever that kernel keeps them.
// Compiled into k_fun.hip only (FMH_WITH_FUN_KERNEL); mh_engine.hip includes the argument structs.
#pragma once
#include "mh_rowowner.hpp"

namespace {

struct UserArgs {
  int k, rng_mode;
  long long nchains, nsteps, burnin, thin, ldS, chain_base, step_base;
  unsigned long long seed;
  const double* fed_logu;
  // state
  double* theta0;
  double* f0;
  // out
  double* samples;
  double* logpost;
  double* draws;
  long long* accept_count;
  unsigned int* accept_bits;
  int* status;
  long long* status_step;
  double* status_theta;
  // the caller's proposal [C][k], its evaluation [C] and the caller's log-ratio [C] (nullptr: f1 - f0)
  const double* th1;
  const double* f1;
  const double* logratio;
  // this launch
  long long step;            // the loop step whose proposal has been evaluated (1: row 1)
  int phase;                 // UPH_*
};

enum { UPH_START = 1, UPH_ACCEPT = 2 };

struct EvalArgs {
  int family, p, intercept, guard;
  long long n, nchains;
  double prior_div;
  const double* X;           // [p][n]
  const double* y;           // [n]
  const double* hs;          // logistic: the data-only sums of logit_hs_kernel (mh_prep.hpp)
  const double* theta;       // [C][k]
  double* out;               // [C]
};

__host__ __device__ inline int eval_params(int family, int p, int intercept) {   // k of a family
  return family == FMCMC_FAM_GAUSSIAN_LINREG ? (intercept ? 1 : 0) + p + 1 : family == FMCMC_FAM_LOGISTIC ? (intercept ? 1 : 0) + p
       : family == FMCMC_FAM_IID_NORMAL ? 2 : -1;
}

#ifdef FMH_WITH_FUN_KERNEL   /* compiled into k_fun.hip only */
template <int NTH>
__global__ __launch_bounds__(NTH) void mh_user_step(const UserArgs A) {
  const int r = threadIdx.x, k = A.k;
  const long long c = blockIdx.x;            // one chain per workgroup (grid = nchains)
  const long long i = A.step;
  const bool par = r < k, start = A.phase == UPH_START;
  const double th1 = par ? A.th1[c * k + r] : 0.0;
  double th0 = par ? A.theta0[c * k + r] : 0.0;
  RoCarried ch = ro_carried(A, c, start);   // the chain's carried values (uniform: every thread keeps them)
  __syncthreads();   // (every wave has read the status before thread 0 writes it)

  if (start)   // row 1 (R/mcmc.R:728-735)
    ro_row1(A, c, r, NTH, par, &th0, &th1, ch.f0);
  else if (ch.status == FMCMC_CHAIN_OK)   // accept / store of step i (R/mcmc.R:754-778); theta0 is this thread's own: no barrier
    ro_accept_store(A, c, r, par, i, A.f1[c], A.logratio ? A.logratio[c] : A.f1[c] - ch.f0, ch, &th0, &th1, []() {});
  ro_write_back(A, c, r, par, ch, &th0);
}

// The canonical log-posterior of ONE parameter vector by the NT threads of a workgroup (the oracle's logpost_canon): the body of
// logpost_eval_kernel and of mh_sweep_batch's evaluation (mh_batch.hpp).  th: the k parameters (global memory or LDS); xat(j, i)
// / yat(i): element i of column j of X / of y, from wherever the caller keeps the data; s_th [ic + p], s_w [NW]: LDS scratch.
// Every thread calls it (two barriers; the caller's th is visible to the workgroup before); thread 0 returns f, the others 0.
// The caller puts a barrier between thread 0's return and the next call.
template <class FX, class FY>
__device__ __forceinline__ double logpost_canon_wg(int family, int p, int intercept, int guard, long long n, double prior_div,
                                                   const double* hs, const double* th, FX xat, FY yat, double* s_th, double* s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool logit = family == FMCMC_FAM_LOGISTIC;
  const int pp = (family == FMCMC_FAM_IID_NORMAL) ? 0 : p;
  const int ic = (family == FMCMC_FAM_IID_NORMAL) ? 1 : intercept;
  const int k = eval_params(family, p, intercept);
  // the coefficients the observation loop reads: the logistic ones scaled by 64 (exact), so that the table's reduced argument
  // falls out of eta (include/fmh_detmath.h, fmh_logit_g_scaled)
  for (int j = tid; j < ic + pp; j += NT) s_th[j] = logit ? th[j] * FMH_LG_SCALE : th[j];
  __syncthreads();
  double acc = 0.0;
  for (long long i = tid; i < n; i += NT) {
    double m = ic ? s_th[0] : 0.0;
    for (int j = 0; j < pp; j++) m = fmh_fma(xat(j, i), s_th[ic + j], m);
    if (logit) {
      acc = acc + fmh_logit_g_scaled(fmh_abs(m));
    } else {
      const double r = yat(i) - m;
      acc = fmh_fma(r, r, acc);
    }
  }
  const double v = wave_xor_sum(acc);
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  if (tid != 0) return 0.0;
  const double tot = ((s_w[0] + s_w[1]) + (s_w[2] + s_w[3])) + ((s_w[4] + s_w[5]) + (s_w[6] + s_w[7]));
  double f;
  if (logit) {   // logl = sum_j b_j hs_j - sum_i g(|eta_i|) - sum_j b_j^2 / prior_div
    double lin = 0.0;
    for (int j = 0; j < k; j++) lin = fmh_fma(th[j], hs[j], lin);
    f = lin - tot;
    if (prior_div != 0.0) {
      double ss = 0.0;
      for (int j = 0; j < k; j++) ss = fmh_fma(th[j], th[j], ss);
      f = f - ss / prior_div;
    }
  } else {
    const double sigma = th[ic + pp];
    if (sigma < 0.0 || fmh_isnan(sigma)) {
      f = fmh_nan();
    } else if (sigma == 0.0) {
      f = -fmh_inf();
    } else {
      const double t1 = fmh_log(sigma) + FMH_LN_SQRT_2PI;
      const double q = (0.5 * tot) / (sigma * sigma);
      f = -((double)n * t1) - q;
    }
  }
  if (guard && !fmh_isfinite(f)) f = -fmh_inf();
  return f;
}

__global__ __launch_bounds__(NT) void logpost_eval_kernel(const EvalArgs A) {
  __shared__ double s_th[MAXK], s_w[NW];
  const long long c = blockIdx.x, n = A.n;   // one chain per workgroup (grid = nchains)
  const int k = eval_params(A.family, A.p, A.intercept);
  const double f = logpost_canon_wg(A.family, A.p, A.intercept, A.guard, n, A.prior_div, A.hs, A.theta + c * k,
                                    [&](int j, long long i) { return A.X[(long long)j * n + i]; }, [&](long long i) { return A.y[i]; },
                                    s_th, s_w);
  if (threadIdx.x == 0) A.out[c] = f;
}
#endif  // FMH_WITH_FUN_KERNEL

}  // namespace
