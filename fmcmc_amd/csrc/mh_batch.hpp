// mh_batch.hpp -- mh_sweep_batch<LDS_DATA, MASKED>: ONE model fitted to MANY datasets in one launch (fmcmc_mcmc_run_batch_*; Python:
// MCMC_batch).  The callback path (mh_fun.hpp) cuts a step at the evaluation and returns to the host; here the evaluation is a
// family's closed form, so the whole loop i = 2 .. nsteps runs inside one kernel:
//   row 1      f0 = f(initial), kernel state initialised, row stored                                    (mh_fun_step: START)
//   step i     f1 = f(theta1); kernel_ram: the adaptation on f(un-reflected theta1), the reflection and -- bounded only -- the
//              second evaluation (RAM); NaN checks, log u < f1 - f0, the kept row (ACCEPT); the variates, the proposal and
//              kernel_adapt's adaptation of step i + 1 (PROPOSE)
//   the end    the Sigma square handed on, the carried values written back                              (FINISH)
// in the order mh_fun_step<64> and its host loop (run_fun) give the phases: the same bits as the callback path evaluating the
// family, the oracle's and the family path's.
//
// Layout: one workgroup of NT = 512 threads per chain, grid = nchains; no hand-over between workgroups, so a grid larger than
// the card queues.  Local chain c belongs to dataset d = c / chains_per_model: X + d x_stride ([p][n] column-major),
// y + d y_stride, hs + d hs_stride (logistic).  The 512 threads ARE the canonical lanes of the evaluation (logpost_canon_wg,
// mh_user.hpp: the body of logpost_eval_kernel); thread r < k is also the row owner of parameter r (mh_rowowner.hpp, fun_propose).
// theta0, theta1, the variates, kernel_adapt's LDL^T factor, running row sum and mean_prev live in LDS for the whole call, f0,
// the accept count, abs_iter, nerrors, have_mean in registers (uniform); Sigma / S is worked in place in the chain's Sigma
// square in HBM (the owner pieces' barriers are __syncthreads).  A chain whose status turns non-zero leaves its loop: uniform,
// one workgroup serves one chain, so every barrier sits in uniform control flow.  BatchArgs.active switches whole datasets off
// (MCMC_batch(stop_each = ...): the datasets that have converged): their workgroups return at once.
//
// Where the data sit (the same bits): LDS_DATA = true ("batch-lds") copies the dataset into LDS once, column-major as in HBM --
// lane l reads address l of a column, consecutive doubles, no bank conflict --; false ("batch-stream") reads it from global
// memory every step, 64 consecutive doubles of a column per wavefront.  batch_data_in_lds() picks.
#pragma once
#include "mh_fun.hpp"
#include "mh_user.hpp"

namespace {

struct BatchArgs {
  FunArgs F;                 // kernel, run, state, out (th1, f1, rsum, step, phase: unused)
  // the model: dataset 0 and the distance between datasets, in doubles
  int family, p, intercept, guard;
  long long n;
  double prior_div;
  const double* X;
  const double* y;
  const double* hs;          // logistic: [D][hs_stride] the data-only sums of every dataset
  long long x_stride, y_stride, hs_stride;
  long long chains_per_model;
  const int* active;         // [nmodels] or NULL: the chains of a dataset whose entry is 0 do not run (fmcmc_mcmc_run_batch_sel_dev)
};

// LDS doubles of the dataset copy: logistic reads X only (y is in hs), the Gaussian families X and y
__host__ __device__ inline size_t batch_data_doubles(int family, long long n, int p) {
  const size_t cols = (family == FMCMC_FAM_IID_NORMAL) ? 1 : (family == FMCMC_FAM_LOGISTIC) ? (size_t)p : (size_t)p + 1;
  return cols * (size_t)n;
}
// dynamic LDS doubles next to the data: the vectors of mh_fun_step<64> (with kernel_adapt's LDL^T factor) and, carried across
// the steps, kernel_adapt's running row sum and mean_prev
__host__ __device__ inline size_t batch_step_doubles(int k, int kf, int kind) { return fun_lds_doubles(k, kf, kind, 64) + 2 * (size_t)kf; }
constexpr size_t BATCH_STATIC_LDS = sizeof(double) * (FMCMC_MAX_K_WAVE + NW + 2);   // s_th, s_w, s_f of the kernel
constexpr size_t BATCH_LDS_BYTES = 160 * 1024;   // the LDS of a CU (mh_route.hpp assumes the same)
// The rule: the dataset goes into LDS when it fits into the CU's 160 KB next to the step's vectors, sized for the widest chain
// (k = FMCMC_MAX_K_WAVE) so that it is a function of (family, n, p, kf, kind) alone.  DESIGN 5.11 has the reason.
inline bool batch_data_in_lds(int family, long long n, int p, int kf, int kind) {
  if (n > (long long)(BATCH_LDS_BYTES / sizeof(double))) return false;
  return sizeof(double) * (batch_step_doubles(FMCMC_MAX_K_WAVE, kf, kind) + batch_data_doubles(family, n, p)) + BATCH_STATIC_LDS <= BATCH_LDS_BYTES;
}

#ifdef FMH_WITH_FUN_KERNEL   /* compiled into k_fun.hip only */
// (four waves per SIMD = two workgroups per CU: the loop waits on its barriers and on the owners' serial chains, a second
// workgroup fills the gaps -- 128 VGPRs with 312 B of scratch per lane against 221 VGPRs and one workgroup per CU: 9.7 against
// 14.5 us per step at tools/bench_batch.py's shape)
// MASKED = false (active == NULL) is the kernel without a word of the mask: the early exit below, small as it is, moves the
// register allocation of a kernel that spills 266 SGPRs, and the step loop then reloads more of them -- 9.60 against 9.51 us
// per step at that shape with the test compiled in and a NULL mask.
template <bool LDS_DATA, bool MASKED>
__global__ __launch_bounds__(NT, 4) void mh_sweep_batch(const BatchArgs B) {
  extern __shared__ double smem[];
  __shared__ double s_th[FMCMC_MAX_K_WAVE], s_w[NW], s_f[2];
  const FunArgs& A = B.F;
  const int r = threadIdx.x;
  const int k = A.k, kf = A.kf;
  const long long c = blockIdx.x;            // one chain per workgroup (grid = nchains)
  const long long d = c / B.chains_per_model, n = B.n;
  // a dataset that is switched off: its chains' state, rows and outputs stay as they are.  One workgroup serves one chain, so
  // the test is uniform, and it comes before the first LDS access and the first barrier.
  if constexpr (MASKED) {
    if (B.active[d] == 0) return;
  }
  double* s_mu = smem;
  double* s_scale = s_mu + k;
  double* s_lb = s_scale + k;
  double* s_ub = s_lb + k;
  double* th0 = s_ub + k;                    // [k]
  double* th1 = th0 + k;                     // [k]
  double* s_z = th1 + k;                     // [k + 1] variates of a step
  double* vv = s_z + (k + 1);                // [kf] the vectors of mh_fun_step, in its order
  double* vmp = vv + kf;
  double* vmt = vmp + kf;
  double* vd = vmt + kf;
  double* vk = vd + kf;
  double* vq = vk + kf;
  double* vt = vq + kf;
  double* fac = vt + kf;                     // kernel_adapt: [kf][kf | 1] the LDL^T factor
  int* s_flag = (int*)(fac + ((A.kind == FMCMC_KERNEL_ADAPT) ? kf * (kf | 1) : 0));   // (2 doubles)
  double* s_rsum = (double*)s_flag + 2;      // [kf] kernel_adapt: the running sum of this call's rows
  double* s_mean = s_rsum + kf;              // [kf] kernel_adapt: mean_prev
  double* s_dat = s_mean + kf;               // LDS_DATA: [p][n] X, then [n] y
  const FunLds L{s_mu, s_scale, s_lb, s_ub, th0, th1, s_z, vv, vmp, vmt, vd, vk, vq, vt, fac};
  const bool row = r < kf, par = r < k;
  const int wr = row ? A.which[r] : 0;      // the free parameter of matrix row r
  const bool adapt = A.kind == FMCMC_KERNEL_ADAPT, ram = A.kind == FMCMC_KERNEL_RAM, adaptive = adapt || ram;
  const bool logit = B.family == FMCMC_FAM_LOGISTIC;
  const int pp = (B.family == FMCMC_FAM_IID_NORMAL) ? 0 : B.p;
  const double* Xg = B.X + d * B.x_stride;
  const double* yg = B.y + d * B.y_stride;
  const double* hs = logit ? B.hs + d * B.hs_stride : nullptr;
  if (par) {
    s_mu[r] = A.mu[r]; s_scale[r] = A.scale[r]; s_lb[r] = A.lb[r]; s_ub[r] = A.ub[r];
    th0[r] = A.theta0[c * k + r];
    th1[r] = th0[r];                         // (row 1: theta1 = theta0)
  }
  if (adapt && row) s_mean[r] = A.mean_prev[c * kf + r];
  if constexpr (LDS_DATA) {
    const long long nx = (long long)pp * n;
    for (long long e = r; e < nx; e += NT) s_dat[e] = Xg[e];
    if (!logit)
      for (long long e = r; e < n; e += NT) s_dat[nx + e] = yg[e];
  }
  RoCarried ch = {FMCMC_CHAIN_OK, 0.0, 0};  // the chain's carried values (uniform: every thread keeps them)
  long long abs_iter = 0;
  int have_mean = 0, nerr = 0;
  double* const Mg = adaptive ? A.Sigma + c * (long long)kf * kf : nullptr;   // the chain's Sigma / S square
  auto bar = []() { __syncthreads(); };
  auto ma = [&](int a, int b) -> double& { return Mg[a * kf + b]; };
  if (adaptive && !A.fresh) {
    abs_iter = A.abs_iter[c];
    nerr = A.nerrors[c];
    if (adapt) have_mean = A.have_mean[c];
  }
  __syncthreads();

  // f(th) for the whole workgroup (th: LDS, visible to every thread); a barrier behind it
  auto eval = [&](const double* th) -> double {
    double f;
    if constexpr (LDS_DATA) {
      const double* xs = s_dat;
      const double* ys = s_dat + (long long)pp * n;
      f = logpost_canon_wg(B.family, B.p, B.intercept, B.guard, n, B.prior_div, hs, th,
                           [&](int j, long long i) { return xs[(long long)j * n + i]; }, [&](long long i) { return ys[i]; }, s_th, s_w);
    } else {
      f = logpost_canon_wg(B.family, B.p, B.intercept, B.guard, n, B.prior_div, hs, th,
                           [&](int j, long long i) { return Xg[(long long)j * n + i]; }, [&](long long i) { return yg[i]; }, s_th, s_w);
    }
    if (r == 0) s_f[0] = f;
    __syncthreads();
    return s_f[0];
  };

  // ================= row 1 (R/mcmc.R:728-735) =================
  ch.f0 = eval(th0);
  if (adaptive && A.fresh) ro_square_fresh(Mg, kf, A.eps, r, NT);
  ro_row1(A, c, r, NT, par, &th0[r], &th1[r], ch.f0);
  if (adapt && row) s_rsum[r] = th0[wr];
  __syncthreads();
  if (A.nsteps >= 2) fun_propose<true>(A, L, Mg, c, r, 2, ch, abs_iter, have_mean, &s_rsum[r], &s_mean[r]);

  for (long long i = 2; i <= A.nsteps && ch.status == FMCMC_CHAIN_OK; i++) {
    double f1 = eval(th1);
    // ---- kernel_ram: the adaptation with f(un-reflected theta1), then the reflection (R/kernel_ram.R:129-152); s_z still
    // holds the variates U of this step's proposal
    if (ram) {
      if (A.until > (double)abs_iter && abs_iter > A.warmup && (i % A.freq) == 0)
        if (ro_ram_adapt(row, r, kf, i, f1, ch.f0, A.ram_neg_exp, A.arate, A.constr, s_z, vq, vt, vd, vk, &s_flag[0], bar, ma)) nerr += 1;
      abs_iter += 1;
      if (A.ram_bounded) {
        if (row) th1[wr] = reflect1(th1[wr], s_lb[wr], s_ub[wr]);
        __syncthreads();
        f1 = eval(th1);
      }
    }
    // ---- accept / store of step i (R/mcmc.R:754-778)
    ro_accept_store(A, c, r, par, i, f1, f1 - ch.f0, ch, &th0[r], &th1[r], bar);
    if (ch.status != FMCMC_CHAIN_OK) break;
    if (adapt && row) s_rsum[r] = s_rsum[r] + th0[wr];
    // ---- proposal of step i + 1
    if (i < A.nsteps) fun_propose<true>(A, L, Mg, c, r, i + 1, ch, abs_iter, have_mean, &s_rsum[r], &s_mean[r]);
  }

  // ================= the end of the call: the Sigma square as the family path hands it on, the carried values =================
  if (adaptive) {
    __syncthreads();
    ro_square_hand_on(Mg, kf, adapt, r, NT);
  }
  ro_write_back(A, c, r, par, ch, &th0[r]);
  if (adapt && row) A.mean_prev[c * kf + r] = s_mean[r];
  if (r == 0 && adaptive) {
    A.abs_iter[c] = abs_iter;
    A.nerrors[c] = nerr;
    if (adapt) A.have_mean[c] = have_mean;
  }
}
#endif  // FMH_WITH_FUN_KERNEL

}  // namespace
