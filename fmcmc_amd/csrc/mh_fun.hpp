// mh_fun.hpp -- mh_fun_step<NTH>: the sweep for a log-posterior the CALLER evaluates (fmcmc_mcmc_run_fun_*, the batched
// fmcmc_logpost_fn of include/fmcmc_amd.h).  The family kernels fuse the evaluation into the step; here it is the caller's, so
// the step is cut at the evaluation: one launch moves every chain of the call from one evaluation to the next --
//   [START]   row 1: f0 = fun(initial), kernel state initialised, row stored
//   [RAM]     kernel_ram: the adaptation with f(un-reflected theta1) (R/kernel_ram.R:129-152), then the reflection
//   [ACCEPT]  step i: NaN checks, log u < f1 - f0, theta0 / f0, the kept row, draws, logpost, accept bit (R/mcmc.R:754-778)
//   [PROPOSE] step i + 1: the variates, the proposal and kernel_adapt's adaptation, theta1 -> the [C][k] buffer fun reads
//   [FINISH]  the last launch: the Sigma square handed on in the layout of the family path
// so that a plain step is one launch plus the caller's evaluation (bounded kernel_ram: two of each).
//
// Layout: one workgroup per chain, thread r = parameter r / matrix row r; NTH = 64 (k <= 64: one wavefront, "fun") or 256
// (k > 64: "fun-wg").  Every value carried from launch to launch lives in HBM, in the caller's fmcmc_state / fmcmc_out buffers
// (theta0, f0, abs_iter, Sigma, mean_prev, have_mean, nerrors, accept_count, status) and in the call's scratch (theta1, the
// running row sum of kernel_adapt, the free-parameter list); LDS holds one launch's vectors.  Sigma (kernel_adapt) / S
// (kernel_ram) are worked in place in the lower triangle of the chain's Sigma square; the kernel_adapt factor, rebuilt every
// step and never carried, is the LDL^T factor in LDS for k <= 64 (L strictly lower, the numerators W_ib at [b][i], as the
// owner waves of mh_sweep_kernel keep it) and the Cholesky factor transposed into the square's upper half for k > 64 (its
// diagonal in LDS, as mh_sweep_bigk<true>).  Hand-offs through global memory stay inside the workgroup and are ordered by
// __syncthreads().
//
// Bit contract: the same operations in the same order as the oracle (fmcmc_oracle.c: propose_normal, propose_adapt -- LDL^T for
// k <= 64, Cholesky beyond --, propose_ram, scan_sq_canon, ram_factor_update_canon, reflect1) and the family kernels.  The
// kernel_adapt / kernel_ram arithmetic, the variates, the fresh start and hand-on of the square and the accept / store half
// are the row owner's pieces of mh_rowowner.hpp (mh_sweep_bigk<true> keeps its own lines of the same arithmetic);
// mh_user_step shares the accept / store half.  Here stay: the cut of a step into phases, the simple kernels with their
// single-parameter schemes, and the LDL^T factor of k <= 64 -- the last two in fun_propose, the PROPOSE phase as a device
// function that mh_sweep_batch (mh_batch.hpp: the same step with a family's evaluation fused in, one launch) calls as well.
#pragma once
#include "mh_rowowner.hpp"

namespace {

struct FunArgs {
  // kernel
  int kind, k, kf, scheme, warmup, freq, scheme_len, ram_bounded;
  double until, eps, arate;
  double ram_df;             // Student-t degrees of freedom of kernel_ram's variates, 0 = N(0,1)
  double ram_neg_exp;        // eta(i, k) = min(1, k * exp(ram_neg_exp * log(i)))
  const double* mu;
  const double* scale;
  const double* lb;
  const double* ub;
  const int* scheme_seq;
  const double* constr;
  const int* which;          // [kf] the free parameters (scratch of the call)
  // run
  long long nchains, nsteps, burnin, thin, ldS, chain_base, step_base;
  unsigned long long seed;
  int rng_mode, kz, fresh;
  const double* fed_logu;
  const double* fed_z;
  // state
  double* theta0;
  double* f0;
  long long* abs_iter;
  double* Sigma;
  double* mean_prev;
  int* have_mean;
  int* nerrors;
  int* scheme_cols;
  double* rsum;              // [C][kf] kernel_adapt: the running sum of this call's rows (its first running mean)
  // out
  double* samples;
  double* logpost;
  double* draws;
  long long* accept_count;
  unsigned int* accept_bits;
  int* status;
  long long* status_step;
  double* status_theta;
  // the caller's evaluation: theta1 of every chain [C][k] in, f(theta1) [C] out
  double* th1;
  const double* f1;
  // this launch
  long long step;            // the loop step whose evaluation has just come back (1: row 1)
  int phase;                 // FPH_*
};

enum { FPH_START = 1, FPH_RAM = 2, FPH_ACCEPT = 4, FPH_PROPOSE = 8, FPH_FINISH = 16 };

// LDS doubles of one launch: parameters, theta0 / theta1, the variates, the vectors, and kernel_adapt's factor (k <= 64: the
// LDL^T square [kf][kf | 1]; k > 64: the Cholesky diagonal)
__host__ __device__ inline size_t fun_lds_doubles(int k, int kf, int kind, int nth) {
  const size_t fac = (kind == FMCMC_KERNEL_ADAPT) ? (nth <= 64 ? (size_t)kf * (size_t)(kf | 1) : (size_t)kf) : 0;
  return 4 * (size_t)k + 2 * (size_t)k + (size_t)(k + 1) + 7 * (size_t)kf + fac + 2;
}

#ifdef FMH_WITH_FUN_KERNEL   /* compiled into k_fun.hip only */
// the LDS vectors of a step (carved by the caller)
struct FunLds {
  double *mu, *scale, *lb, *ub;   // [k] the kernel's parameters
  double *th0, *th1, *z;          // [k], [k], [k + 1]
  double *vv, *vmp, *vmt, *vd, *vk, *vq, *vt;   // [kf] each
  double* fac;                    // kernel_adapt: [kf][kf | 1] the LDL^T factor (LDL) | [kf] the Cholesky diagonal
};

// The proposal of loop step ip >= 2 of local chain c into L.th1, with kernel_adapt's adaptation in front of it: the PROPOSE
// phase of mh_fun_step and the proposal of mh_sweep_batch's loop (mh_batch.hpp).  Every thread of the workgroup (thread r =
// row r) calls it; it ends with a barrier behind theta1.  LDL: kernel_adapt factors Sigma as L D L^T in LDS (k <= 64),
// else by the row owner's Cholesky in the square's upper half.  Mg: the chain's Sigma / S square.  rsum_r, mean_r: this row's
// element of kernel_adapt's running row sum and of mean_prev, wherever the caller carries them.  A chain whose Sigma is not
// positive definite gets its status here (theta1: the previous proposal, as in the oracle).
template <bool LDL>
__device__ __forceinline__ void fun_propose(const FunArgs& A, const FunLds& L, double* Mg, long long c, int r, long long ip,
                                            RoCarried& ch, long long& abs_iter, int& have_mean, const double* rsum_r, double* mean_r) {
  const int k = A.k, kf = A.kf, kz = A.kz, LD = kf | 1;
  double *s_mu = L.mu, *s_scale = L.scale, *s_lb = L.lb, *s_ub = L.ub, *th0 = L.th0, *th1 = L.th1, *s_z = L.z;
  double *vv = L.vv, *vmp = L.vmp, *vmt = L.vmt, *vd = L.vd, *vq = L.vq, *fac = L.fac;
  const bool row = r < kf, par = r < k;
  const int wr = row ? A.which[r] : 0;
  const bool adapt = A.kind == FMCMC_KERNEL_ADAPT, simple = !adapt && A.kind != FMCMC_KERNEL_RAM;
  const bool unif = A.kind == FMCMC_KERNEL_UNIF || A.kind == FMCMC_KERNEL_UNIF_REFLECTIVE;
  auto bar = []() { __syncthreads(); };
  auto ma = [&](int a, int b) -> double& { return Mg[a * kf + b]; };
  auto mbl = [&](int a, int b) -> double& { return Mg[b * kf + a]; };
  auto mbd = [&](int j) -> double& { return fac[j]; };
  if (r < kz) s_z[r] = ro_variate(A, c, ip, r, unif);
  __syncthreads();
  if (simple) {   // kernel_normal(_reflective), kernel_unif(_reflective) (R/kernel_normal.R:65-72, :146-164; R/kernel_unif.R)
    if (par) th1[r] = th0[r];
    __syncthreads();
    // plan_update_sequence (R/kernel.R:66-133): every scheme but "joint" updates ONE parameter per step
    const bool single = A.scheme != FMCMC_SCHEME_JOINT;
    int col = 0;
    if (A.scheme == FMCMC_SCHEME_ORDERED) {
      col = A.which[(int)((ip - 1) % kf)];
    } else if (A.scheme == FMCMC_SCHEME_EXPLICIT) {
      col = A.scheme_seq[(int)((ip - 1) % A.scheme_len)];
    } else if (A.scheme == FMCMC_SCHEME_RANDOM) {
      if (A.rng_mode == FMCMC_RNG_FED) {
        col = A.scheme_cols[c * A.nsteps + (ip - 1)];
      } else {
        // sample(which(!fixed), nsteps, TRUE)[i]; a single free parameter at position j makes R sample from 1:j
        const unsigned int npool = (kf == 1) ? (unsigned int)(A.which[0] + 1) : (unsigned int)kf;
        const unsigned int idx = fmh_scheme_index(A.seed, (unsigned int)ip, (unsigned int)(A.chain_base + c), npool);
        col = (kf == 1) ? (int)idx : A.which[idx];
        if (A.scheme_cols && r == 0) A.scheme_cols[c * A.nsteps + (ip - 1)] = col;
      }
    }
    const int nupd = single ? 1 : kf;
    if (r < nupd) {
      const int j = single ? col : wr;
      double t = th0[j] + (s_mu[j] + s_scale[j] * s_z[r]);
      if (A.kind == FMCMC_KERNEL_NORMAL_REFLECTIVE || A.kind == FMCMC_KERNEL_UNIF_REFLECTIVE) t = reflect1(t, s_lb[j], s_ub[j]);
      th1[j] = t;
    }
  } else if (adapt) {   // R/kernel_adapt.R:117-180, bw = 0, freq = 1
    if (A.until > (double)abs_iter && abs_iter > A.warmup && ip > 2) {
      const double x = row ? th0[wr] : 0.0;
      const double mp = !row ? 0.0 : have_mean ? *mean_r : (*rsum_r / (double)(ip - 1));
      const double mt = ro_sigma_update(row, r, (double)(abs_iter - 1), A.eps, x, mp, vv, vmp, vmt, bar, ma);
      if (row) *mean_r = mt;
      have_mean = 1;
    }
    abs_iter += 1;
    bool notpd = false;
    if constexpr (LDL) {
      // root-free factor Sigma = L D L^T, left-looking, thread = row (ldl_lower_canon): L strictly lower in fac, W_ib at [b][i], D in vd
      for (int j = 0; j < kf; j++) {
        double s = 0.0;
        if (row && r >= j) {
          s = Mg[r * kf + j];
          for (int b = 0; b < j; b++) s = fmh_fma(-fac[r * LD + b], fac[b * LD + j], s);
          if (r == j) vq[0] = s;
        }
        __syncthreads();
        const double d = vq[0];
        if (!(d > 0.0) || !fmh_isfinite(d)) { notpd = true; break; }   // (uniform)
        if (r == j) { fac[j * LD + j] = 1.0; vd[j] = d; }
        else if (row && r > j) { fac[r * LD + j] = s / d; fac[j * LD + r] = s; }
        __syncthreads();
      }
      if (!notpd) {
        if (par) th1[r] = th0[r];
        if (row) vq[r] = fmh_sqrt(vd[r]) * s_z[r];    // u = sqrt(D) z
        __syncthreads();
        if (row) {
          double s = 0.0;
          for (int b = 0; b <= r; b++) s = fmh_fma(fac[r * LD + b], vq[b], s);   // (L_rr = 1)
          th1[wr] = reflect1(th0[wr] + (s_mu[wr] + s), s_lb[wr], s_ub[wr]);
        }
      }
    } else {
      // the Cholesky factor (chol_lower_canon): L_rb (r > b) at [b][r] of the square, the diagonal in fac
      notpd = ro_cholesky(row, r, kf, &vq[0], bar, ma, mbl, mbd);
      if (!notpd) ro_adapt_propose(row, par, r, wr, th0, th1, s_z, s_mu, s_lb, s_ub, bar, mbl, mbd);
    }
    if (notpd) {   // (theta1: the previous proposal, as in the oracle)
      ch.status = FMCMC_CHAIN_NOT_PD;
      ro_fail(A, c, r, par, ch.status, ip, &th1[r]);
    }
  } else {   // kernel_ram, R/kernel_ram.R:123-126
    if (row) th1[wr] = th0[wr] + ro_ram_propose(r, s_z, ma);
  }
  __syncthreads();
}

template <int NTH>
__global__ __launch_bounds__(NTH) void mh_fun_step(const FunArgs A) {
  extern __shared__ double smem[];
  const int r = threadIdx.x;
  const int k = A.k, kf = A.kf, ph = A.phase;
  const long long c = blockIdx.x;            // one chain per workgroup (grid = nchains)
  const long long i = A.step;
  double* s_mu = smem;
  double* s_scale = s_mu + k;
  double* s_lb = s_scale + k;
  double* s_ub = s_lb + k;
  double* th0 = s_ub + k;                    // [k]
  double* th1 = th0 + k;                     // [k]
  double* s_z = th1 + k;                     // [k + 1] variates of a step
  double* vv = s_z + (k + 1);                // [kf] kernel_adapt: x
  double* vmp = vv + kf;                     // [kf] mean_prev
  double* vmt = vmp + kf;                    // [kf] mean_t
  double* vd = vmt + kf;                     // [kf] ram: d_j | adapt: the pivots D (k <= 64); [0] the pivot of a column
  double* vk = vd + kf;                      // [kf] ram: kappa_j
  double* vq = vk + kf;                      // [kf] scan buffer A | adapt: u = sqrt(D) z
  double* vt = vq + kf;                      // [kf] scan buffer B
  double* fac = vt + kf;                     // kernel_adapt: [kf][LD] the LDL^T factor (k <= 64) | [kf] the Cholesky diagonal
  int* s_flag = (int*)(fac + ((A.kind == FMCMC_KERNEL_ADAPT) ? (NTH <= 64 ? kf * (kf | 1) : kf) : 0));
  const bool row = r < kf, par = r < k;
  const int wr = row ? A.which[r] : 0;      // the free parameter of matrix row r
  const bool adapt = A.kind == FMCMC_KERNEL_ADAPT, ram = A.kind == FMCMC_KERNEL_RAM, adaptive = adapt || ram;
  if (par) {
    s_mu[r] = A.mu[r]; s_scale[r] = A.scale[r]; s_lb[r] = A.lb[r]; s_ub[r] = A.ub[r];
    th0[r] = A.theta0[c * k + r];
    th1[r] = A.th1[c * k + r];
  }
  const bool start = (ph & FPH_START) != 0;
  const bool unif = A.kind == FMCMC_KERNEL_UNIF || A.kind == FMCMC_KERNEL_UNIF_REFLECTIVE;   // (the kind is not normalised here)
  RoCarried ch = ro_carried(A, c, start);   // the chain's carried values (uniform: every thread keeps them)
  long long abs_iter = 0;
  int have_mean = 0, nerr = 0;
  double* const Mg = adaptive ? A.Sigma + c * (long long)kf * kf : nullptr;   // the chain's Sigma / S square
  // its elements: Sigma / S (i >= j), the Cholesky factor's strictly lower part transposed into the upper half, its diagonal
  auto bar = []() { __syncthreads(); };
  auto ma = [&](int a, int b) -> double& { return Mg[a * kf + b]; };
  if (adaptive && !(start && A.fresh)) {
    abs_iter = A.abs_iter[c];
    nerr = A.nerrors[c];
    if (adapt) have_mean = A.have_mean[c];
  }
  __syncthreads();

  // ================= row 1 (R/mcmc.R:728-735) =================
  if (start) {
    if (adaptive && A.fresh) ro_square_fresh(Mg, kf, A.eps, r, NTH);
    ro_row1(A, c, r, NTH, par, &th0[r], &th1[r], ch.f0);
    if (adapt && row) A.rsum[c * kf + r] = th0[wr];
    __syncthreads();
  }

  // ================= kernel_ram: the adaptation with f(un-reflected theta1), then the reflection =================
  if ((ph & FPH_RAM) && ram && ch.status == FMCMC_CHAIN_OK) {
    if (A.until > (double)abs_iter && abs_iter > A.warmup && (i % A.freq) == 0) {
      if (row) s_z[r] = ro_variate(A, c, i, r, unif);   // (the variates U of this step's proposal, drawn again)
      if (ro_ram_adapt(row, r, kf, i, A.f1[c], ch.f0, A.ram_neg_exp, A.arate, A.constr, s_z, vq, vt, vd, vk, &s_flag[0], bar, ma)) nerr += 1;
    }
    abs_iter += 1;
    if (A.ram_bounded) {
      if (row) th1[wr] = reflect1(th1[wr], s_lb[wr], s_ub[wr]);
      __syncthreads();
      if (!(ph & FPH_ACCEPT) && par) A.th1[c * k + r] = th1[r];   // (the reflected proposal goes to the second evaluation)
    }
  }

  // ================= accept / store of step i (R/mcmc.R:754-778) =================
  if ((ph & FPH_ACCEPT) && ch.status == FMCMC_CHAIN_OK) {
    ro_accept_store(A, c, r, par, i, A.f1[c], A.f1[c] - ch.f0, ch, &th0[r], &th1[r], bar);
    if (ch.status == FMCMC_CHAIN_OK && adapt && row) A.rsum[c * kf + r] = A.rsum[c * kf + r] + th0[wr];
  }

  // ================= proposal of step ip = i + 1 =================
  const long long ip = i + 1;
  if ((ph & FPH_PROPOSE) && ch.status == FMCMC_CHAIN_OK && ip <= A.nsteps) {
    const FunLds L{s_mu, s_scale, s_lb, s_ub, th0, th1, s_z, vv, vmp, vmt, vd, vk, vq, vt, fac};
    fun_propose<(NTH <= 64)>(A, L, Mg, c, r, ip, ch, abs_iter, have_mean, adapt ? &A.rsum[c * kf + r] : nullptr,
                             adapt ? &A.mean_prev[c * kf + r] : nullptr);
    if (par && ch.status == FMCMC_CHAIN_OK) A.th1[c * k + r] = th1[r];
  }

  // ================= the last launch: the Sigma square as the family path hands it on =================
  if ((ph & FPH_FINISH) && adaptive) {
    __syncthreads();
    ro_square_hand_on(Mg, kf, adapt, r, NTH);
  }

  // ---- carried values back to HBM
  ro_write_back(A, c, r, par, ch, &th0[r]);
  if (r == 0 && adaptive) {
    A.abs_iter[c] = abs_iter;
    A.nerrors[c] = nerr;
    if (adapt) A.have_mean[c] = have_mean;
  }
}
#endif  // FMH_WITH_FUN_KERNEL

}  // namespace
