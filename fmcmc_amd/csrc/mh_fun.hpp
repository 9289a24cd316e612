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
// k <= 64, Cholesky beyond --, propose_ram, scan_sq_canon, ram_factor_update_canon, reflect1) and the family kernels.
#pragma once

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
// variate `a` of loop step i of local chain c; a == kz: the log accept uniform (the canonical stream, or the fed one)
__device__ __forceinline__ double fun_variate(const FunArgs& A, long long c, long long i, int a) {
  const unsigned int st = (unsigned int)(A.step_base + i), cg = (unsigned int)(A.chain_base + c);
  const bool fed = A.rng_mode == FMCMC_RNG_FED;
  if (a == A.kz) return fed ? A.fed_logu[c * A.nsteps + (i - 1)] : fmh_log_accept_u(A.seed, st, cg);
  if (fed) return A.fed_z[(c * A.nsteps + (i - 1)) * A.kz + a];
  if (A.kind == FMCMC_KERNEL_RAM && A.ram_df > 0.0) return fmh_student_t(A.seed, st, cg, (unsigned int)a, A.ram_df);
  if (A.kind == FMCMC_KERNEL_UNIF || A.kind == FMCMC_KERNEL_UNIF_REFLECTIVE) return fmh_unif(A.seed, st, cg, (unsigned int)a);
  return fmh_normal(A.seed, st, cg, (unsigned int)a);
}

template <int NTH>
__global__ __launch_bounds__(NTH) void mh_fun_step(const FunArgs A) {
  extern __shared__ double smem[];
  const int r = threadIdx.x;
  const int k = A.k, kf = A.kf, kz = A.kz, ph = A.phase;
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
  const int LD = kf | 1;
  const bool row = r < kf, par = r < k;
  const int wr = row ? A.which[r] : 0;      // the free parameter of matrix row r
  const bool adapt = A.kind == FMCMC_KERNEL_ADAPT, ram = A.kind == FMCMC_KERNEL_RAM, adaptive = adapt || ram;
  const bool simple = !adaptive;
  if (par) {
    s_mu[r] = A.mu[r]; s_scale[r] = A.scale[r]; s_lb[r] = A.lb[r]; s_ub[r] = A.ub[r];
    th0[r] = A.theta0[c * k + r];
    th1[r] = A.th1[c * k + r];
  }
  const bool start = (ph & FPH_START) != 0;
  // ---- the chain's carried values (uniform: every thread keeps them)
  int status = start ? FMCMC_CHAIN_OK : A.status[c];
  double f0 = start ? A.f1[c] : A.f0[c];
  long long nacc = start ? 0 : A.accept_count[c];
  long long abs_iter = 0;
  int have_mean = 0, nerr = 0;
  double* const Mg = adaptive ? A.Sigma + c * (long long)kf * kf : nullptr;   // the chain's Sigma / S square
  if (adaptive && !(start && A.fresh)) {
    abs_iter = A.abs_iter[c];
    nerr = A.nerrors[c];
    if (adapt) have_mean = A.have_mean[c];
  }
  const long long nwords = (A.nsteps + 31) >> 5;
  auto store_row = [&](long long ir, double lpv) {   // row ir of ans: kept when ir > burnin and (ir - burnin) mod thin == 0
    if (ir > A.burnin && (ir - A.burnin) % A.thin == 0) {
      const long long s = (ir - A.burnin) / A.thin - 1;
      if (par) {
        A.samples[(c * k + r) * A.ldS + s] = th0[r];
        if (A.draws) A.draws[(c * k + r) * A.ldS + s] = th1[r];
      }
      if (A.logpost && r == 0) A.logpost[c * A.ldS + s] = lpv;
    }
  };
  auto fail = [&](long long ir) {
    if (r == 0) { A.status[c] = status; A.status_step[c] = ir; }
    if (par) A.status_theta[c * k + r] = th1[r];
  };
  __syncthreads();

  // ================= row 1 (R/mcmc.R:728-735) =================
  if (start) {
    if (adaptive && A.fresh)
      for (int e = r; e < kf * kf; e += NTH) {
        const int a = e / kf, b = e - a * kf;
        if (b <= a) Mg[e] = (a == b) ? 1.0 * A.eps : 0.0;
      }
    if (A.accept_bits)
      for (long long w = r; w < nwords; w += NTH) A.accept_bits[c * nwords + w] = 0u;
    if (r == 0) { A.status[c] = FMCMC_CHAIN_OK; A.status_step[c] = 0; }
    store_row(1, f0);
    if (adapt && row) A.rsum[c * kf + r] = th0[wr];
    __syncthreads();
  }

  // ================= kernel_ram: the adaptation with f(un-reflected theta1), then the reflection =================
  if ((ph & FPH_RAM) && ram && status == FMCMC_CHAIN_OK) {
    if (A.until > (double)abs_iter && abs_iter > A.warmup && (i % A.freq) == 0) {
      const double f1u = A.f1[c];
      double a_n = fmh_exp(f1u - f0);
      if (fmh_isnan(a_n)) a_n = 0.0;
      else if (a_n > 1.0) a_n = 1.0;
      double eta = (double)kf * fmh_exp(A.ram_neg_exp * fmh_log((double)i));
      if (eta > 1.0) eta = 1.0;
      if (row) s_z[r] = fun_variate(A, c, i, r);   // (the variates U of this step's proposal, drawn again)
      if (r == 0) s_flag[0] = 0;
      __syncthreads();
      // prefix sums of z^2: Hillis-Steele over the index, offsets 1, 2, 4, ... (scan_sq_canon)
      double* qa = vq;
      double* qb = vt;
      if (row) qa[r] = s_z[r] * s_z[r];
      __syncthreads();
      for (int s = 1; s < kf; s <<= 1) {
        if (row) qb[r] = (r >= s) ? qa[r] + qa[r - s] : qa[r];
        __syncthreads();
        double* tmp = qa; qa = qb; qb = tmp;
      }
      const double cp = (eta * (a_n - A.arate)) / qa[kf - 1];
      if (cp != 0.0 && fmh_isfinite(cp)) {
        if (row) {
          double dl = 0.0, kl = 0.0;
          const double Pj1 = qa[r], Pj = (r == 0) ? 0.0 : qa[r - 1];
          if (!ram_coef(cp, Pj, Pj1, s_z[r], dl, kl)) s_flag[0] = 1;
          vd[r] = dl; vk[r] = kl;
        }
        __syncthreads();
        if (s_flag[0] != 0) {
          nerr += 1;
        } else if (row) {   // S'_rj = S_rj d_j + G_rj kappa_j, G formed from the diagonal down (ram_factor_update_canon)
          double G = 0.0;
          for (int j = r; j >= 0; j--) {
            const double sij = Mg[r * kf + j];
            Mg[r * kf + j] = fmh_fma(G, vk[j], sij * vd[j]);
            G = fmh_fma(sij, s_z[j], G);
          }
        }
      }
      if (A.constr && row)   // Sigma <<- constr[which., which.] * Sigma (R/kernel_ram.R:149-150)
        for (int b = 0; b <= r; b++) Mg[r * kf + b] = A.constr[r * kf + b] * Mg[r * kf + b];
      __syncthreads();
    }
    abs_iter += 1;
    if (A.ram_bounded) {
      if (row) th1[wr] = reflect1(th1[wr], s_lb[wr], s_ub[wr]);
      __syncthreads();
      if (!(ph & FPH_ACCEPT) && par) A.th1[c * k + r] = th1[r];   // (the reflected proposal goes to the second evaluation)
    }
  }

  // ================= accept / store of step i (R/mcmc.R:754-778) =================
  if ((ph & FPH_ACCEPT) && status == FMCMC_CHAIN_OK) {
    const double f1 = A.f1[c];
    if (fmh_isnan(f1)) status = FMCMC_CHAIN_NAN_LOGPOST;
    const double ratio = f1 - f0;
    if (status == FMCMC_CHAIN_OK && fmh_isnan(ratio)) status = FMCMC_CHAIN_NAN_RATIO;
    if (status != FMCMC_CHAIN_OK) {
      fail(i);
    } else {
      const double lu = fun_variate(A, c, i, kz);
      if (lu < ratio) {
        if (par) th0[r] = th1[r];
        f0 = f1;
        nacc += 1;
        if (A.accept_bits && r == 0) A.accept_bits[c * nwords + ((i - 1) >> 5)] |= (1u << ((i - 1) & 31));
      }
      __syncthreads();
      store_row(i, f1);
      if (adapt && row) A.rsum[c * kf + r] = A.rsum[c * kf + r] + th0[wr];
    }
  }

  // ================= proposal of step ip = i + 1 =================
  const long long ip = i + 1;
  if ((ph & FPH_PROPOSE) && status == FMCMC_CHAIN_OK && ip <= A.nsteps) {
    if (r < kz) s_z[r] = fun_variate(A, c, ip, r);
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
        const double t = (double)(abs_iter - 1);
        double x = 0.0, mp = 0.0, mt = 0.0;
        if (row) {
          x = th0[wr];
          mp = have_mean ? A.mean_prev[c * kf + r] : (A.rsum[c * kf + r] / (double)(ip - 1));
          mt = (mp * t + x) / (t + 1);
          vv[r] = x; vmp[r] = mp; vmt[r] = mt;
        }
        __syncthreads();
        if (row) {
          const double c1 = (t - 1) / t, c2 = 1.0 / t;
          for (int b = 0; b <= r; b++) {      // (the lower triangle; element (r, b) has the bits of (b, r))
            const double ik = (b == r) ? 1.0 * A.eps : 0.0;
            const double inner = t * (mp * vmp[b]) - (t + 1) * (mt * vmt[b]) + x * vv[b] + 1e-5 * ik;
            Mg[r * kf + b] = c1 * Mg[r * kf + b] + c2 * inner;
          }
          A.mean_prev[c * kf + r] = mt;
        }
        have_mean = 1;
        __syncthreads();
      }
      abs_iter += 1;
      bool notpd = false;
      if constexpr (NTH <= 64) {
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
        // left-looking Cholesky, thread = row (chol_lower_canon): L_rb (r > b) at [b][r] of the square, the diagonal in fac
        for (int j = 0; j < kf; j++) {
          double s = 0.0;
          if (row && r >= j) {
            s = Mg[r * kf + j];
            for (int b = 0; b < j; b++) s = fmh_fma(-Mg[b * kf + r], Mg[b * kf + j], s);
            if (r == j) vq[0] = s;
          }
          __syncthreads();
          const double d = vq[0];
          if (!(d > 0.0) || !fmh_isfinite(d)) { notpd = true; break; }   // (uniform)
          const double ljj = fmh_sqrt(d);
          if (r == j) fac[j] = ljj;
          else if (row && r > j) Mg[j * kf + r] = s / ljj;
          __syncthreads();
        }
        if (!notpd) {
          if (par) th1[r] = th0[r];
          __syncthreads();
          if (row) {
            double s = 0.0;
            for (int b = 0; b < r; b++) s = fmh_fma(Mg[b * kf + r], s_z[b], s);
            s = fmh_fma(fac[r], s_z[r], s);
            th1[wr] = reflect1(th0[wr] + (s_mu[wr] + s), s_lb[wr], s_ub[wr]);
          }
        }
      }
      if (notpd) { status = FMCMC_CHAIN_NOT_PD; fail(ip); }   // (theta1: the previous proposal, as in the oracle)
    } else {   // kernel_ram, R/kernel_ram.R:123-126: (S U)_r from the diagonal down to column 0
      if (row) {
        double s = 0.0;
        for (int b = r; b >= 0; b--) s = fmh_fma(Mg[r * kf + b], s_z[b], s);
        th1[wr] = th0[wr] + s;
      }
    }
    __syncthreads();
    if (par && status == FMCMC_CHAIN_OK) A.th1[c * k + r] = th1[r];
  }

  // ================= the last launch: the Sigma square as the family path hands it on =================
  if ((ph & FPH_FINISH) && adaptive) {
    __syncthreads();
    for (int e = r; e < kf * kf; e += NTH) {   // kernel_adapt: the symmetric Sigma; kernel_ram: the lower factor, +0 above
      const int a = e / kf, b = e - a * kf;
      if (b > a) Mg[e] = adapt ? Mg[b * kf + a] : 0.0;
    }
  }

  // ---- carried values back to HBM
  if (par) A.theta0[c * k + r] = th0[r];
  if (r == 0) {
    A.f0[c] = f0;
    A.accept_count[c] = nacc;
    if (adaptive) {
      A.abs_iter[c] = abs_iter;
      A.nerrors[c] = nerr;
      if (adapt) A.have_mean[c] = have_mean;
    }
  }
}
#endif  // FMH_WITH_FUN_KERNEL

}  // namespace
