// mh_rowowner.hpp -- the arithmetic of a ROW OWNER: a kernel that gives a chain one workgroup and makes thread r row r of the
// chain's matrices.  Callers: mh_fun_step<NTH> (mh_fun.hpp: every piece), mh_sweep_batch (mh_batch.hpp: every piece, the step
// loop in one launch) and mh_user_step<NTH> (mh_user.hpp: the accept / store half).  mh_sweep_bigk<HBM> (mh_bigk.hpp) still carries its own lines of the same arithmetic: its latency-bound loops change
// their time by 1-6 % with any edit around them (profiles/bench_rowowner_placement.json), so it joins only with a shape measured
// neutral.  Every operation and its order is pinned to the oracle (fmcmc_oracle.c: propose_adapt, chol_lower_canon,
// scan_sq_canon, ram_factor_update_canon, propose_ram, reflect1; the accept rule of R/mcmc.R:754-778).
//
// The pieces do not know where a matrix lives.  They take
//   bar()       the workgroup barrier of the caller: lds_barrier (LDS ordering only) where the matrices are in LDS,
//               __syncthreads (global memory too) where they are in the chain's Sigma square in HBM
//   ma(i, j)    element (i, j), j <= i, of Sigma (kernel_adapt) / of the factor S (kernel_ram), as an lvalue
//   mbl(i, j)   element (i, j), j < i, of kernel_adapt's Cholesky factor
//   mbd(j)      its diagonal
// and the O(k) vectors as LDS pointers.  `row` = r < kf (the thread owns a matrix row), `par` = r < k (it owns a parameter).
// Every thread of the workgroup calls a piece that has a barrier in it; what a piece returns is uniform over the workgroup.
// The barriers of a piece are mh_sweep_bigk's.
//
// Outside: the k <= 64 LDL^T factor of mh_fun_step<64> and the wave owners of mh_streamed.hpp / mh_spec.hpp (the same
// arithmetic through lane shuffles, mh_owner.hpp), the single-parameter schemes of the callback step, logpost_eval_kernel,
// and mh_sweep_bigk.
#pragma once

namespace {

// ---- the variates of a step (the canonical Philox stream, or the fed one)
// the log accept uniform of loop step i of local chain c
template <class Args>
__device__ __forceinline__ double ro_log_u(const Args& A, long long c, long long i) {
  return (A.rng_mode == FMCMC_RNG_FED) ? A.fed_logu[c * A.nsteps + (i - 1)]
                                       : fmh_log_accept_u(A.seed, (unsigned int)(A.step_base + i), (unsigned int)(A.chain_base + c));
}
// variate `a` of loop step i of local chain c; a == kz: the log accept uniform.  `unif`: the kernel draws U(0,1) variates
template <class Args>
__device__ __forceinline__ double ro_variate(const Args& A, long long c, long long i, int a, bool unif) {
  if (a == A.kz) return ro_log_u(A, c, i);
  const unsigned int st = (unsigned int)(A.step_base + i), cg = (unsigned int)(A.chain_base + c);
  if (A.rng_mode == FMCMC_RNG_FED) return A.fed_z[(c * A.nsteps + (i - 1)) * A.kz + a];
  if (A.kind == FMCMC_KERNEL_RAM && A.ram_df > 0.0) return fmh_student_t(A.seed, st, cg, (unsigned int)a, A.ram_df);
  if (unif) return fmh_unif(A.seed, st, cg, (unsigned int)a);
  return fmh_normal(A.seed, st, cg, (unsigned int)a);
}

// ---- the chain's Sigma square [kf][kf] in HBM, worked in place in its lower triangle
// a fresh state: Sigma = S = eps I (the lower triangle; the upper half is the caller's to use)
__device__ __forceinline__ void ro_square_fresh(double* Mg, int kf, double eps, int tid, int nth) {
  for (int e = tid; e < kf * kf; e += nth) {
    const int i = e / kf, j = e - i * kf;
    if (j <= i) Mg[e] = (i == j) ? 1.0 * eps : 0.0;
  }
}
// the end of a call: kernel_adapt hands on the full symmetric Sigma, kernel_ram its lower factor (+0 above the diagonal).  The
// lower triangle is in place; the caller's last barrier ordered its stores.
__device__ __forceinline__ void ro_square_hand_on(double* Mg, int kf, bool adapt, int tid, int nth) {
  for (int e = tid; e < kf * kf; e += nth) {
    const int a = e / kf, b = e - a * kf;
    if (b > a) Mg[e] = adapt ? Mg[b * kf + a] : 0.0;
  }
}

// ---- kernel_adapt (R/kernel_adapt.R:117-180, bw = 0, freq = 1)
// The recursive update of Sigma with the row x of the chain, t = abs_iter - 1.  x, mp: this row's element of x and of mean_prev.
// Returns this row's element of mean_t, which the caller stores where it keeps mean_prev (after the piece: vmp is read by
// every row until its last barrier).
template <class Bar, class MA>
__device__ __forceinline__ double ro_sigma_update(bool row, int r, double t, double eps, double x, double mp, double* vv, double* vmp,
                                                  double* vmt, Bar bar, MA ma) {
  const double mt = (mp * t + x) / (t + 1);
  if (row) { vv[r] = x; vmp[r] = mp; vmt[r] = mt; }
  bar();
  if (row) {
    const double c1 = (t - 1) / t, c2 = 1.0 / t;
    for (int b = 0; b <= r; b++) {      // (the element (r, b) of the symmetric update: the same bits as (b, r))
      const double ik = (b == r) ? 1.0 * eps : 0.0;
      const double inner = t * (mp * vmp[b]) - (t + 1) * (mt * vmt[b]) + x * vv[b] + 1e-5 * ik;
      ma(r, b) = c1 * ma(r, b) + c2 * inner;
    }
  }
  bar();
  return mt;
}

// Left-looking Cholesky of Sigma, thread = row (twin of the oracle's chol_lower_canon); a column costs two barriers.
// pivot: one LDS double.  Returns "not positive definite"; the early exit is uniform (every thread reads the one pivot).
template <class Bar, class MA, class MBL, class MBD>
__device__ __forceinline__ bool ro_cholesky(bool row, int r, int kf, double* pivot, Bar bar, MA ma, MBL mbl, MBD mbd) {
  bool notpd = false;
  for (int j = 0; j < kf; j++) {
    double s = 0.0;
    if (row && r >= j) {
      s = ma(r, j);
      for (int b = 0; b < j; b++) s = fmh_fma(-mbl(r, b), mbl(j, b), s);
      if (r == j) *pivot = s;
    }
    bar();
    const double d = *pivot;
    if (!(d > 0.0) || !fmh_isfinite(d)) { notpd = true; break; }   // (uniform)
    const double ljj = fmh_sqrt(d);
    if (row) {
      if (r == j) mbd(j) = ljj;
      else if (r > j) mbl(r, j) = s / ljj;
    }
    bar();
  }
  return notpd;
}

// The proposal through the factor: theta1 = reflect(theta0 + (mu + L z)), row r of L z as one fma chain b < r, then the diagonal.
// j: the free parameter of row r.
template <class Bar, class MBL, class MBD>
__device__ __forceinline__ void ro_adapt_propose(bool row, bool par, int r, int j, const double* th0, double* th1, const double* z,
                                                 const double* mu, const double* lb, const double* ub, Bar bar, MBL mbl, MBD mbd) {
  if (par) th1[r] = th0[r];
  bar();
  if (row) {
    double s = 0.0;
    for (int b = 0; b < r; b++) s = fmh_fma(mbl(r, b), z[b], s);
    s = fmh_fma(mbd(r), z[r], s);
    th1[j] = reflect1(th0[j] + (mu[j] + s), lb[j], ub[j]);
  }
}

// ---- kernel_ram (R/kernel_ram.R:123-152)
// row r of S U, from the diagonal down to column 0 (propose_ram): theta1 = theta0 + it in the free coordinates
template <class MA>
__device__ __forceinline__ double ro_ram_propose(int r, const double* z, MA ma) {
  double s = 0.0;
  for (int b = r; b >= 0; b--) s = fmh_fma(ma(r, b), z[b], s);
  return s;
}

// The adaptation of loop step i with f1u = f(un-reflected theta1): a_n and eta, the prefix sums of z^2, the coefficients of the
// product-form update, the update of S in place, constr.  z: the variates of the step's proposal ([r] may be this thread's own
// store just before: the first barrier of the scan is in front of every read of another row's).  vq, vt: the two scan buffers;
// vd, vk: d_j, kappa_j; flag: one LDS int.  Returns whether the update failed and the caller counts an error.
template <class Bar, class MA>
__device__ __forceinline__ bool ro_ram_adapt(bool row, int r, int kf, long long i, double f1u, double f0, double neg_exp, double arate,
                                             const double* constr, const double* z, double* vq, double* vt, double* vd, double* vk,
                                             int* flag, Bar bar, MA ma) {
  double a_n = fmh_exp(f1u - f0);
  if (fmh_isnan(a_n)) a_n = 0.0;
  else if (a_n > 1.0) a_n = 1.0;
  double eta = (double)kf * fmh_exp(neg_exp * fmh_log((double)i));
  if (eta > 1.0) eta = 1.0;
  // prefix sums of z^2: Hillis-Steele over the index, offsets 1, 2, 4, ... (the oracle's scan_sq_canon; the order a
  // wavefront's lane scan has for k <= 64)
  double* qa = vq;
  double* qb = vt;
  if (row) qa[r] = z[r] * z[r];
  bar();
  for (int s = 1; s < kf; s <<= 1) {
    if (row) qb[r] = (r >= s) ? qa[r] + qa[r - s] : qa[r];
    bar();
    double* tmp = qa; qa = qb; qb = tmp;
  }
  const double nrm2 = qa[kf - 1];
  const double cp = (eta * (a_n - arate)) / nrm2;
  if (r == 0) *flag = 0;
  bar();
  bool failed = false;
  if (cp != 0.0 && fmh_isfinite(cp)) {
    double dl = 0.0, kl = 0.0;
    if (row) {
      const double Pj1 = qa[r], Pj = (r == 0) ? 0.0 : qa[r - 1];
      const bool okl = ram_coef(cp, Pj, Pj1, z[r], dl, kl);
      if (!okl) *flag = 1;
      vd[r] = dl; vk[r] = kl;
    }
    bar();
    failed = *flag != 0;
    if (!failed && row) {   // S'_rj = S_rj d_j + G_rj kappa_j, G re-formed from the diagonal down (ram_factor_update_canon)
      double G = 0.0;
      for (int j = r; j >= 0; j--) {
        const double sij = ma(r, j);
        ma(r, j) = fmh_fma(G, vk[j], sij * vd[j]);
        G = fmh_fma(sij, z[j], G);
      }
    }
  }
  if (constr && row)   // Sigma <<- constr[which., which.] * Sigma (R/kernel_ram.R:149-150)
    for (int b = 0; b <= r; b++) ma(r, b) = constr[r * kf + b] * ma(r, b);
  bar();
  return failed;
}

// ---- the accept / store half of a callback step (mh_fun_step, mh_user_step): one launch per step, so everything carried lives
// in the caller's state / out buffers.  th0, th1: this thread's parameter of theta0 / theta1 (read and written under `par` only).
struct RoCarried {   // uniform: every thread keeps them
  int status;
  double f0;
  long long nacc;
};
template <class Args>
__device__ __forceinline__ RoCarried ro_carried(const Args& A, long long c, bool start) {
  return {start ? FMCMC_CHAIN_OK : A.status[c], start ? A.f1[c] : A.f0[c], start ? 0 : A.accept_count[c]};
}
// row ir of ans: kept when ir > burnin and (ir - burnin) mod thin == 0
template <class Args>
__device__ __forceinline__ void ro_store_row(const Args& A, long long c, int r, bool par, long long ir, const double* th0,
                                             const double* th1, double lpv) {
  if (ir > A.burnin && (ir - A.burnin) % A.thin == 0) {
    const long long s = (ir - A.burnin) / A.thin - 1;
    if (par) {
      A.samples[(c * A.k + r) * A.ldS + s] = *th0;
      if (A.draws) A.draws[(c * A.k + r) * A.ldS + s] = *th1;
    }
    if (A.logpost && r == 0) A.logpost[c * A.ldS + s] = lpv;
  }
}
template <class Args>
__device__ __forceinline__ void ro_fail(const Args& A, long long c, int r, bool par, int status, long long ir, const double* th1) {
  if (r == 0) { A.status[c] = status; A.status_step[c] = ir; }
  if (par) A.status_theta[c * A.k + r] = *th1;
}
// row 1 (R/mcmc.R:728-735): the accept words and the status reset, the row stored
template <class Args>
__device__ __forceinline__ void ro_row1(const Args& A, long long c, int r, int nth, bool par, const double* th0, const double* th1, double f0) {
  const long long nwords = (A.nsteps + 31) >> 5;
  if (A.accept_bits)
    for (long long w = r; w < nwords; w += nth) A.accept_bits[c * nwords + w] = 0u;
  if (r == 0) { A.status[c] = FMCMC_CHAIN_OK; A.status_step[c] = 0; }
  ro_store_row(A, c, r, par, 1, th0, th1, f0);
}
// step i (R/mcmc.R:754-778): the NaN checks, log u < ratio, theta0 / f0 / the count / the bit, the kept row.  f1: f(theta1), from
// wherever the caller keeps it (uniform).  bar(): between the new theta0 and its readers, for a caller that keeps theta0 where
// other threads read it.
template <class Args, class Bar>
__device__ __forceinline__ void ro_accept_store(const Args& A, long long c, int r, bool par, long long i, double f1, double ratio,
                                                RoCarried& ch, double* th0, const double* th1, Bar bar) {
  if (fmh_isnan(f1)) ch.status = FMCMC_CHAIN_NAN_LOGPOST;
  else if (fmh_isnan(ratio)) ch.status = FMCMC_CHAIN_NAN_RATIO;
  if (ch.status != FMCMC_CHAIN_OK) {
    ro_fail(A, c, r, par, ch.status, i, th1);
    return;
  }
  if (ro_log_u(A, c, i) < ratio) {
    if (par) *th0 = *th1;
    ch.f0 = f1;
    ch.nacc += 1;
    if (A.accept_bits && r == 0) A.accept_bits[c * ((A.nsteps + 31) >> 5) + ((i - 1) >> 5)] |= (1u << ((i - 1) & 31));
  }
  bar();
  ro_store_row(A, c, r, par, i, th0, th1, f1);
}
template <class Args>
__device__ __forceinline__ void ro_write_back(const Args& A, long long c, int r, bool par, const RoCarried& ch, const double* th0) {
  if (par) A.theta0[c * A.k + r] = *th0;
  if (r == 0) {
    A.f0[c] = ch.f0;
    A.accept_count[c] = ch.nacc;
  }
}

}  // namespace
