// diag_loo_predictive.hpp — leave-one-out predictive checks from the Pareto-smoothed importance weights that diag_loo.hpp builds:
// per observation the LOO predictive mean and sd and the LOO probability integral transform of y_i (loo::E_loo, bayesplot's
// ppc_loo_pit), for the Gaussian regression and the logistic family (the definition is INTEGRATION.md §2.2, the host restatement
// fmcmc_amd/summary.py: loo_predictive_host, the kernels, the scratch and the measured errors DESIGN.md §5.10).  Included by
// summary.hip behind diag_loo.hpp, whose whole call (loo_run) runs first and leaves the sorted tail, the capped log weights of
// the tail ranks and the six numbers of its `point`; WAIC's a and w of the draws are still in `work`.
//
// Every E_loo[h] = sum_s omega_s h_s / sum_s omega_s.  The weight of a draw is a function of the VALUE of its r = -l (the
// order-preserving key of the device's own r, diag_common.hpp: key_of), so ties, which repeated MH rows make the normal case,
// cannot make it depend on the order in which equal values were appended to the tail:
//   lpd_draw_kernel     a thread a draw: 1 / sigma and sigma^2 into `work` (Gaussian family).
//   lpd_runs_kernel     a workgroup an observation: for every run of equal keys of the sorted tail the mean of exp(lambda_j), the
//                       sum taken by the thread of the run's first rank in rank order: wbar [n][M]; the run that equals the cutoff
//                       (if the tail starts with one) leaves its length c_T and its sum in bnd [n][2].
//   lpd_tile_kernel<.>  one more sweep of the tiles in WAIC's part structure with the evaluation of loo_tile_kernel restated, so
//                       that r has the bits of the collect pass.  Per element: key below the cutoff's: omega = fmh_exp(r - R); above:
//                       wbar at the position a binary search of the sorted tail finds (through L2: 64 observations share a
//                       workgroup), counted when the key found there is the element's; equal: unweighted sums and a count.  A lane
//                       keeps sum omega, sum omega d, sum omega (d^2 + sigma^2), sum omega Phi(-d / sigma) (logistic: sum omega
//                       expit(eta)); the four lane groups of an observation merge in the order ((0 + 1) + 2) + 3: one partial of
//                       LPD_SLOTS per (part, observation).
//   lpd_finish_kernel   a thread an observation: the parts in part order, the weight of the boundary run, the integrity check
//                       (found above the cutoff == M - c_T, equal to it >= c_T + 1), mean, sd, pit and loo's k, n_eff, elpd_i.
//   lpd_count_kernel    one workgroup: the rows that are not finite.
// No floating-point atomics, every sum in a fixed order, the plan that of loo (a function of (chains, N, n) alone): the same bits
// on every call, wherever the window sits.
#pragma once

namespace {

constexpr int LPD_SLOTS = 10;           // 8-byte slots per (part, observation): the sums below, then two integer counts
enum { LPD_W = 0, LPD_WD, LPD_WQ, LPD_WP, LPD_ED, LPD_EQ, LPD_EP, LPD_NGT, LPD_NEQ };

struct LpdPlan {
  // behind loo's `work`: the tail [n][M], its capped log weights [n][M], the run means [n][M], the boundary run [n][2], loo's
  // point [n][6] (where the caller wants none), 1 / sigma and sigma^2 [2][S'] (Gaussian family), the partials
  // [nparts][n][LPD_SLOTS]
  long long off_tail, off_lw, off_wbar, off_bnd, off_pt, off_rsig, off_sig2, off_part, len;
};

inline LpdPlan lpd_plan(const WaicPlan& W, const LooPlan& L, long long cpg, long long N, long long n) {
  LpdPlan D;
  D.off_tail = L.len;
  D.off_lw = D.off_tail + n * L.M;
  D.off_wbar = D.off_lw + n * L.M;
  D.off_bnd = D.off_wbar + n * L.M;
  D.off_pt = D.off_bnd + 2 * n;
  D.off_rsig = D.off_pt + 6 * n;
  D.off_sig2 = D.off_rsig + (W.gauss ? cpg * N : 0);
  D.off_part = D.off_sig2 + (W.gauss ? cpg * N : 0);
  D.len = D.off_part + W.nparts * n * LPD_SLOTS;
  return D;
}

struct LpdArgs {
  WaicArgs W;
  LpdPlan D;
  long long M;
  const double* loo_pt;                 // loo's point [n][6], in the caller's buffer or in `work`
  double* point; double* total;
};

// One copy of fmh_pnorm_both in a kernel, however often its loop is unrolled.
__device__ __noinline__ double lpd_phi(double u) {
  double lower, upper;
  fmh_pnorm_both(u, &lower, &upper);
  return lower;
}

__device__ __forceinline__ double lpd_expit(double eta) {   // (the branch form of diag_predict.hpp: pred_expit)
  const double e = fmh_exp(-fmh_abs(eta));
  return eta >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

__global__ __launch_bounds__(LOO_T) void lpd_draw_kernel(LpdArgs Q) {
  const WaicArgs& A = Q.W;
  const long long e = (long long)blockIdx.x * LOO_T + threadIdx.x;
  if (e >= A.cpg * A.N) return;
  const long long c = e / A.N, row = e % A.N;
  const double sigma = A.samples[c * A.k * A.S + (long long)(A.k - 1) * A.S + A.row0 + row];
  A.work[Q.D.off_rsig + e] = 1.0 / sigma;
  A.work[Q.D.off_sig2 + e] = sigma * sigma;
}

__global__ __launch_bounds__(LOO_T) void lpd_runs_kernel(LpdArgs Q) {
  const WaicArgs& A = Q.W;
  const long long obs = blockIdx.x, M = Q.M;
  const double* __restrict__ tail = A.work + Q.D.off_tail + obs * M;
  const double* __restrict__ lw = A.work + Q.D.off_lw + obs * M;
  double* __restrict__ wbar = A.work + Q.D.off_wbar + obs * M;
  const unsigned long long ckey = key_of(Q.loo_pt[obs * 6 + 5]);
  for (long long j = threadIdx.x; j < M; j += LOO_T) {
    const unsigned long long kj = key_of(tail[j]);
    if (j > 0 && key_of(tail[j - 1]) == kj) continue;               // (not the first rank of its run)
    double sum = 0.0;
    long long b = j;
    for (; b < M && key_of(tail[b]) == kj; b++) sum += fmh_exp(lw[b]);
    const double mean = sum / (double)(b - j);
    for (long long i = j; i < b; i++) wbar[i] = mean;
    if (j == 0) {
      double* bnd = A.work + Q.D.off_bnd + 2 * obs;
      bnd[0] = kj == ckey ? (double)b : 0.0;
      bnd[1] = kj == ckey ? sum : 0.0;
    }
  }
}

// The tile evaluation of loo_tile_kernel<., LOO_COLLECT> (diag_loo.hpp), restated with another use of every element.  NQR: the
// steps of four operand columns whose B values a lane keeps in registers; 0: the B tile lives in LDS.
template <int NQR>
__global__ __launch_bounds__(LOO_T) void lpd_tile_kernel(LpdArgs Q) {
  constexpr bool LDSB = NQR == 0;
  constexpr int NB = NQR ? NQR : 1;
  extern __shared__ double s_b[];
  const WaicArgs& A = Q.W;
  const WaicPlan& P = A.P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, col = lane & 15;
  const long long tile = blockIdx.x, part = blockIdx.y, M = Q.M;
  const long long obs = tile * 64 + wave * 16 + col;
  const bool obs_ok = obs < A.n;
  const long long oo = obs_ok ? obs : 0;
  const double* __restrict__ X = A.X;
  const double* __restrict__ y = A.y;
  const int nq = P.nq, ncoef = P.ncoef, onecol = P.onecol;
  auto bval = [&](int q) -> double {
    const int j = 4 * q + kk;
    if (!obs_ok) return 0.0;
    if (j < ncoef) return (P.ic && j == 0) ? 1.0 : X[(long long)(j - P.ic) * A.n + obs];
    return j == onecol ? -y[obs] : 0.0;
  };
  double b[NB];
  if (LDSB) {
    for (int q = 0; q < nq; q++) s_b[(q * 4 + wave) * 64 + lane] = bval(q);
  } else {
#pragma unroll
    for (int q = 0; q < NB; q++) b[q] = q < nq ? bval(q) : 0.0;
  }
  const bool ypos = !P.gauss && obs_ok && y[obs] != 0.0;
  const double* __restrict__ tail = A.work + Q.D.off_tail + oo * M;
  const double* __restrict__ wbar = A.work + Q.D.off_wbar + oo * M;
  const double R = tail[M - 1];
  const unsigned long long ckey = key_of(Q.loo_pt[oo * 6 + 5]);

  const long long i0 = part * P.upp, i1 = i0 + P.upp < P.U ? i0 + P.upp : P.U;
  const double* __restrict__ smp = A.samples + A.row0;
  const double* __restrict__ av = A.work;
  const double* __restrict__ wv = av + P.off_w;
  const double* __restrict__ rsig = A.work + Q.D.off_rsig;
  const double* __restrict__ sig2 = A.work + Q.D.off_sig2;
  double sw = 0.0, swd = 0.0, swq = 0.0, swp = 0.0, ed = 0.0, eq = 0.0, ep = 0.0;
  unsigned long long ngt = 0ull, neq = 0ull;
  for (long long u = i0; u < i1; u++) {
    const long long c = u / P.T, t = u - c * P.T;
    const long long rb = 16 * t;
    const int valid = A.N - rb < 16 ? (int)(A.N - rb) : 16;
    const double* __restrict__ base = smp + c * A.k * A.S + rb + col;
    const bool aok = col < valid;
    waic_d4 acc = {0.0, 0.0, 0.0, 0.0};
    if (LDSB) {
      for (int q = 0; q < nq; q++) {
        const int j = 4 * q + kk;
        const double a = j < ncoef ? (aok ? base[(long long)j * A.S] : 0.0) : (j == onecol ? 1.0 : 0.0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, s_b[(q * 4 + wave) * 64 + lane], acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < NB; q++) {
        if (q < nq) {
          const int j = 4 * q + kk;
          const double a = j < ncoef ? (aok ? base[(long long)j * A.S] : 0.0) : (j == onecol ? 1.0 : 0.0);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[q], acc, 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int rr = 4 * r + kk;
      if (rr >= valid || !obs_ok) continue;
      const double eta = acc[r];                      // Gaussian: eta - y_i (the column of ones against -y_i)
      double l, hq = 0.0, hp;
      if (P.gauss) {
        const long long di = c * A.N + rb + rr;
        l = fmh_fma(-wv[di], eta * eta, av[di]);
        hq = fmh_fma(eta, eta, sig2[di]);
        hp = lpd_phi(-eta * rsig[di]);
      } else {
        const double ts = ypos ? eta : -eta;
        l = (ts < 0.0 ? ts : 0.0) - fmh_log1p(fmh_exp(-fmh_abs(ts)));
        hp = lpd_expit(eta);
      }
      const double rv = -l;
      const unsigned long long key = key_of(rv);
      if (key == ckey) {
        neq++;
        ed += eta; eq += hq; ep += hp;
        continue;
      }
      double w;
      if (key < ckey) {
        w = fmh_exp(rv - R);
      } else {
        long long lo = 0, hi = M;                     // the first rank whose key is not below the element's
        while (lo < hi) {
          const long long mid = (lo + hi) >> 1;
          if (key_of(tail[mid]) < key) lo = mid + 1; else hi = mid;
        }
        const long long pos = lo < M ? lo : M - 1;
        ngt += key_of(tail[pos]) == key ? 1ull : 0ull;
        w = wbar[pos];
      }
      sw += w;
      swd = fmh_fma(w, eta, swd);
      swq = fmh_fma(w, hq, swq);
      swp = fmh_fma(w, hp, swp);
    }
  }
  double v[7] = {sw, swd, swq, swp, ed, eq, ep}, m7[7];
#pragma unroll
  for (int q = 0; q < 7; q++) {
#pragma unroll
    for (int gs = 0; gs < 4; gs++) {                  // the four lane groups of an observation, ((0 + 1) + 2) + 3
      const double o = __shfl(v[q], col + 16 * gs, 64);
      m7[q] = gs == 0 ? o : m7[q] + o;
    }
  }
  unsigned long long cg = 0ull, ce = 0ull;
#pragma unroll
  for (int gs = 0; gs < 4; gs++) {
    cg += __shfl(ngt, col + 16 * gs, 64);
    ce += __shfl(neq, col + 16 * gs, 64);
  }
  if (kk == 0 && obs_ok) {
    double* o = A.work + Q.D.off_part + (part * A.n + obs) * LPD_SLOTS;
#pragma unroll
    for (int q = 0; q < 7; q++) o[q] = m7[q];
    unsigned long long* oc = reinterpret_cast<unsigned long long*>(o);
    oc[LPD_NGT] = cg; oc[LPD_NEQ] = ce;
  }
}

__global__ __launch_bounds__(LOO_T) void lpd_finish_kernel(LpdArgs Q) {
  const WaicArgs& A = Q.W;
  const WaicPlan& P = A.P;
  const long long obs = (long long)blockIdx.x * LOO_T + threadIdx.x, M = Q.M;
  if (obs >= A.n) return;
  double s[7];
  unsigned long long ngt = 0ull, neq = 0ull;
  for (long long part = 0; part < P.nparts; part++) {
    const double* __restrict__ o = A.work + Q.D.off_part + (part * A.n + obs) * LPD_SLOTS;
    const unsigned long long* __restrict__ oc = reinterpret_cast<const unsigned long long*>(o);
#pragma unroll
    for (int q = 0; q < 7; q++) s[q] = part == 0 ? o[q] : s[q] + o[q];
    ngt += oc[LPD_NGT]; neq += oc[LPD_NEQ];
  }
  const double* __restrict__ pt = Q.loo_pt + obs * 6;
  const double* __restrict__ bnd = A.work + Q.D.off_bnd + 2 * obs;
  double* out = Q.point + obs * 6;
  const double elpd = pt[0], kpar = pt[3], neff = pt[4], cutoff = pt[5];
  const bool loo_ok = elpd == elpd && neff == neff && kpar == kpar && cutoff == cutoff;
  const double cT = loo_ok ? bnd[0] : 0.0;
  const bool ok = loo_ok && (double)ngt == (double)M - cT && (double)neq >= cT + 1.0;
  if (!ok) {
#pragma unroll
    for (int q = 0; q < 6; q++) out[q] = fmh_nan();
    return;
  }
  const double R = A.work[Q.D.off_tail + obs * M + M - 1], dneq = (double)neq;
  const double wc = fmh_fma(dneq - cT, fmh_exp(cutoff - R), bnd[1]) / dneq;    // the weight of every draw of the boundary run
  const double den = fmh_fma(wc, dneq, s[LPD_W]);
  const double e_d = fmh_fma(wc, s[LPD_ED], s[LPD_WD]) / den;
  const double e_q = fmh_fma(wc, s[LPD_EQ], s[LPD_WQ]) / den;
  const double e_p = fmh_fma(wc, s[LPD_EP], s[LPD_WP]) / den;
  if (P.gauss) {
    out[0] = A.y[obs] + e_d;
    out[1] = fmh_sqrt(e_q - e_d * e_d);
    out[2] = e_p;
  } else {
    out[0] = e_p;
    out[1] = fmh_sqrt(e_p * (1.0 - e_p));
    out[2] = fmh_nan();
  }
  out[3] = kpar; out[4] = neff; out[5] = elpd;
}

__global__ __launch_bounds__(LOO_T) void lpd_count_kernel(LpdArgs Q) {
  __shared__ double red[LOO_T / 64];
  const WaicArgs& A = Q.W;
  double bad = 0.0;
  for (long long i = threadIdx.x; i < A.n; i += LOO_T)
    bad += (fmh_isfinite(Q.point[6 * i]) && fmh_isfinite(Q.point[6 * i + 1])) ? 0.0 : 1.0;
  bad = block_sum<LOO_T / 64>(bad, red);
  if (threadIdx.x == 0) Q.total[12] = bad;
}

template <int NQR>
int lpd_launch_tile(const char* who, const LpdArgs& Q, size_t lds, hipStream_t st) {
  const WaicPlan& P = Q.W.P;
  if (lds) {
    const int rc = allow_lds(who, lpd_tile_kernel<NQR>, lds);
    if (rc != FMCMC_OK) return rc;
  }
  hipLaunchKernelGGL((lpd_tile_kernel<NQR>), dim3((unsigned)P.tiles, (unsigned)P.nparts), dim3(LOO_T), lds, st, Q);
  return FMCMC_OK;
}

inline int lpd_family(const char* who, const fmcmc_model* m) {
  if (m->family == FMCMC_FAM_IID_NORMAL)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: iid_normal has no covariates to predict at; the families are gaussian_linreg and "
                "logistic", who);
  return FMCMC_OK;
}

}  // namespace

extern "C" {

int64_t fmcmc_loo_predictive_work_len(const fmcmc_model* m, int64_t nchains, int64_t N) {
  const int64_t base = fmcmc_loo_work_len(m, 1, nchains, N);
  if (base == 0 || m->family == FMCMC_FAM_IID_NORMAL) return 0;
  const WaicPlan W = waic_plan(m, 1, nchains, N);
  const LooPlan L = loo_plan(W, 1, nchains, N, m->n);
  return lpd_plan(W, L, nchains, N, m->n).len;
}

int fmcmc_loo_predictive_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0,
                             int64_t N, double* work, double* point, double* loo_point, double* total, void* hip_stream) {
  const char* who = "fmcmc_loo_predictive_dev";
  if (!m || !samples || !work || !point || !total) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = lpd_family(who, m);
  if (rc != FMCMC_OK) return rc;
  if ((rc = loo_check(who, m, 0, 0, samples, 1, nchains, k, S, row0, N)) != FMCMC_OK) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  LpdArgs Q;
  WaicArgs& A = Q.W;
  A.samples = samples; A.X = m->X; A.y = m->y; A.active = nullptr; A.work = work;
  A.x_stride = 0; A.y_stride = 0; A.S = S; A.row0 = row0; A.N = N; A.n = m->n; A.cpg = nchains;
  A.k = k;
  A.P = waic_plan(m, 1, nchains, N);
  const LooPlan L = loo_plan(A.P, 1, nchains, N, m->n);
  Q.D = lpd_plan(A.P, L, nchains, N, m->n);
  Q.M = L.M;
  double* lpt = loo_point ? loo_point : work + Q.D.off_pt;
  Q.loo_pt = lpt; Q.point = point; Q.total = total;
  if ((rc = loo_run(who, m, 0, 0, samples, 1, nchains, k, S, row0, N, nullptr, work, lpt, work + Q.D.off_tail, work + Q.D.off_lw,
                    total, hip_stream)) != FMCMC_OK)
    return rc;
  const WaicPlan& P = A.P;
  if (P.gauss) hipLaunchKernelGGL(lpd_draw_kernel, dim3((unsigned)P.nblk), dim3(LOO_T), 0, st, Q);
  hipLaunchKernelGGL(lpd_runs_kernel, dim3((unsigned)A.n), dim3(LOO_T), 0, st, Q);
  if (P.nq <= 2) rc = lpd_launch_tile<2>(who, Q, 0, st);
  else if (P.nq <= 4) rc = lpd_launch_tile<4>(who, Q, 0, st);
  else if (P.nq <= WAIC_REG_Q) rc = lpd_launch_tile<WAIC_REG_Q>(who, Q, 0, st);
  else rc = lpd_launch_tile<0>(who, Q, (size_t)P.nq * LOO_T * sizeof(double), st);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(lpd_finish_kernel, dim3((unsigned)((A.n + LOO_T - 1) / LOO_T)), dim3(LOO_T), 0, st, Q);
  hipLaunchKernelGGL(lpd_count_kernel, dim3(1), dim3(LOO_T), 0, st, Q);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

}  // extern "C"
