// diag_predictive.hpp — the posterior predictive distribution of a new OBSERVATION y at a point for the Gaussian regression family:
// its quantiles (prediction intervals) and the probability integral transform of a given y, from the kept rows where the sweep
// left them (the definition is INTEGRATION.md §2.2, the host restatement fmcmc_amd/summary.py: predictive_host, the kernels, the
// scratch, the derivation of the constant c and the times DESIGN.md §5.10).  Included by summary.hip behind diag_predict.hpp: it
// reuses diag_waic.hpp's split of the draws into parts (waic_plan with n := the m points) and diag_predict.hpp's Chan merges
// (pred_merge, pred_merge_groups), and RESTATES the tile evaluation of pred_tile_kernel (pdv_walk), so that predict()'s object
// code, and with it its bits, is not touched.
//
// The predictive distribution is a mixture of S' normals, F_i(t) = (1 / S') sum_s Phi((t - eta_si) / sigma_s); nothing is simulated:
//   pdv_draw_kernel      a thread a draw: bad draws as pred_draw_kernel counts them, sigma^2, min and max sigma: a workgroup's
//                        values into `work`; 1 / sigma_s into `work` for the evaluation passes.
//   pdv_total_kernel     one workgroup: those partials in index order.
//   pdv_tile_kernel<., PDV_FOLD>   a workgroup = 64 points x one part of the draws: (count, mean, M2) of eta as PRED_FOLD has
//                        them, and min eta, max eta; one partial per (part, point).
//   pdv_init_kernel      a thread a point: the parts in part order; mean, sd_pred; per prob a bracket that encloses the root and
//                        the start t0; the PIT's slot starts (and stays) at y_i.
//   pdv_tile_kernel<., PDV_EVAL>   THE HOT PATH.  The same workgroup; every lane holds the four eta of its point in a tile and, for
//                        a batch of up to PDV_BATCH slots, the point's current t, a tail sum and a density sum in registers.  Per
//                        element and slot: u = (t - eta) (1 / sigma_s), one fmh_pnorm_ex; the lower tail is summed for p <= 1/2,
//                        the upper for p > 1/2 (against 1 - p, which is exact there); the four lane groups of a point are merged
//                        in the order ((0 + 1) + 2) + 3 and one partial {tail, density} per (part, point, slot) goes to `work`.
//                        The PIT is one such pass with one slot and {lower, upper} for its two sums.  A workgroup whose 64 points
//                        are finished in every slot of the batch returns at once: pdv_step_kernel never reads a finished slot's
//                        partials, so nothing depends on whether it does.
//   pdv_step_kernel      a thread a (point, slot): the parts in part order, g = F - p (or its upper-tail form), the convergence
//                        test, the bracket end of g's sign moves to t, then the Newton step t - g / f, or the midpoint where that
//                        leaves the bracket, f is 0, or neither the bracket at least halved over the last two passes nor |g|
//                        over the last one.
//   pdv_finish_kernel    a thread a point: point[i]; pdv_count_kernel: one workgroup, total[0 .. 6).
// No floating-point atomics, every sum in a fixed order, the plan a function of (chains, N, m) alone: the same bits on every call.
// Only FMCMC_FAM_GAUSSIAN_LINREG: the predictive distribution of a logistic y is Bernoulli(mean of epred), which predict() returns
// already, and iid_normal has no covariates.
#pragma once

namespace {

constexpr int PDV_BATCH = 8;            // slots (probs) whose t and sums a lane of the evaluation pass keeps in registers
constexpr int PDV_STATE = 8;            // doubles of state per (point, slot)
enum { PDV_ST_T = 0, PDV_ST_LO, PDV_ST_HI, PDV_ST_G, PDV_ST_DONE, PDV_ST_W1, PDV_ST_W2, PDV_ST_F };
enum { PDV_FOLD = 0, PDV_EVAL = 1 };
constexpr int PDV_TOT = 8;              // S', bad draws, mean sigma^2, min sigma, max sigma, passes done so far, 2 spare

struct PdvPlan {
  int ic, ncoef, nq, nprobs, nslots;    // nslots = nprobs + 1: the last slot is the PIT's
  long long T, U, upp, nparts, tiles, nblk;
  // `work`: per 256 draws {bad, sigma^2, min sigma, max sigma} [4][nblk] at 0, the totals [PDV_TOT], 1 / sigma [S'], the fold's
  // partials [nparts][m][4], the head {mean, sd_pred, min eta, max eta} [m][4], the state [m][nslots][PDV_STATE], the
  // evaluation's partials [nparts][m][PDV_BATCH][2], the PIT's [nparts][m][2]
  long long off_tot, off_rsig, off_fold, off_head, off_state, off_eval, off_pit, len;
};

inline PdvPlan pdv_plan(const fmcmc_model* m, long long cpg, long long N, int nprobs) {
  const WaicPlan W = waic_plan(m, 1, cpg, N);
  PdvPlan P;
  P.ic = m->intercept ? 1 : 0;
  P.ncoef = P.ic + m->p;
  P.nq = (P.ncoef + 3) / 4;
  P.nprobs = nprobs;
  P.nslots = nprobs + 1;
  P.T = W.T; P.U = W.U; P.upp = W.upp; P.nparts = W.nparts; P.tiles = W.tiles; P.nblk = W.nblk;
  P.off_tot = 4 * P.nblk;
  P.off_rsig = P.off_tot + PDV_TOT;
  P.off_fold = P.off_rsig + cpg * N;
  P.off_head = P.off_fold + P.nparts * m->n * 4;
  P.off_state = P.off_head + m->n * 4;
  P.off_eval = P.off_state + m->n * P.nslots * PDV_STATE;
  P.off_pit = P.off_eval + P.nparts * m->n * PDV_BATCH * 2;
  P.len = P.off_pit + P.nparts * m->n * 2;
  return P;
}

// The convergence test |g| <= tol(p) = c eps min(p, 1 - p), eps = 2^-52.  g = T / S' - p with T the tail sum as the kernels form
// it; every term is positive, so the relative error of T is at most the sum of the relative errors along the longest chain of
// operations that one term passes through, to first order, each rounding counting eps / 2:
//   the term itself        fmh_pnorm_ex of u: 2 FMH_PNORM_REL (twice the largest error measured; tests/test_pnorm_host.py
//                          asserts that bound)                                                       -> 4 FMH_PNORM_REL / eps  halves
//   a lane's sum           at most 4 rows of each of the upp tiles of a part: 4 min(upp, U) additions
//   the lane groups        ((0 + 1) + 2) + 3: 3 additions
//   the parts              in part order: nparts - 1 additions
//   T / S' and the subtraction of p (for |g| <= tol the difference of two numbers within a factor of 2 is exact; counted
//                          anyway): 2
// c = (4 min(upp, U) + 3 + (nparts - 1) + 2) / 2 + 2 FMH_PNORM_REL / eps.  The rounding of u itself moves t, not F: it is inside
// the other criterion (the bracket no wider than 2 ulp of its larger end).  Below tol the sign of g carries no information;
// above it, it is the sign of the true F - p, which is what keeps the bracket true.  summary.py: predictive_tol is the same line.
inline double pdv_c(const PdvPlan& P) {
  const long long per_lane = 4 * (P.upp < P.U ? P.upp : P.U);
  return 0.5 * (double)(per_lane + 3 + (P.nparts - 1) + 2) + 2.0 * FMH_PNORM_REL / 2.220446049250313e-16;
}

struct PdvProbs {                       // per prob: z = fmh_qnorm(p), side = min(p, 1 - p) (exact for p >= 1/2), tol = c eps side
  double z[PRED_MAX_PROBS], side[PRED_MAX_PROBS], tol[PRED_MAX_PROBS];
};

struct PdvArgs {
  const double* samples; const double* X; const double* y; double* work;
  long long S, row0, N, n, cpg;
  int k, slot0, nb, pass, pit, npasses;   // a pass's batch: the slots [slot0, slot0 + nb); pass = 1 .. npasses within the call
  unsigned int upmask;                  // bit i: prob i > 1/2, its sums are upper tails
  PdvPlan P;
};

// the spacing of the doubles at |x| (numpy.spacing), x finite
__device__ __forceinline__ double pdv_ulp(double x) {
  const uint64_t e = (fmh_d2u(x) >> 52) & 0x7ffu;
  return e > 52 ? fmh_u2d((e - 52) << 52) : fmh_u2d(1ull << (e > 0 ? e - 1 : 0));
}

// One copy of fmh_pnorm_ex in a kernel, however often its loops are unrolled.
struct PdvPhi { double lower, upper, ex; };
__device__ __noinline__ PdvPhi pdv_phi(double u) {
  PdvPhi r;
  fmh_pnorm_ex(u, &r.lower, &r.upper, &r.ex);
  return r;
}

__global__ __launch_bounds__(PRED_T) void pdv_draw_kernel(PdvArgs A) {
  __shared__ double red[PRED_T / 64];
  __shared__ double red_mn[PRED_T / 64], red_mx[PRED_T / 64];
  const PdvPlan& P = A.P;
  const long long e = (long long)blockIdx.x * PRED_T + threadIdx.x;
  double bad = 0.0, s2 = 0.0, mn = fmh_inf(), mx = -fmh_inf();
  if (e < A.cpg * A.N) {
    const long long c = e / A.N, row = e % A.N;
    const double* __restrict__ th = A.samples + c * A.k * A.S + A.row0 + row;
    int nf = 0;
    for (int j = 0; j < A.k; j++) nf |= !fmh_isfinite(th[(long long)j * A.S]);
    const double sigma = th[(long long)(A.k - 1) * A.S];
    nf |= !(sigma > 0.0);
    s2 = sigma * sigma;
    if (sigma > 0.0) { mn = sigma; mx = sigma; }
    A.work[P.off_rsig + e] = 1.0 / sigma;
    bad = nf ? 1.0 : 0.0;
  }
  const double tb = block_sum<PRED_T / 64>(bad, red);
  const double ts = block_sum<PRED_T / 64>(s2, red);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {                 // (min and max are exact: any order gives the same value)
    const double a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) { red_mn[threadIdx.x >> 6] = mn; red_mx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < PRED_T / 64; w++) { mn = red_mn[w] < mn ? red_mn[w] : mn; mx = red_mx[w] > mx ? red_mx[w] : mx; }
    A.work[blockIdx.x] = tb; A.work[P.nblk + blockIdx.x] = ts; A.work[2 * P.nblk + blockIdx.x] = mn; A.work[3 * P.nblk + blockIdx.x] = mx;
  }
}

__global__ __launch_bounds__(PRED_T) void pdv_total_kernel(PdvArgs A) {
  __shared__ double red[PRED_T / 64];
  __shared__ double red_mn[PRED_T / 64], red_mx[PRED_T / 64];
  const PdvPlan& P = A.P;
  double bad = 0.0, s2 = 0.0, mn = fmh_inf(), mx = -fmh_inf();
  for (long long i = threadIdx.x; i < P.nblk; i += PRED_T) {
    bad += A.work[i]; s2 += A.work[P.nblk + i];
    const double a = A.work[2 * P.nblk + i], b = A.work[3 * P.nblk + i];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  bad = block_sum<PRED_T / 64>(bad, red);
  s2 = block_sum<PRED_T / 64>(s2, red);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double a = __shfl_xor(mn, o, 64), b = __shfl_xor(mx, o, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if ((threadIdx.x & 63) == 0) { red_mn[threadIdx.x >> 6] = mn; red_mx[threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < PRED_T / 64; w++) { mn = red_mn[w] < mn ? red_mn[w] : mn; mx = red_mx[w] > mx ? red_mx[w] : mx; }
    const double draws = (double)(A.cpg * A.N);
    double* t = A.work + P.off_tot;
    t[0] = draws; t[1] = bad; t[2] = s2 / draws; t[3] = mn; t[4] = mx; t[5] = 0.0; t[6] = 0.0; t[7] = 0.0;
  }
}

// The tile walk of pred_tile_kernel (diag_predict.hpp), restated: the workgroup's 64 points against the units of its part, 16 rows
// of one chain at a time, ceil(k' / 4) v_mfma_f64_16x16x4 a tile; use(eta, draw) for every element of the lane, draw = the row's
// index c N + row among the S' draws.  NQR: the steps of four operand columns whose B values a lane keeps in registers; 0: LDS.
template <int NQR, typename Use>
__device__ __forceinline__ void pdv_walk(const PdvArgs& A, double* s_b, long long obs, bool obs_ok, long long part, Use use) {
  constexpr bool LDSB = NQR == 0;
  constexpr int NB = NQR ? NQR : 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, col = lane & 15;
  const PdvPlan& P = A.P;
  const int nq = P.nq, ncoef = P.ncoef;
  auto bval = [&](int q) -> double {
    const int j = 4 * q + kk;
    if (!obs_ok || j >= ncoef) return 0.0;
    return (P.ic && j == 0) ? 1.0 : A.X[(long long)(j - P.ic) * A.n + obs];
  };
  double b[NB];
  if (LDSB) {
    for (int q = 0; q < nq; q++) s_b[(q * 4 + wave) * 64 + lane] = bval(q);
  } else {
#pragma unroll
    for (int q = 0; q < NB; q++) b[q] = q < nq ? bval(q) : 0.0;
  }
  const long long u0 = part * P.upp, u1 = u0 + P.upp < P.U ? u0 + P.upp : P.U;
  const double* __restrict__ smp = A.samples + A.row0;
  long long c = u0 / P.T, t = u0 - c * P.T;
  for (long long u = u0; u < u1; u++, t++) {
    if (t == P.T) { t = 0; c++; }
    const long long rb = 16 * t;
    const int valid = A.N - rb < 16 ? (int)(A.N - rb) : 16;
    const double* __restrict__ base = smp + c * A.k * A.S + rb + col;
    const bool aok = col < valid;
    waic_d4 acc = {0.0, 0.0, 0.0, 0.0};
    if (LDSB) {
      for (int q = 0; q < nq; q++) {
        const int j = 4 * q + kk;
        const double a = (j < ncoef && aok) ? base[(long long)j * A.S] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, s_b[(q * 4 + wave) * 64 + lane], acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < NB; q++) {
        if (q < nq) {
          const int j = 4 * q + kk;
          const double a = (j < ncoef && aok) ? base[(long long)j * A.S] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[q], acc, 0, 0, 0);
        }
      }
    }
    // D register r of lane l is draw 4 r + l / 16, point l % 16
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int rr = 4 * r + kk;
      if (rr >= valid || !obs_ok) continue;
      use(acc[r], c * A.N + rb + rr);
    }
  }
}

template <int NQR, int MODE>
__global__ __launch_bounds__(PRED_T) void pdv_tile_kernel(PdvArgs A) {
  extern __shared__ double s_b[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, col = lane & 15;
  const PdvPlan& P = A.P;
  const long long tile = blockIdx.x, part = blockIdx.y;
  const long long obs = tile * 64 + wave * 16 + col;
  const bool obs_ok = obs < A.n;

  if (MODE == PDV_FOLD) {
    double K = 0.0, sd = 0.0, sdd = 0.0, mn = fmh_inf(), mx = -fmh_inf();
    int cnt = 0;
    pdv_walk<NQR>(A, s_b, obs, obs_ok, part, [&](double eta, long long) {
      if (cnt == 0) K = eta;
      cnt++;
      const double d = eta - K;
      sd += d;
      sdd = fmh_fma(d, d, sdd);
      mn = eta < mn ? eta : mn;
      mx = eta > mx ? eta : mx;
    });
    const PredAcc e4 = pred_merge_groups(pred_lane_acc(cnt, K, sd, sdd), col);
#pragma unroll
    for (int gs = 1; gs < 4; gs++) {                  // (from lane col + 16 gs to lane col; the other lanes' values are not used)
      const double a = __shfl(mn, (lane + 16 * gs) & 63, 64), b = __shfl(mx, (lane + 16 * gs) & 63, 64);
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
    }
    if (kk == 0 && obs_ok) {
      double* o = A.work + P.off_fold + (part * A.n + obs) * 4;
      o[0] = e4.mean; o[1] = e4.M2; o[2] = mn; o[3] = mx;
    }
  } else {
    double tq[PDV_BATCH], s0[PDV_BATCH], s1[PDV_BATCH];
    unsigned int live = 0u;
    const double* __restrict__ st = A.work + P.off_state + ((obs_ok ? obs : 0) * P.nslots + A.slot0) * PDV_STATE;
#pragma unroll
    for (int s = 0; s < PDV_BATCH; s++) {
      tq[s] = 0.0; s0[s] = 0.0; s1[s] = 0.0;
      if (s < A.nb && obs_ok) {
        tq[s] = st[s * PDV_STATE + PDV_ST_T];
        if (st[s * PDV_STATE + PDV_ST_DONE] == 0.0) live |= 1u << s;
      }
    }
    if (__syncthreads_or((int)live) == 0) return;     // all 64 points finished in every slot of the batch
    const double* __restrict__ rsig = A.work + P.off_rsig;
    const unsigned int up = A.upmask >> A.slot0;
    const bool pit = A.pit != 0;
    pdv_walk<NQR>(A, s_b, obs, obs_ok, part, [&](double eta, long long draw) {
      const double rs = rsig[draw];
#pragma unroll
      for (int s = 0; s < PDV_BATCH; s++) {
        if (!((live >> s) & 1u)) continue;
        const PdvPhi f = pdv_phi((tq[s] - eta) * rs);
        if (pit) {
          s0[s] += f.lower;
          s1[s] += f.upper;
        } else {
          s0[s] += ((up >> s) & 1u) ? f.upper : f.lower;
          s1[s] = fmh_fma(f.ex * FMH_INV_SQRT_2PI, rs, s1[s]);
        }
      }
    });
#pragma unroll
    for (int s = 0; s < PDV_BATCH; s++) {
      if (s >= A.nb) continue;                        // (the same for every lane)
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int gs = 0; gs < 4; gs++) {                // ((0 + 1) + 2) + 3, as pred_merge_groups
        const double o0 = __shfl(s0[s], col + 16 * gs, 64), o1 = __shfl(s1[s], col + 16 * gs, 64);
        a0 = gs == 0 ? o0 : a0 + o0;
        a1 = gs == 0 ? o1 : a1 + o1;
      }
      if (kk == 0 && obs_ok) {
        double* o = pit ? A.work + P.off_pit + (part * A.n + obs) * 2
                        : A.work + P.off_eval + ((part * A.n + obs) * PDV_BATCH + s) * 2;
        o[0] = a0; o[1] = a1;
      }
    }
  }
}

// A thread a point: the fold's parts in part order, the head, and the start of every slot.  The bracket: the p-quantile of every
// component lies in [min eta + z sigma', max eta + z sigma''] with sigma', sigma'' the end of [min sigma, max sigma] that makes
// the term smallest, largest; a mixture's p-quantile lies between the least and the largest of its components' (at the least,
// every component's CDF is <= p; at the largest, >= p).  Widened by 2^-46 |z| max sigma (fmh_qnorm's relative error, 4e-15,
// and the roundings of the two products) and 2^-50 of the larger end (the rounding of the sums).
__global__ __launch_bounds__(PRED_T) void pdv_init_kernel(PdvArgs A, PdvProbs R) {
  const PdvPlan& P = A.P;
  const long long obs = (long long)blockIdx.x * PRED_T + threadIdx.x;
  if (obs >= A.n) return;
  const double* __restrict__ tot = A.work + P.off_tot;
  PredAcc e;
  double mn = fmh_inf(), mx = -fmh_inf();
  for (long long part = 0; part < P.nparts; part++) {
    const long long u0 = part * P.upp, u1 = u0 + P.upp < P.U ? u0 + P.upp : P.U;
    const double* __restrict__ o = A.work + P.off_fold + (part * A.n + obs) * 4;
    PredAcc be;
    be.cnt = (double)waic_unit_rows(u0, u1, P.T, A.N);
    be.mean = o[0]; be.M2 = o[1];
    e = part == 0 ? be : pred_merge(e, be);
    mn = o[2] < mn ? o[2] : mn;
    mx = o[3] > mx ? o[3] : mx;
  }
  const double draws = tot[0], smin = tot[3], smax = tot[4];
  const double mean = e.mean, sdp = fmh_sqrt(e.M2 / (draws - 1.0) + tot[2]);
  double* h = A.work + P.off_head + obs * 4;
  h[0] = mean; h[1] = sdp; h[2] = mn; h[3] = mx;
  double* st = A.work + P.off_state + obs * P.nslots * PDV_STATE;
  for (int i = 0; i < P.nslots; i++, st += PDV_STATE) {
    double t, lo, hi;
    if (i < P.nprobs) {
      const double z = R.z[i];
      lo = mn + z * (z < 0.0 ? smax : smin);
      hi = mx + z * (z < 0.0 ? smin : smax);
      const double big = fmh_abs(lo) > fmh_abs(hi) ? fmh_abs(lo) : fmh_abs(hi);
      const double pad = 1.4210854715202004e-14 * (fmh_abs(z) * smax) + 8.881784197001252e-16 * big;   // 2^-46, 2^-50
      lo -= pad;
      hi += pad;
      t = mean + sdp * z;
      t = t < lo ? lo : (t > hi ? hi : t);
    } else {
      t = A.y ? A.y[obs] : fmh_nan();
      lo = t; hi = t;
    }
    st[PDV_ST_T] = t; st[PDV_ST_LO] = lo; st[PDV_ST_HI] = hi; st[PDV_ST_G] = fmh_nan(); st[PDV_ST_DONE] = 0.0;
    st[PDV_ST_W1] = fmh_inf(); st[PDV_ST_W2] = fmh_inf(); st[PDV_ST_F] = 0.0;
  }
}

// A thread a (point, slot of the batch), after the batch's evaluation pass.
__global__ __launch_bounds__(PRED_T) void pdv_step_kernel(PdvArgs A, PdvProbs R) {
  const PdvPlan& P = A.P;
  const long long idx = (long long)blockIdx.x * PRED_T + threadIdx.x;
  if (idx >= A.n * A.nb) return;
  const long long obs = idx / A.nb;
  const int s = (int)(idx - obs * A.nb), slot = A.slot0 + s;
  double* st = A.work + P.off_state + (obs * P.nslots + slot) * PDV_STATE;
  if (st[PDV_ST_DONE] != 0.0) return;
  const double* __restrict__ tot = A.work + P.off_tot;
  double tail = 0.0, dens = 0.0;
  for (long long part = 0; part < P.nparts; part++) {
    const double* __restrict__ o = A.work + P.off_eval + ((part * A.n + obs) * PDV_BATCH + s) * 2;
    tail = part == 0 ? o[0] : tail + o[0];
    dens = part == 0 ? o[1] : dens + o[1];
  }
  const double draws = tot[0], pass = tot[5] + (double)A.pass;
  const double F = tail / draws, f = dens / draws;
  const double g = ((A.upmask >> slot) & 1u) ? R.side[slot] - F : F - R.side[slot];
  const double t = st[PDV_ST_T], gprev = st[PDV_ST_G];
  double lo = st[PDV_ST_LO], hi = st[PDV_ST_HI];
  st[PDV_ST_G] = g; st[PDV_ST_F] = f;
  if (fmh_abs(g) <= R.tol[slot]) {                    // finished: the Newton correction that this evaluation pays for is still
    const double tf = t - g / f;                      // applied where it stays inside the bracket (g is the residual before it)
    if (f > 0.0 && tf > lo && tf < hi) st[PDV_ST_T] = tf;
    st[PDV_ST_DONE] = pass;
    return;
  }
  if (g < 0.0) lo = t; else hi = t;
  st[PDV_ST_LO] = lo; st[PDV_ST_HI] = hi;
  const double w = hi - lo;
  const double big = fmh_abs(lo) > fmh_abs(hi) ? fmh_abs(lo) : fmh_abs(hi);
  if (w <= 2.0 * pdv_ulp(big)) { st[PDV_ST_DONE] = pass; return; }
  double tn = t - g / f;
  // Newton approaches a root in a convex or concave stretch from one side, and then only one end of the bracket moves: a pass
  // that at least halved |g| is making its own progress and is left alone (the first pass has no earlier g: NaN compares false)
  const bool stalled = w > 0.5 * st[PDV_ST_W2] && fmh_abs(g) > 0.5 * fmh_abs(gprev);
  const bool newton = f > 0.0 && tn > lo && tn < hi && !stalled;
  if (!newton) tn = lo + 0.5 * w;
  st[PDV_ST_W2] = st[PDV_ST_W1]; st[PDV_ST_W1] = w; st[PDV_ST_T] = tn;
}

// A thread a point: point[i] = {mean, sd_pred, pit, pit_upper, per prob t, g, hi - lo, the pass at which it finished}.
__global__ __launch_bounds__(PRED_T) void pdv_finish_kernel(PdvArgs A, double* __restrict__ point) {
  const PdvPlan& P = A.P;
  const long long obs = (long long)blockIdx.x * PRED_T + threadIdx.x;
  if (obs >= A.n) return;
  const double* __restrict__ h = A.work + P.off_head + obs * 4;
  double* out = point + obs * (4 + 4 * P.nprobs);
  out[0] = h[0]; out[1] = h[1];
  if (A.y) {
    double lower = 0.0, upper = 0.0;
    for (long long part = 0; part < P.nparts; part++) {
      const double* __restrict__ o = A.work + P.off_pit + (part * A.n + obs) * 2;
      lower = part == 0 ? o[0] : lower + o[0];
      upper = part == 0 ? o[1] : upper + o[1];
    }
    const double draws = A.work[P.off_tot];
    out[2] = lower / draws; out[3] = upper / draws;
  } else {
    out[2] = fmh_nan(); out[3] = fmh_nan();
  }
  const double* __restrict__ st = A.work + P.off_state + obs * P.nslots * PDV_STATE;
  for (int i = 0; i < P.nprobs; i++, st += PDV_STATE) {
    out[4 + 4 * i] = st[PDV_ST_T]; out[5 + 4 * i] = st[PDV_ST_G]; out[6 + 4 * i] = st[PDV_ST_HI] - st[PDV_ST_LO];
    out[7 + 4 * i] = st[PDV_ST_DONE];
  }
}

// One workgroup, behind everything else of the call: the (point, prob) not yet finished (an integer count: exact in any order),
// total[0 .. 6), and the passes that the state has now seen.
__global__ __launch_bounds__(PRED_T) void pdv_count_kernel(PdvArgs A, double* __restrict__ total) {
  __shared__ double red[PRED_T / 64];
  const PdvPlan& P = A.P;
  double open = 0.0;
  for (long long i = threadIdx.x; i < A.n * P.nprobs; i += PRED_T) {
    const long long obs = i / P.nprobs, slot = i - obs * P.nprobs;
    open += A.work[P.off_state + (obs * P.nslots + slot) * PDV_STATE + PDV_ST_DONE] == 0.0 ? 1.0 : 0.0;
  }
  open = block_sum<PRED_T / 64>(open, red);
  if (threadIdx.x == 0) {
    double* t = A.work + P.off_tot;
    for (int j = 0; j < 5; j++) total[j] = t[j];
    total[5] = open;
    t[5] = t[5] + (double)A.npasses;
  }
}

inline int pdv_check(const char* who, const fmcmc_model* m, int64_t cpg, int32_t k, int64_t S, int64_t row0, int64_t N,
                     const double* probs, int32_t nprobs) {
  if (!m) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (m->family == FMCMC_FAM_LOGISTIC)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: the predictive distribution of a logistic y is Bernoulli(mean of epred), which "
                "fmcmc_predict_dev returns (kind 1, point[i][0])", who);
  const int rc = pred_check(who, m, cpg, k, S, row0, N, PRED_LINPRED, nullptr, nprobs);
  if (rc != FMCMC_OK) return rc;
  if (probs)
    for (int i = 0; i < nprobs; i++)
      if (!(probs[i] > 0.0 && probs[i] < 1.0))
        return fail(FMCMC_ERR_ARG, "%s: probs[%d] = %g is not strictly inside (0, 1)", who, i, probs[i]);
  return FMCMC_OK;
}

template <int MODE>
int pdv_launch_tiles(const char* who, const PdvArgs& A, hipStream_t st) {
  const PdvPlan& P = A.P;
  const dim3 grid((unsigned)P.tiles, (unsigned)P.nparts);
  if (P.nq <= 2) {
    hipLaunchKernelGGL((pdv_tile_kernel<2, MODE>), grid, dim3(PRED_T), 0, st, A);
  } else if (P.nq <= 4) {
    hipLaunchKernelGGL((pdv_tile_kernel<4, MODE>), grid, dim3(PRED_T), 0, st, A);
  } else if (P.nq <= WAIC_REG_Q) {
    hipLaunchKernelGGL((pdv_tile_kernel<WAIC_REG_Q, MODE>), grid, dim3(PRED_T), 0, st, A);
  } else {
    const size_t lds = (size_t)P.nq * PRED_T * sizeof(double);
    const int rc = allow_lds(who, pdv_tile_kernel<0, MODE>, lds);
    if (rc != FMCMC_OK) return rc;
    hipLaunchKernelGGL((pdv_tile_kernel<0, MODE>), grid, dim3(PRED_T), lds, st, A);
  }
  return FMCMC_OK;
}

}  // namespace

extern "C" {

int64_t fmcmc_predictive_work_len(const fmcmc_model* m, int64_t nchains, int64_t N, int32_t nprobs) {
  if (!m) return 0;
  if (pdv_check("fmcmc_predictive_work_len", m, nchains, pred_family_k(m), N, 0, N, nullptr, nprobs) != FMCMC_OK) return 0;
  return pdv_plan(m, nchains, N, nprobs).len;
}

int fmcmc_predictive_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0,
                         int64_t N, const double* probs, int32_t nprobs, int32_t npasses, int32_t resume, double* work,
                         double* point, double* total, void* hip_stream) {
  const char* who = "fmcmc_predictive_dev";
  if (!m || !samples || !work || !point || !total || (nprobs > 0 && !probs)) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = pdv_check(who, m, nchains, k, S, row0, N, probs, nprobs);
  if (rc != FMCMC_OK) return rc;
  if (npasses < 1) return fail(FMCMC_ERR_ARG, "%s: npasses = %d: at least 1 is needed", who, (int)npasses);
  if (resume != 0 && resume != 1) return fail(FMCMC_ERR_ARG, "%s: resume = %d; 0 or 1", who, (int)resume);
  hipStream_t st = (hipStream_t)hip_stream;
  PdvArgs A;
  A.samples = samples; A.X = m->X; A.y = m->y; A.work = work;
  A.S = S; A.row0 = row0; A.N = N; A.n = m->n; A.cpg = nchains;
  A.k = k; A.slot0 = 0; A.nb = 0; A.pass = 0; A.pit = 0; A.npasses = npasses; A.upmask = 0u;
  A.P = pdv_plan(m, nchains, N, nprobs);
  const PdvPlan& P = A.P;
  PdvProbs R = {};
  const double c = pdv_c(P);
  for (int i = 0; i < nprobs; i++) {
    const bool up = probs[i] > 0.5;
    if (up) A.upmask |= 1u << i;
    R.z[i] = fmh_qnorm(probs[i]);
    R.side[i] = up ? 1.0 - probs[i] : probs[i];
    R.tol[i] = c * 2.220446049250313e-16 * R.side[i];
  }
  const dim3 per_point((unsigned)((A.n + PRED_T - 1) / PRED_T));
  if (!resume) {
    hipLaunchKernelGGL(pdv_draw_kernel, dim3((unsigned)P.nblk), dim3(PRED_T), 0, st, A);
    hipLaunchKernelGGL(pdv_total_kernel, dim3(1), dim3(PRED_T), 0, st, A);
    if ((rc = pdv_launch_tiles<PDV_FOLD>(who, A, st)) != FMCMC_OK) return rc;
    hipLaunchKernelGGL(pdv_init_kernel, per_point, dim3(PRED_T), 0, st, A, R);
    if (m->y) {
      A.slot0 = nprobs; A.nb = 1; A.pit = 1;
      if ((rc = pdv_launch_tiles<PDV_EVAL>(who, A, st)) != FMCMC_OK) return rc;
      A.pit = 0;
    }
  }
  for (int pass = 1; pass <= npasses && nprobs > 0; pass++) {
    A.pass = pass;
    for (int slot0 = 0; slot0 < nprobs; slot0 += PDV_BATCH) {
      A.slot0 = slot0;
      A.nb = nprobs - slot0 < PDV_BATCH ? nprobs - slot0 : PDV_BATCH;
      if ((rc = pdv_launch_tiles<PDV_EVAL>(who, A, st)) != FMCMC_OK) return rc;
      hipLaunchKernelGGL(pdv_step_kernel, dim3((unsigned)((A.n * A.nb + PRED_T - 1) / PRED_T)), dim3(PRED_T), 0, st, A, R);
    }
  }
  hipLaunchKernelGGL(pdv_finish_kernel, per_point, dim3(PRED_T), 0, st, A, point);
  hipLaunchKernelGGL(pdv_count_kernel, dim3(1), dim3(PRED_T), 0, st, A, total);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

}  // extern "C"
