// diag_predict.hpp — fitted values, predictions at new covariates and their credible bands for the two regression families from the
// kept rows where the sweep left them (the definition is INTEGRATION.md §2.2, the host restatement fmcmc_amd/summary.py:
// predict_host, the kernels, the scratch and the times DESIGN.md §5.10).  Included by summary.hip behind diag_pointwise.hpp; it
// reuses diag_waic.hpp's split of the draws into parts (waic_plan with n := the m points) and restates its tile evaluation, as
// diag_loo.hpp does, so that WAIC's and LOO's object code is not touched.
//
// The S' x m matrix eta[s][i] = b0_s + x_i . beta_s is never stored:
//   pred_draw_kernel     a thread a draw: the count of bad draws (a coefficient that is not finite, Gaussian: a sigma that is not
//                        > 0) and, Gaussian, sigma^2: a workgroup's sums into `work` (no atomics).
//   pred_total_kernel    one workgroup: those partials in index order, total = {S', bad draws, mean sigma^2, 0}.
//   pred_tile_kernel<., PRED_FOLD>   a workgroup = 64 points x one part of the draws, a wavefront = 16 points.  ceil(k' / 4)
//                        v_mfma_f64_16x16x4 form a 16 x 16 tile of eta (the B tile is Xn, ones for the intercept; no -y column);
//                        every lane folds its four elements into (count, mean, M2) of q (and, for the logistic mean, also of eta);
//                        the four lane groups of a point are merged in the order ((0 + 1) + 2) + 3 by Chan's update and one
//                        partial {mean q, M2 q, mean eta, M2 eta} per (part, point) goes to `work`.
//   pred_init_kernel, 8 x (pred_tile_kernel<., PRED_HIST>, pred_scan_kernel)   per batch of up to PRED_BATCH ranks: a
//                        most-significant-digit radix select over ALL draws for the exact keys (diag_common.hpp: key_of) of the
//                        order statistics the type-7 quantiles need, every pass re-evaluating the tiles.  Integer histograms in HBM;
//                        ranks of a point that share a prefix share one histogram; a lane sends a run of equal digits as one atomic.
//                        After the eighth pass a rank's prefix IS its order statistic: nothing is read back, ties need nothing.
//   pred_finish_kernel   a thread a point: the parts in part order, then point[i] = {mean, sd, sd_pred, mean of eta, quantiles}.
// The plan is a function of (chains, N, m, nprobs) alone; counts are integers; every floating sum has a fixed order: the same bits
// on every call, wherever the window sits.  Nothing here writes `samples` or the model.
#pragma once

namespace {

constexpr int PRED_T = 256;             // threads of every kernel here
constexpr int PRED_MAX_PROBS = 16;      // as fmcmc_summary_dev
constexpr int PRED_MAX_RANKS = 2 * PRED_MAX_PROBS;
constexpr int PRED_BATCH = 8;           // ranks whose histograms (1 KB each per point) live in `work` at a time
enum { PRED_FOLD = 0, PRED_HIST = 1 };
enum { PRED_LINPRED = 0, PRED_EPRED = 1 };

struct PredPlan {
  int gauss, ic, ncoef, nq, sig, nprobs, nslots, nbatch;   // sig: q = the logistic map of eta; nslots = 2 nprobs state slots
  long long T, U, upp, nparts, tiles, nblk, partcap;
  long long off_s2, off_part, off_state, off_hist, len;     // `work`: bad counts [nblk] at 0, sigma^2 sums [nblk], the partials
};                                                          // [partcap][m][4], the state [m][nslots][2], the histograms

// The distinct 0-based ranks of the call, ascending, and for every prob the slots of its two neighbours.
struct PredRanks {
  unsigned long long rank[PRED_MAX_RANKS];
  double h[PRED_MAX_PROBS];
  int lo[PRED_MAX_PROBS], hi[PRED_MAX_PROBS], between[PRED_MAX_PROBS];
  int nr;
};

inline int pred_family_k(const fmcmc_model* m) {
  return (m->intercept ? 1 : 0) + m->p + (m->family == FMCMC_FAM_GAUSSIAN_LINREG ? 1 : 0);
}

// WAIC's split with n := m (units of 16 rows of one chain, upp units a part).  The partials are laid out for partcap =
// min(256, ceil(U / 32)) >= nparts parts, whatever m, so that the length of `work` never shrinks when N, m or nprobs grow.
inline PredPlan pred_plan(const fmcmc_model* m, long long cpg, long long N, int kind, int nprobs) {
  const WaicPlan W = waic_plan(m, 1, cpg, N);
  PredPlan P;
  P.gauss = m->family == FMCMC_FAM_GAUSSIAN_LINREG;
  P.ic = m->intercept ? 1 : 0;
  P.ncoef = P.ic + m->p;
  P.nq = (P.ncoef + 3) / 4;
  P.sig = !P.gauss && kind == PRED_EPRED;
  P.nprobs = nprobs;
  P.nslots = 2 * nprobs;
  P.nbatch = P.nslots < PRED_BATCH ? P.nslots : PRED_BATCH;
  P.T = W.T; P.U = W.U; P.upp = W.upp; P.nparts = W.nparts; P.tiles = W.tiles; P.nblk = W.nblk;
  const long long most = (P.U + WAIC_PART_ROWS / 16 - 1) / (WAIC_PART_ROWS / 16);
  P.partcap = most < WAIC_MAX_PARTS_SMALL ? most : WAIC_MAX_PARTS_SMALL;
  P.off_s2 = P.nblk;
  P.off_part = 2 * P.nblk;
  P.off_state = P.off_part + P.partcap * m->n * 4;
  P.off_hist = P.off_state + m->n * P.nslots * 2;
  P.len = P.off_hist + m->n * P.nbatch * 128;
  return P;
}

struct PredArgs {
  const double* samples; const double* X; double* work;
  long long S, row0, N, n, cpg;
  int k, pass, slot0, nb;               // the batch of a select pass: the slots [slot0, slot0 + nb)
  PredPlan P;
};

// {count, mean, M2} of a set of draws, for one point; a, then b by Chan, Golub and LeVeque's update, as waic_merge does: an
// empty side leaves the other as it is, bit for bit.
struct PredAcc { double cnt, mean, M2; };

__device__ __forceinline__ PredAcc pred_merge(const PredAcc& a, const PredAcc& b) {
  if (b.cnt == 0.0) return a;
  if (a.cnt == 0.0) return b;
  PredAcc o;
  o.cnt = a.cnt + b.cnt;
  const double delta = b.mean - a.mean;
  o.mean = a.mean + delta * (b.cnt / o.cnt);
  o.M2 = (a.M2 + b.M2) + delta * delta * (a.cnt * b.cnt / o.cnt);
  return o;
}

// 1 / (1 + exp(-eta)) in the branch form of the family's evaluation: exp of a non-positive argument only.
__device__ __forceinline__ double pred_expit(double eta) {
  const double e = fmh_exp(-fmh_abs(eta));
  return eta >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// A lane's shifted sums (K the first value it saw) as {count, mean, M2}.
__device__ __forceinline__ PredAcc pred_lane_acc(int cnt, double K, double sd, double sdd) {
  PredAcc a;
  a.cnt = (double)cnt;
  a.mean = cnt ? K + sd / (double)cnt : 0.0;
  a.M2 = cnt ? sdd - sd * sd / (double)cnt : 0.0;
  if (a.M2 < 0.0) a.M2 = 0.0;                        // (a rounding of the difference; a NaN stays)
  return a;
}

// The four lane groups of a point, ((0 + 1) + 2) + 3.
__device__ __forceinline__ PredAcc pred_merge_groups(const PredAcc& mine, int col) {
  PredAcc acc4;
#pragma unroll
  for (int gs = 0; gs < 4; gs++) {
    const int src = col + 16 * gs;
    PredAcc o;
    o.cnt = __shfl(mine.cnt, src, 64); o.mean = __shfl(mine.mean, src, 64); o.M2 = __shfl(mine.M2, src, 64);
    acc4 = gs == 0 ? o : pred_merge(acc4, o);
  }
  return acc4;
}

__global__ __launch_bounds__(PRED_T) void pred_draw_kernel(PredArgs A) {
  __shared__ double red[PRED_T / 64];
  const long long e = (long long)blockIdx.x * PRED_T + threadIdx.x;
  double bad = 0.0, s2 = 0.0;
  if (e < A.cpg * A.N) {
    const long long c = e / A.N, row = e % A.N;
    const double* __restrict__ th = A.samples + c * A.k * A.S + A.row0 + row;
    int nf = 0;
    for (int j = 0; j < A.k; j++) nf |= !fmh_isfinite(th[(long long)j * A.S]);
    if (A.P.gauss) {
      const double sigma = th[(long long)(A.k - 1) * A.S];
      nf |= !(sigma > 0.0);
      s2 = sigma * sigma;
    }
    bad = nf ? 1.0 : 0.0;
  }
  const double tb = block_sum<PRED_T / 64>(bad, red);
  const double ts = block_sum<PRED_T / 64>(s2, red);
  if (threadIdx.x == 0) { A.work[blockIdx.x] = tb; A.work[A.P.off_s2 + blockIdx.x] = ts; }
}

__global__ __launch_bounds__(PRED_T) void pred_total_kernel(PredArgs A, double* __restrict__ total) {
  __shared__ double red[PRED_T / 64];
  double bad = 0.0, s2 = 0.0;
  for (long long i = threadIdx.x; i < A.P.nblk; i += PRED_T) { bad += A.work[i]; s2 += A.work[A.P.off_s2 + i]; }
  bad = block_sum<PRED_T / 64>(bad, red);
  s2 = block_sum<PRED_T / 64>(s2, red);
  if (threadIdx.x == 0) {
    const double draws = (double)(A.cpg * A.N);
    total[0] = draws; total[1] = bad; total[2] = A.P.gauss ? s2 / draws : fmh_nan(); total[3] = 0.0;
  }
}

// The tile evaluation of waic_tile_kernel (diag_waic.hpp) without the -y column and with another use of every eta.  NQR: the
// steps of four operand columns whose B values a lane keeps in registers; 0: the B tile lives in LDS.
template <int NQR, int MODE>
__global__ __launch_bounds__(PRED_T) void pred_tile_kernel(PredArgs A) {
  constexpr bool LDSB = NQR == 0;
  constexpr int NB = NQR ? NQR : 1;
  extern __shared__ double s_b[];                    // LDSB: [nq][4 wavefronts][64 lanes], a lane reads what it wrote
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, col = lane & 15;
  const PredPlan& P = A.P;
  const long long tile = blockIdx.x, part = blockIdx.y;
  const long long obs = tile * 64 + wave * 16 + col;
  const bool obs_ok = obs < A.n;
  const int nq = P.nq, ncoef = P.ncoef;

  // the B operand of lane l, step q: row 4 q + l / 16 (a coefficient's covariate, ones for the intercept), column = the point
  // l % 16 of the wavefront; zeros beyond m and beyond the columns
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

  // PRED_HIST: the prefixes of the batch's ranks of my point; a slot leads when its prefix differs from the slot before it (the
  // ranks ascend, so equal prefixes are neighbours); a led slot's keys are counted in its leader's histogram
  unsigned long long pre[PRED_BATCH];
  unsigned int run_bin[PRED_BATCH], run_cnt[PRED_BATCH];
  unsigned int* __restrict__ hist = nullptr;
  if (MODE == PRED_HIST) {
    const unsigned long long* __restrict__ st =
        reinterpret_cast<const unsigned long long*>(A.work + P.off_state) + ((obs_ok ? obs : 0) * P.nslots + A.slot0) * 2;
    hist = reinterpret_cast<unsigned int*>(A.work + P.off_hist) + (obs_ok ? obs : 0) * P.nbatch * 256;
#pragma unroll
    for (int s = 0; s < PRED_BATCH; s++) {
      pre[s] = s < A.nb ? st[2 * s] : 0ull;
      run_bin[s] = 0u; run_cnt[s] = 0u;
    }
  }
  unsigned int leads = 0u;
  if (MODE == PRED_HIST) {
#pragma unroll
    for (int s = 0; s < PRED_BATCH; s++)
      if (s < A.nb && (s == 0 || pre[s] != pre[s - 1])) leads |= 1u << s;
  }

  const long long u0 = part * P.upp, u1 = u0 + P.upp < P.U ? u0 + P.upp : P.U;
  const double* __restrict__ smp = A.samples + A.row0;
  double K = 0.0, sd = 0.0, sdd = 0.0, K2 = 0.0, sd2 = 0.0, sdd2 = 0.0;
  int cnt = 0;
  long long c = u0 / P.T, t = u0 - c * P.T;           // unit u = c T + t, followed without a division a tile
  for (long long u = u0; u < u1; u++, t++) {
    if (t == P.T) { t = 0; c++; }
    const long long rb = 16 * t;
    const int valid = A.N - rb < 16 ? (int)(A.N - rb) : 16;
    // the A operand of lane l, step q: draw l % 16 of the tile, column 4 q + l / 16: 16 consecutive doubles of a column
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
      const double eta = acc[r];
      if (MODE == PRED_FOLD) {
        const double q = P.sig ? pred_expit(eta) : eta;
        if (cnt == 0) { K = q; K2 = eta; }
        cnt++;
        const double d = q - K;
        sd += d;
        sdd = fmh_fma(d, d, sdd);
        if (P.sig) {
          const double d2 = eta - K2;
          sd2 += d2;
          sdd2 = fmh_fma(d2, d2, sdd2);
        }
      } else {
        const unsigned long long key = key_of(eta);
        const unsigned long long high = radix_high(key, A.pass);
        const unsigned int digit = radix_digit(key, A.pass);
#pragma unroll
        for (int s = 0; s < PRED_BATCH; s++) {
          if (((leads >> s) & 1u) && high == pre[s]) {
            if (run_cnt[s] && run_bin[s] != digit) { atomicAdd(&hist[s * 256 + run_bin[s]], run_cnt[s]); run_cnt[s] = 0u; }
            run_bin[s] = digit;
            run_cnt[s]++;
          }
        }
      }
    }
  }
  if (MODE == PRED_HIST) {
#pragma unroll
    for (int s = 0; s < PRED_BATCH; s++)
      if (run_cnt[s]) atomicAdd(&hist[s * 256 + run_bin[s]], run_cnt[s]);
  } else {
    const PredAcc q4 = pred_merge_groups(pred_lane_acc(cnt, K, sd, sdd), col);
    PredAcc e4 = q4;
    if (P.sig) e4 = pred_merge_groups(pred_lane_acc(cnt, K2, sd2, sdd2), col);
    if (kk == 0 && obs_ok) {
      double* o = A.work + P.off_part + (part * A.n + obs) * 4;
      o[0] = q4.mean; o[1] = q4.M2; o[2] = e4.mean; o[3] = e4.M2;
    }
  }
}

// A workgroup a point: the batch's slots start at prefix 0 with their ranks, the batch's histograms at zero.
__global__ __launch_bounds__(PRED_T) void pred_init_kernel(PredArgs A, PredRanks R) {
  const PredPlan& P = A.P;
  const long long obs = blockIdx.x;
  const int tid = threadIdx.x;
  unsigned long long* __restrict__ st = reinterpret_cast<unsigned long long*>(A.work + P.off_state) + (obs * P.nslots + A.slot0) * 2;
  unsigned int* __restrict__ hist = reinterpret_cast<unsigned int*>(A.work + P.off_hist) + obs * P.nbatch * 256;
  for (int s = 0; s < A.nb; s++) hist[s * 256 + tid] = 0u;
  if (tid < A.nb) { st[2 * tid] = 0ull; st[2 * tid + 1] = R.rank[A.slot0 + tid]; }
}

// Pass A.pass of the select, a workgroup a point, a thread a bin: for every leading slot the inclusive sums of its histogram
// (which is zeroed for the next pass); every slot it leads takes the bin that holds its remaining rank.
__global__ __launch_bounds__(PRED_T) void pred_scan_kernel(PredArgs A) {
  __shared__ unsigned long long s_pre[PRED_BATCH], s_rem[PRED_BATCH], s_npre[PRED_BATCH], s_nrem[PRED_BATCH];
  __shared__ unsigned int s_w[PRED_T / 64];
  const PredPlan& P = A.P;
  const long long obs = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* __restrict__ st = reinterpret_cast<unsigned long long*>(A.work + P.off_state) + (obs * P.nslots + A.slot0) * 2;
  unsigned int* __restrict__ hist = reinterpret_cast<unsigned int*>(A.work + P.off_hist) + obs * P.nbatch * 256;
  if (tid < A.nb) {
    s_pre[tid] = st[2 * tid]; s_rem[tid] = st[2 * tid + 1];
    s_npre[tid] = st[2 * tid] << 8; s_nrem[tid] = st[2 * tid + 1];
  }
  __syncthreads();
  for (int r = 0; r < A.nb; r++) {
    if (r > 0 && s_pre[r] == s_pre[r - 1]) continue;  // (led by an earlier slot; the same for every thread)
    const unsigned int cbin = hist[r * 256 + tid];
    hist[r * 256 + tid] = 0u;
    unsigned int incl = cbin;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    unsigned long long base = 0ull;
    for (int w = 0; w < wave; w++) base += s_w[w];
    const unsigned long long hi = base + incl, lo = hi - cbin;
    for (int s = r; s < A.nb && s_pre[s] == s_pre[r]; s++) {
      const unsigned long long rem = s_rem[s];
      if (lo <= rem && rem < hi) { s_npre[s] = (s_pre[s] << 8) | (unsigned long long)tid; s_nrem[s] = rem - lo; }
    }
    __syncthreads();
  }
  if (tid < A.nb) { st[2 * tid] = s_npre[tid]; st[2 * tid + 1] = s_nrem[tid]; }
}

// A thread a point: the parts in part order; the quantiles in the arithmetic of summary.py: type7_quantiles (two rounded
// products, one rounded sum), on the order statistics mapped first where q is the logistic map of eta.
__global__ __launch_bounds__(PRED_T) void pred_finish_kernel(PredArgs A, PredRanks R, const double* __restrict__ total,
                                                             double* __restrict__ point) {
  const PredPlan& P = A.P;
  const long long obs = (long long)blockIdx.x * PRED_T + threadIdx.x;
  if (obs >= A.n) return;
  PredAcc q, e;
  for (long long part = 0; part < P.nparts; part++) {
    const long long u0 = part * P.upp, u1 = u0 + P.upp < P.U ? u0 + P.upp : P.U;
    const double* __restrict__ o = A.work + P.off_part + (part * A.n + obs) * 4;
    PredAcc bq, be;
    bq.cnt = be.cnt = (double)waic_unit_rows(u0, u1, P.T, A.N);
    bq.mean = o[0]; bq.M2 = o[1]; be.mean = o[2]; be.M2 = o[3];
    q = part == 0 ? bq : pred_merge(q, bq);
    e = part == 0 ? be : pred_merge(e, be);
  }
  const double draws = (double)(A.cpg * A.N);
  double* out = point + obs * (4 + P.nprobs);
  out[0] = q.mean;
  out[1] = fmh_sqrt(q.M2 / (draws - 1.0));
  out[2] = P.gauss ? fmh_sqrt(e.M2 / (draws - 1.0) + total[2]) : fmh_nan();
  out[3] = e.mean;
  const unsigned long long* __restrict__ st = reinterpret_cast<const unsigned long long*>(A.work + P.off_state) + obs * P.nslots * 2;
  for (int i = 0; i < P.nprobs; i++) {
    double xlo = value_of(st[2 * R.lo[i]]), xhi = value_of(st[2 * R.hi[i]]);
    if (P.sig) { xlo = pred_expit(xlo); xhi = pred_expit(xhi); }
    out[4 + i] = (R.between[i] && xhi != xlo) ? __dadd_rn(__dmul_rn(1.0 - R.h[i], xlo), __dmul_rn(R.h[i], xhi)) : xlo;
  }
}

// Every check of the two entries, before any device call.
inline int pred_check(const char* who, const fmcmc_model* m, int64_t cpg, int32_t k, int64_t S, int64_t row0, int64_t N,
                      int32_t kind, const double* probs, int32_t nprobs) {
  if (!m) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (m->family == FMCMC_FAM_IID_NORMAL)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: iid_normal has no covariates to predict at; its mean and sd are fmcmc_summary_dev's", who);
  if (m->family != FMCMC_FAM_GAUSSIAN_LINREG && m->family != FMCMC_FAM_LOGISTIC)
    return fail(FMCMC_ERR_ARG, "%s: unknown family %d", who, (int)m->family);
  if (m->n < 1 || m->p < 0 || (m->p > 0 && !m->X))
    return fail(FMCMC_ERR_ARG, "%s: the model needs n >= 1 points and X for its p >= 0 columns", who);
  if ((long long)m->p + 2 > 0x7fffffffLL || pred_family_k(m) < 1 || pred_family_k(m) > FMCMC_MAX_K)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: the family has %lld parameters; supported are 1 .. %d", who,
                (long long)m->p + (m->intercept ? 1 : 0) + (m->family == FMCMC_FAM_GAUSSIAN_LINREG), FMCMC_MAX_K);
  if (k != pred_family_k(m))
    return fail(FMCMC_ERR_ARG, "%s: k = %d, but the family has %d parameters", who, (int)k, pred_family_k(m));
  if (cpg < 1) return fail(FMCMC_ERR_ARG, "%s: nchains = %lld: at least 1 is needed", who, (long long)cpg);
  if (N < 1 || row0 < 0 || row0 + N > S)
    return fail(FMCMC_ERR_ARG, "%s: the window [%lld, %lld) is outside the %lld rows of a chain", who, (long long)row0,
                (long long)(row0 + N), (long long)S);
  if (cpg > 0x7fffffffLL || N > 0x7fffffffLL / cpg)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld chains x %lld rows exceed the 2^31 - 1 draws of one call", who, (long long)cpg,
                (long long)N);
  if (cpg * N < 2) return fail(FMCMC_ERR_ARG, "%s: S = %lld draw: a prediction needs at least 2", who, (long long)(cpg * N));
  if (kind != PRED_LINPRED && kind != PRED_EPRED)
    return fail(FMCMC_ERR_ARG, "%s: kind = %d; 0 (linpred) or 1 (epred)", who, (int)kind);
  if (nprobs < 0 || nprobs > PRED_MAX_PROBS)
    return fail(FMCMC_ERR_ARG, "%s: nprobs = %d outside [0, %d]", who, (int)nprobs, PRED_MAX_PROBS);
  if (nprobs > 0 && probs)
    for (int i = 0; i < nprobs; i++)
      if (!(probs[i] >= 0.0 && probs[i] <= 1.0))
        return fail(FMCMC_ERR_ARG, "%s: probs[%d] = %g is not a probability", who, i, probs[i]);
  if (m->n > 0x7fffffffLL) return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld points exceed one launch", who, (long long)m->n);
  return FMCMC_OK;
}

inline PredRanks pred_ranks(long long draws, const double* probs, int nprobs) {
  PredRanks R = {};
  long long lo[PRED_MAX_PROBS], hi[PRED_MAX_PROBS];
  for (int i = 0; i < nprobs; i++) {
    const Type7 r = type7_ranks(draws, probs[i]);
    lo[i] = r.lo; hi[i] = r.hi; R.between[i] = r.between; R.h[i] = r.h;
  }
  for (int i = 0; i < nprobs; i++) {                 // the distinct ranks, ascending (an insertion sort of at most 32)
    const long long both[2] = {lo[i], hi[i]};
    for (int w = 0; w < 2; w++) {
      const unsigned long long v = (unsigned long long)both[w];
      int at = 0;
      while (at < R.nr && R.rank[at] < v) at++;
      if (at < R.nr && R.rank[at] == v) continue;
      for (int j = R.nr; j > at; j--) R.rank[j] = R.rank[j - 1];
      R.rank[at] = v;
      R.nr++;
    }
  }
  for (int i = 0; i < nprobs; i++)
    for (int s = 0; s < R.nr; s++) {
      if (R.rank[s] == (unsigned long long)lo[i]) R.lo[i] = s;
      if (R.rank[s] == (unsigned long long)hi[i]) R.hi[i] = s;
    }
  return R;
}

template <int MODE>
int pred_launch_tiles(const char* who, const PredArgs& A, hipStream_t st) {
  const PredPlan& P = A.P;
  const dim3 grid((unsigned)P.tiles, (unsigned)P.nparts);
  if (P.nq <= 2) {                                   // (k' <= 8: the headline regression)
    hipLaunchKernelGGL((pred_tile_kernel<2, MODE>), grid, dim3(PRED_T), 0, st, A);
  } else if (P.nq <= 4) {
    hipLaunchKernelGGL((pred_tile_kernel<4, MODE>), grid, dim3(PRED_T), 0, st, A);
  } else if (P.nq <= WAIC_REG_Q) {
    hipLaunchKernelGGL((pred_tile_kernel<WAIC_REG_Q, MODE>), grid, dim3(PRED_T), 0, st, A);
  } else {
    const size_t lds = (size_t)P.nq * PRED_T * sizeof(double);
    const int rc = allow_lds(who, pred_tile_kernel<0, MODE>, lds);
    if (rc != FMCMC_OK) return rc;
    hipLaunchKernelGGL((pred_tile_kernel<0, MODE>), grid, dim3(PRED_T), lds, st, A);
  }
  return FMCMC_OK;
}

}  // namespace

extern "C" {

int64_t fmcmc_predict_work_len(const fmcmc_model* m, int64_t nchains, int64_t N, int32_t nprobs) {
  if (!m) return 0;
  if (pred_check("fmcmc_predict_work_len", m, nchains, pred_family_k(m), N, 0, N, PRED_LINPRED, nullptr, nprobs) != FMCMC_OK)
    return 0;
  return pred_plan(m, nchains, N, PRED_LINPRED, nprobs).len;
}

int fmcmc_predict_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0,
                      int64_t N, int32_t kind, const double* probs, int32_t nprobs, double* work, double* point, double* total,
                      void* hip_stream) {
  const char* who = "fmcmc_predict_dev";
  if (!m || !samples || !work || !point || !total || (nprobs > 0 && !probs)) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = pred_check(who, m, nchains, k, S, row0, N, kind, probs, nprobs);
  if (rc != FMCMC_OK) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  PredArgs A;
  A.samples = samples; A.X = m->X; A.work = work;
  A.S = S; A.row0 = row0; A.N = N; A.n = m->n; A.cpg = nchains;
  A.k = k; A.pass = 0; A.slot0 = 0; A.nb = 0;
  A.P = pred_plan(m, nchains, N, kind, nprobs);
  const PredPlan& P = A.P;
  const PredRanks R = pred_ranks(nchains * N, probs, nprobs);
  hipLaunchKernelGGL(pred_draw_kernel, dim3((unsigned)P.nblk), dim3(PRED_T), 0, st, A);
  hipLaunchKernelGGL(pred_total_kernel, dim3(1), dim3(PRED_T), 0, st, A, total);
  if ((rc = pred_launch_tiles<PRED_FOLD>(who, A, st)) != FMCMC_OK) return rc;
  for (int slot0 = 0; slot0 < R.nr; slot0 += PRED_BATCH) {
    A.slot0 = slot0;
    A.nb = R.nr - slot0 < PRED_BATCH ? R.nr - slot0 : PRED_BATCH;
    hipLaunchKernelGGL(pred_init_kernel, dim3((unsigned)A.n), dim3(PRED_T), 0, st, A, R);
    for (int pass = 0; pass < 8; pass++) {
      A.pass = pass;
      if ((rc = pred_launch_tiles<PRED_HIST>(who, A, st)) != FMCMC_OK) return rc;
      hipLaunchKernelGGL(pred_scan_kernel, dim3((unsigned)A.n), dim3(PRED_T), 0, st, A);
    }
  }
  hipLaunchKernelGGL(pred_finish_kernel, dim3((unsigned)((A.n + PRED_T - 1) / PRED_T)), dim3(PRED_T), 0, st, A, R, total, point);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

}  // extern "C"
