// diag_waic.hpp — the widely applicable information criterion (Watanabe 2010; Gelman, Hwang, Vehtari 2014; loo::waic) of the
// three closed-form families from the kept rows where the sweep left them (the definition is INTEGRATION.md §2.2, the host
// restatement fmcmc_amd/summary.py: waic_host, the kernel description and the error bound DESIGN.md §5.10).  Included by
// summary.hip alone, behind its reductions (block_sum).
//
// The pointwise log-likelihood l[s][i] = log p(y_i | theta_s) of S = C N draws and n observations is never stored:
//   waic_draw_kernel    a thread a draw: the count of bad draws (a coefficient that is not finite, a sigma that is not > 0), a
//                       workgroup's count into `work` (integers, no atomics); the Gaussian families also leave
//                       a[s] = -(log sigma + ln sqrt(2 pi)) and w[s] = 0.5 / sigma^2 there.
//   waic_tile_kernel    a workgroup = 64 observations x one part of the draws; a wavefront = 16 observations.  The wavefront
//                       walks its part 16 rows of one chain at a time: ceil(k' / 4) v_mfma_f64_16x16x4 form the 16 x 16 tile of
//                       eta (logistic) or eta - y (Gaussian: the operand has a column of ones against -y_i in the place of
//                       sigma), every lane turns its four elements into l and folds them into the accumulators of its one
//                       observation: the running maximum M with E = sum exp(l - M), and the sums of d and d^2, d = l - K, K the
//                       first l the lane saw.  At the end of the part the four lane groups of an observation are merged in the
//                       order ((0 + 1) + 2) + 3 (log-sum-exp for (M, E), Chan's update for (count, mean, M2)) and one partial
//                       {M, E, mean, M2} per (part, observation) goes to `work`.  The B tile (the observations' covariates) is
//                       loaded once per workgroup: into registers up to 64 operand columns (three forms, for up to 2, 4 and
//                       16 steps of four columns: 74, 86 and 157 VGPRs), into LDS beyond, up to FMCMC_MAX_K.
//   waic_merge_kernel   a thread an observation: the parts in part order, then point[i] = {elpd_i, p_waic_i, lppd_i, mean_i}.
//   waic_total_kernel   a workgroup a group: the sums over the n rows (a thread the rows t, t + 256, ..., then block_sum), the
//                       variances behind the standard errors in a second pass, the counts.
// The split of the draws into parts (waic_plan) is a function of (chains per group, N, n <= 1024) alone, so every sum has a
// shape that the launch, the device and the number of groups do not change.  Nothing here writes `samples` or the model.
#pragma once

namespace {

constexpr int WAIC_PART_ROWS = 512;     // the least rows of a part (32 tiles of 16 rows)
constexpr int WAIC_MAX_PARTS = 64;      // partials per observation ...
constexpr int WAIC_MAX_PARTS_SMALL = 256;   // ... and while n <= WAIC_SMALL_N (few observation tiles: the parts fill the device)
constexpr int WAIC_SMALL_N = 1024;
constexpr int WAIC_REG_Q = 16;          // operand columns / 4 that the B tile keeps in registers (64 columns); beyond: LDS
constexpr int WAIC_T = 256;             // threads of every kernel here

typedef double waic_d4 __attribute__((ext_vector_type(4)));

struct WaicPlan {
  int gauss, ic, ncoef, onecol, nq;     // columns [0, ncoef) of a draw are coefficients, column onecol is read as 1.0 (against -y)
  long long T, U, upp, nparts, tiles, nblk;     // tiles of 16 rows a chain, units = cpg T, units a part, parts, tiles of 64 obs
  long long off_w, off_bad, off_part, len;      // `work`: a at 0, w, the bad counts [G][nblk], the partials [G][nparts][n][4]
};

inline int waic_family_k(const fmcmc_model* m) {
  const int ic = m->intercept ? 1 : 0;
  if (m->family == FMCMC_FAM_GAUSSIAN_LINREG) return ic + m->p + 1;
  if (m->family == FMCMC_FAM_LOGISTIC) return ic + m->p;
  return 2;
}

// The split: unit u = c T + t is tile t (rows [16 t, 16 t + 16) of the window) of chain c of the group; part j takes the units
// [j upp, (j + 1) upp).  upp = max(WAIC_PART_ROWS / 16, ceil(U / cap)), cap = 256 while n <= 1024, else 64.
inline WaicPlan waic_plan(const fmcmc_model* m, long long G, long long cpg, long long N) {
  WaicPlan P;
  P.gauss = m->family != FMCMC_FAM_LOGISTIC;
  P.ic = m->family == FMCMC_FAM_IID_NORMAL ? 1 : (m->intercept ? 1 : 0);
  const int k = waic_family_k(m);
  P.ncoef = P.gauss ? k - 1 : k;
  P.onecol = P.gauss ? k - 1 : -1;
  P.nq = (k + 3) / 4;
  P.T = (N + 15) / 16;
  P.U = cpg * P.T;
  const long long cap = m->n <= WAIC_SMALL_N ? WAIC_MAX_PARTS_SMALL : WAIC_MAX_PARTS;
  const long long need = (P.U + cap - 1) / cap;
  P.upp = need > WAIC_PART_ROWS / 16 ? need : WAIC_PART_ROWS / 16;
  P.nparts = (P.U + P.upp - 1) / P.upp;
  P.tiles = (m->n + 63) / 64;
  P.nblk = (cpg * N + WAIC_T - 1) / WAIC_T;
  const long long draws = P.gauss ? G * cpg * N : 0;
  P.off_w = draws;
  P.off_bad = 2 * draws;
  P.off_part = P.off_bad + G * P.nblk;
  P.len = P.off_part + G * P.nparts * m->n * 4;
  return P;
}

// The rows of the units [u0, u1): 16 each but for the last tile of a chain.
__device__ __forceinline__ long long waic_unit_rows(long long u0, long long u1, long long T, long long N) {
  return 16 * (u1 - u0) - (u1 / T - u0 / T) * (16 * T - N);
}

struct WaicArgs {
  const double* samples; const double* X; const double* y; const int* active; double* work;
  long long x_stride, y_stride, S, row0, N, n, cpg;
  int k;
  WaicPlan P;
};

// {count, M, E, mean, M2} of a set of draws, for one observation.
struct WaicAcc { double cnt, M, E, mean, M2; };

// a, then b: log-sum-exp for (M, E), Chan, Golub and LeVeque's update for (count, mean, M2).  An empty side leaves the other as
// it is, bit for bit.
__device__ __forceinline__ WaicAcc waic_merge(const WaicAcc& a, const WaicAcc& b) {
  if (b.cnt == 0.0) return a;
  if (a.cnt == 0.0) return b;
  WaicAcc o;
  o.cnt = a.cnt + b.cnt;
  o.M = a.M > b.M ? a.M : b.M;
  o.E = fmh_fma(a.E, fmh_exp(a.M - o.M), b.E * fmh_exp(b.M - o.M));
  const double delta = b.mean - a.mean;
  o.mean = a.mean + delta * (b.cnt / o.cnt);
  o.M2 = (a.M2 + b.M2) + delta * delta * (a.cnt * b.cnt / o.cnt);
  return o;
}

__global__ __launch_bounds__(WAIC_T) void waic_draw_kernel(WaicArgs A) {
  __shared__ double red[WAIC_T / 64];
  const long long g = blockIdx.y;
  if (A.active && !A.active[g]) return;
  const long long e = (long long)blockIdx.x * WAIC_T + threadIdx.x;
  double bad = 0.0;
  if (e < A.cpg * A.N) {
    const long long c = g * A.cpg + e / A.N, row = e % A.N;
    const double* __restrict__ th = A.samples + c * A.k * A.S + A.row0 + row;
    int nf = 0;
    for (int j = 0; j < A.k; j++) nf |= !fmh_isfinite(th[(long long)j * A.S]);
    if (A.P.gauss) {
      const double sigma = th[(long long)(A.k - 1) * A.S];
      nf |= !(sigma > 0.0);
      A.work[c * A.N + row] = -(fmh_log(sigma) + FMH_LN_SQRT_2PI);
      A.work[A.P.off_w + c * A.N + row] = 0.5 / (sigma * sigma);
    }
    bad = nf ? 1.0 : 0.0;
  }
  const double total = block_sum<WAIC_T / 64>(bad, red);
  if (threadIdx.x == 0) A.work[A.P.off_bad + g * A.P.nblk + blockIdx.x] = total;
}

// NQR: the steps of four operand columns whose B values a lane keeps in registers (nq <= NQR); 0: the B tile lives in LDS.
template <int NQR>
__global__ __launch_bounds__(WAIC_T) void waic_tile_kernel(WaicArgs A) {
  constexpr bool LDSB = NQR == 0;
  constexpr int NB = NQR ? NQR : 1;
  extern __shared__ double s_b[];                    // LDSB: [nq][4 wavefronts][64 lanes], a lane reads what it wrote
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, col = lane & 15;
  const WaicPlan& P = A.P;
  const long long g = blockIdx.x / P.tiles, tile = blockIdx.x - g * P.tiles, part = blockIdx.y;
  if (A.active && !A.active[g]) return;
  const long long obs = tile * 64 + wave * 16 + col;
  const bool obs_ok = obs < A.n;
  const double* __restrict__ X = A.X + g * A.x_stride;
  const double* __restrict__ y = A.y + g * A.y_stride;
  const int nq = P.nq, ncoef = P.ncoef, onecol = P.onecol;

  // the B operand of lane l, step q: row 4 q + l / 16 (a coefficient's covariate, ones for the intercept, -y_i against the
  // column of ones), column = the observation l % 16 of the wavefront; zeros beyond n and beyond the columns
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

  const long long u0 = part * P.upp, u1 = u0 + P.upp < P.U ? u0 + P.upp : P.U;
  const double* __restrict__ smp = A.samples + g * A.cpg * A.k * A.S + A.row0;
  const double* __restrict__ av = A.work + g * A.cpg * A.N;
  const double* __restrict__ wv = av + P.off_w;
  double M = -fmh_inf(), E = 0.0, K = 0.0, sd = 0.0, sdd = 0.0;
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
    // D register r of lane l is draw 4 r + l / 16, observation l % 16
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int rr = 4 * r + kk;
      if (rr < valid && obs_ok) {
        const double eta = acc[r];
        double l;
        if (P.gauss) {
          const long long di = c * A.N + rb + rr;
          l = fmh_fma(-wv[di], eta * eta, av[di]);
        } else {
          const double ts = ypos ? eta : -eta;
          l = (ts < 0.0 ? ts : 0.0) - fmh_log1p(fmh_exp(-fmh_abs(ts)));
        }
        if (cnt == 0) K = l;
        cnt++;
        const double d = l - K;
        sd += d;
        sdd = fmh_fma(d, d, sdd);
        const double x = l - M, ex = fmh_exp(-fmh_abs(x));
        if (x > 0.0) { E = fmh_fma(E, ex, 1.0); M = l; }
        else E += ex;
      }
    }
  }
  WaicAcc mine;
  mine.cnt = (double)cnt; mine.M = M; mine.E = E;
  mine.mean = cnt ? K + sd / (double)cnt : 0.0;
  mine.M2 = cnt ? sdd - sd * sd / (double)cnt : 0.0;
  if (mine.M2 < 0.0) mine.M2 = 0.0;                  // (a rounding of the difference; a NaN stays)
  WaicAcc acc4;
#pragma unroll
  for (int gs = 0; gs < 4; gs++) {
    const int src = col + 16 * gs;
    WaicAcc o;
    o.cnt = __shfl(mine.cnt, src, 64); o.M = __shfl(mine.M, src, 64); o.E = __shfl(mine.E, src, 64);
    o.mean = __shfl(mine.mean, src, 64); o.M2 = __shfl(mine.M2, src, 64);
    acc4 = gs == 0 ? o : waic_merge(acc4, o);
  }
  if (kk == 0 && obs_ok) {
    double* o = A.work + P.off_part + ((g * P.nparts + part) * A.n + obs) * 4;
    o[0] = acc4.M; o[1] = acc4.E; o[2] = acc4.mean; o[3] = acc4.M2;
  }
}

__global__ __launch_bounds__(WAIC_T) void waic_merge_kernel(WaicArgs A, double* __restrict__ point) {
  const WaicPlan& P = A.P;
  const long long g = blockIdx.y, obs = (long long)blockIdx.x * WAIC_T + threadIdx.x;
  if (A.active && !A.active[g]) return;
  if (obs >= A.n) return;
  WaicAcc acc;
  for (long long part = 0; part < P.nparts; part++) {
    const long long u0 = part * P.upp, u1 = u0 + P.upp < P.U ? u0 + P.upp : P.U;
    const double* __restrict__ o = A.work + P.off_part + ((g * P.nparts + part) * A.n + obs) * 4;
    WaicAcc b;
    b.cnt = (double)waic_unit_rows(u0, u1, P.T, A.N); b.M = o[0]; b.E = o[1]; b.mean = o[2]; b.M2 = o[3];
    acc = part == 0 ? b : waic_merge(acc, b);
  }
  const double draws = (double)(A.cpg * A.N);
  const double lppd = acc.M + fmh_log(acc.E / draws), pw = acc.M2 / (draws - 1.0);
  double* out = point + (g * A.n + obs) * 4;
  out[0] = lppd - pw; out[1] = pw; out[2] = lppd; out[3] = acc.mean;
}

__global__ __launch_bounds__(WAIC_T) void waic_total_kernel(WaicArgs A, const double* __restrict__ point,
                                                            double* __restrict__ total) {
  __shared__ double red[WAIC_T / 64];
  const long long g = blockIdx.x;
  if (A.active && !A.active[g]) return;
  const double* __restrict__ pt = point + g * A.n * 4;
  constexpr int NW = WAIC_T / 64;
  double s[3] = {0.0, 0.0, 0.0}, high = 0.0, badp = 0.0, badd = 0.0;
  for (long long i = threadIdx.x; i < A.n; i += WAIC_T) {
    const double e = pt[4 * i], pw = pt[4 * i + 1], l = pt[4 * i + 2], mu = pt[4 * i + 3];
    s[0] += e; s[1] += pw; s[2] += l;
    high += pw > 0.4 ? 1.0 : 0.0;
    badp += (fmh_isfinite(e) && fmh_isfinite(pw) && fmh_isfinite(l) && fmh_isfinite(mu)) ? 0.0 : 1.0;
  }
  for (long long i = threadIdx.x; i < A.P.nblk; i += WAIC_T) badd += A.work[A.P.off_bad + g * A.P.nblk + i];
  const double dn = (double)A.n;
  double sum[3], var[3];
  for (int q = 0; q < 3; q++) sum[q] = block_sum<NW>(s[q], red);
  double v[3] = {0.0, 0.0, 0.0};
  for (long long i = threadIdx.x; i < A.n; i += WAIC_T)
    for (int q = 0; q < 3; q++) {
      const double d = pt[4 * i + q] - sum[q] / dn;
      v[q] = fmh_fma(d, d, v[q]);
    }
  for (int q = 0; q < 3; q++) var[q] = block_sum<NW>(v[q], red) / (dn - 1.0);
  high = block_sum<NW>(high, red);
  badp = block_sum<NW>(badp, red);
  badd = block_sum<NW>(badd, red);
  if (threadIdx.x == 0) {
    double* o = total + g * 10;
    o[0] = sum[0]; o[1] = sum[1]; o[2] = sum[2]; o[3] = -2.0 * sum[0];
    for (int q = 0; q < 3; q++) o[4 + q] = fmh_sqrt(dn * var[q]);
    o[7] = high; o[8] = badd; o[9] = badp;
  }
}

// Every check of the two entries, before any device call.
inline int waic_check(const char* who, const fmcmc_model* m, int64_t x_stride, int64_t y_stride, const void* samples, int64_t G,
                      int64_t cpg, int32_t k, int64_t S, int64_t row0, int64_t N) {
  if (!m || !samples) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (m->family != FMCMC_FAM_GAUSSIAN_LINREG && m->family != FMCMC_FAM_LOGISTIC && m->family != FMCMC_FAM_IID_NORMAL)
    return fail(FMCMC_ERR_ARG, "%s: unknown family %d", who, (int)m->family);
  if (m->n < 1 || m->p < 0 || !m->y || (m->p > 0 && !m->X) || (m->family == FMCMC_FAM_IID_NORMAL && m->p != 0))
    return fail(FMCMC_ERR_ARG, "%s: the model needs n >= 1 observations, y, and X for its p >= 0 columns (iid_normal: p = 0)", who);
  if ((long long)m->p + 2 > 0x7fffffffLL || waic_family_k(m) < 1 || waic_family_k(m) > FMCMC_MAX_K)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: the family has %lld parameters; supported are 1 .. %d", who,
                (long long)m->p + (m->intercept ? 1 : 0) + (m->family == FMCMC_FAM_GAUSSIAN_LINREG), FMCMC_MAX_K);
  if (k != waic_family_k(m))
    return fail(FMCMC_ERR_ARG, "%s: k = %d, but the family has %d parameters", who, (int)k, waic_family_k(m));
  if (G < 1 || cpg < 1)
    return fail(FMCMC_ERR_ARG, "%s: ngroups = %lld, chains_per_group = %lld: each must be at least 1", who, (long long)G,
                (long long)cpg);
  if (cpg > 0x7fffffffLL / G)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld groups x %lld chains exceed one launch", who, (long long)G, (long long)cpg);
  if (N < 1 || row0 < 0 || row0 + N > S)
    return fail(FMCMC_ERR_ARG, "%s: the window [%lld, %lld) is outside the %lld rows of a chain", who, (long long)row0,
                (long long)(row0 + N), (long long)S);
  if (N > (1LL << 40) / cpg) return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld chains x %lld rows exceed one launch", who,
                                         (long long)cpg, (long long)N);
  if (cpg * N < 2) return fail(FMCMC_ERR_ARG, "%s: S = %lld draw: WAIC needs at least 2", who, (long long)(cpg * N));
  if (G > 1 && (x_stride < (int64_t)m->p * m->n || y_stride < m->n))
    return fail(FMCMC_ERR_ARG, "%s: x_stride = %lld, y_stride = %lld are smaller than a dataset (%lld, %lld)", who,
                (long long)x_stride, (long long)y_stride, (long long)m->p * (long long)m->n, (long long)m->n);
  if ((m->n + 63) / 64 > 0x7fffffffLL / G || G > 65535 || (cpg * N + WAIC_T - 1) / WAIC_T > 0x7fffffffLL)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld groups x %lld observations x %lld draws exceed one launch", who, (long long)G,
                (long long)m->n, (long long)(cpg * N));
  return FMCMC_OK;
}

int waic_run(const char* who, const fmcmc_model* m0, int64_t x_stride, int64_t y_stride, const double* samples, int64_t ngroups,
             int64_t chains_per_group, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* active, double* work,
             double* point, double* total, void* hip_stream) {
  if (!work || !point || !total) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = waic_check(who, m0, x_stride, y_stride, samples, ngroups, chains_per_group, k, S, row0, N);
  if (rc != FMCMC_OK) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  WaicArgs A;
  A.samples = samples; A.X = m0->X; A.y = m0->y; A.active = active; A.work = work;
  A.x_stride = x_stride; A.y_stride = y_stride; A.S = S; A.row0 = row0; A.N = N; A.n = m0->n; A.cpg = chains_per_group;
  A.k = k;
  A.P = waic_plan(m0, ngroups, chains_per_group, N);
  const WaicPlan& P = A.P;
  const unsigned G = (unsigned)ngroups;
  hipLaunchKernelGGL(waic_draw_kernel, dim3((unsigned)P.nblk, G), dim3(WAIC_T), 0, st, A);
  const dim3 grid((unsigned)(P.tiles * ngroups), (unsigned)P.nparts);
  if (P.nq <= 2) {                                   // (k <= 8: the headline regression, the vignette's logistic model)
    hipLaunchKernelGGL(waic_tile_kernel<2>, grid, dim3(WAIC_T), 0, st, A);
  } else if (P.nq <= 4) {
    hipLaunchKernelGGL(waic_tile_kernel<4>, grid, dim3(WAIC_T), 0, st, A);
  } else if (P.nq <= WAIC_REG_Q) {
    hipLaunchKernelGGL(waic_tile_kernel<WAIC_REG_Q>, grid, dim3(WAIC_T), 0, st, A);
  } else {
    const size_t lds = (size_t)P.nq * WAIC_T * sizeof(double);
    if ((rc = allow_lds(who, waic_tile_kernel<0>, lds)) != FMCMC_OK) return rc;
    hipLaunchKernelGGL(waic_tile_kernel<0>, grid, dim3(WAIC_T), lds, st, A);
  }
  hipLaunchKernelGGL(waic_merge_kernel, dim3((unsigned)((A.n + WAIC_T - 1) / WAIC_T), G), dim3(WAIC_T), 0, st, A, point);
  hipLaunchKernelGGL(waic_total_kernel, dim3(G), dim3(WAIC_T), 0, st, A, point, total);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

}  // namespace

extern "C" {

int64_t fmcmc_waic_part_rows(void) { return WAIC_PART_ROWS; }

int64_t fmcmc_waic_parts(int64_t chains_per_group, int64_t N, int64_t n) {
  if (chains_per_group < 1 || N < 1 || n < 1 || N > (1LL << 40) / chains_per_group) return 0;
  fmcmc_model m;
  m.family = FMCMC_FAM_IID_NORMAL; m.p = 0; m.n = n; m.X = nullptr; m.y = nullptr; m.intercept = 1; m.guard = 0; m.prior_div = 0.0;
  return waic_plan(&m, 1, chains_per_group, N).nparts;
}

int64_t fmcmc_waic_work_len(const fmcmc_model* m, int64_t ngroups, int64_t chains_per_group, int64_t N) {
  static const double nothing = 0.0;
  if (!m) return 0;
  if (waic_check("fmcmc_waic_work_len", m, (int64_t)m->p * m->n, m->n, &nothing, ngroups, chains_per_group, waic_family_k(m), N, 0,
                 N) != FMCMC_OK)
    return 0;
  return waic_plan(m, ngroups, chains_per_group, N).len;
}

int fmcmc_waic_groups_dev(const fmcmc_model* m0, int64_t x_stride, int64_t y_stride, const double* samples, int64_t ngroups,
                          int64_t chains_per_group, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* active,
                          double* work, double* point, double* total, void* hip_stream) {
  return waic_run("fmcmc_waic_groups_dev", m0, x_stride, y_stride, samples, ngroups, chains_per_group, k, S, row0, N, active, work,
                  point, total, hip_stream);
}

int fmcmc_waic_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                   double* work, double* point, double* total, void* hip_stream) {
  return waic_run("fmcmc_waic_dev", m, 0, 0, samples, 1, nchains, k, S, row0, N, nullptr, work, point, total, hip_stream);
}

}  // extern "C"
