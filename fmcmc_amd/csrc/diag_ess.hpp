// diag_ess.hpp — the rank-normalised bulk and tail effective sample size of Vehtari, Gelman, Simpson, Carpenter and Buerkner
// (2021) on top of diag_rank.hpp: the biased autocovariance of every split chain at every lag up to a data-dependent cut, summed
// over the split chains, and Geyer's pair test that finds the cut (the definition is INTEGRATION.md §2.2; the host finish is
// fmcmc_amd/summary.py: geyer_tau, the host restatement fmcmc_amd/convergence.py: ess_host).  Included by raftery.hip alone.
//
// Per column, after the bulk sort of diag_rank.hpp, four series y [m][n] (m = 2 C split chains of n = floor(N / 2) rows) pass
// through the same steps one after another, each in the score buffer z of `work`:
//   bulk   the scores z of the values (rank_score_kernel)
//   q05    1.0 where x <= q05, else 0.0 (ess_fill_kernel; q05, q95: the type-7 quantiles of the sorted bulk keys, ess_quant_kernel)
//   q95    the same for q95
//   mean   the values themselves
//   stats    split_stats_kernel: mean and variance of every split chain
//   rounds   lags [0, 256), [256, 512), [512, 1024), [1024, 2048), ... up to the cap n - 2 (lags 0 .. n - 3).  A round is
//            ess_autocov_kernel (c_s(t) of every split chain for the lags of the round, into the sort's key buffers, which are
//            dead by then), ess_sum_kernel (S(t) = sum_s c_s(t), a thread a lag, in the order s = 0, 1, ...) and
//            geyer_scan_kernel (one workgroup: the pair test on the new lags, the word E_DONE once the cut K is known).  The
//            kernels of later rounds return at once when they read E_DONE; the host enqueues every round and synchronises
//            nothing.
//
// ess_autocov_kernel, one workgroup a (split chain, block of 256 lags): with the centred series u in front of 16 zeros and
// followed by zeros, up[i] = u[i - 16], and L0 = 15 + the block's first lag, the fp64 matrix core sums
//   D[a][b] = sum_q up[q + a] up[q + L0 + 16 b]          (A[a][q] = up[q + a], B[q][b] = up[q + L0 + 16 b])
// so that D holds the 256 lags L0 + 16 b - a.  q walks [0, n + 16 - L0) (beyond it B is zeros) in LDS tiles of EA_T rows: the A
// segment of a tile is EA_T + 16 values, the B segment EA_T + 256 (the halo of the lag block).  The four wavefronts take a quarter of the tile's rows each
// (v_mfma_f64_16x16x4: four rows an instruction) and keep their accumulators from tile to tile; at the end the four partial
// tiles are added in the order ((0 + 1) + 2) + 3 and divided by n.  The order inside an instruction is the matrix core's, so a
// sum is not bit for bit a host sum; it is a function of (n, lag, the series) alone: no atomics, no dependence on the launch,
// the window's place or the other columns.  |c - exact| <= gamma(n + 8) sum |u_i| |u_{i+t}| / n for ANY order of the n - t
// products, each rounded once, u as the device centres it (one rounded subtraction a value, the mean of split_stats_kernel).
//
// What the grouped form (diag_ess_groups.hpp: one workgroup does all of this for a small group's column) computes with the same
// code lives in __device__ functions that the kernels here call: ess_quantile, ess_indicator, ess_autocov_block (the body of
// ess_autocov_kernel), geyer_rho, geyer_head, geyer_pairs, geyer_cut (the three steps of geyer_scan_kernel) and ess_next_round.
#pragma once
#include "diag_rank.hpp"

namespace {

constexpr int EA_T = 2048;                         // rows of q in one LDS tile
constexpr int EA_FRONT = 16;                       // zeros in front of the centred series
constexpr int EA_LAGS = 256;                       // lags of one accumulator tile
constexpr int EA_B = (EA_T + EA_LAGS) / 16 * 18;   // the B segment, 16 values every 18 doubles (see s_b)
constexpr int ESS_KINDS = 4;                       // bulk, q05, q95, mean
constexpr int ESS_INFO = 7;                        // per column: non-finite count, q05, q95, pooled mean, pooled sd, min, max

// The head of `work` past what diag_rank.hpp keeps there (H_MED ends at word 2326 of 2560).
constexpr int E_DONE = 2400;                       // 32-bit word: the cut of the series under way is known
constexpr int E_W = 1204;                          // 64-bit words: W, V of the series under way, q05, q95 of the column
constexpr int E_V = 1205;
constexpr int E_Q = 1206;                          // [2]

struct EssQuant { unsigned int lo[2], hi[2]; int between[2]; double h[2]; };

inline long long ess_lag_cap(long long n) { return n - 2; }   // lags 0 .. n - 3
inline long long ess_kind_len(long long m, long long n) { return 2 * m + 2 + ess_lag_cap(n); }
inline long long ess_col_len(long long m, long long n) { return ESS_KINDS * ess_kind_len(m, n) + ESS_INFO; }

// q05, q95 (R's type 7 on the M sorted values, the arithmetic of summary.py: type7_quantiles), the least and the largest value.
__device__ __forceinline__ double ess_quantile(const unsigned long long* key, const EssQuant& t, int i) {
  const double xlo = value_of(key[t.lo[i]]), xhi = value_of(key[t.hi[i]]);
  return (t.between[i] && xhi != xlo) ? (1.0 - t.h[i]) * xlo + t.h[i] * xhi : xlo;
}

__global__ void ess_quant_kernel(unsigned int* hdr, const unsigned long long* keyA, const unsigned long long* keyB,
                                 unsigned int M, EssQuant t, double* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long* key = hdr[H_FINAL] ? keyB : keyA;
  double* hd = reinterpret_cast<double*>(hdr);
  info[0] = (double)hdr[H_NF];
  for (int i = 0; i < 2; i++) {
    const double q = ess_quantile(key, t, i);
    hd[E_Q + i] = q;
    info[1 + i] = q;
  }
  info[5] = value_of(key[0]);
  info[6] = value_of(key[M - 1]);
}

// kind 1, 2: y = 1.0 where x <= q05 / q95, else 0.0; kind 3: y = x.  Element e = s n + r as rank_gather_kernel reads it.
__device__ __forceinline__ double ess_indicator(int kind, double x, double q) { return kind == 3 ? x : (x <= q ? 1.0 : 0.0); }

__global__ __launch_bounds__(RT_THREADS) void ess_fill_kernel(const double* __restrict__ samples, long long S, int k,
                                                              long long row0, long long N, const int* __restrict__ cols, int j,
                                                              int kind, unsigned int M, const unsigned int* __restrict__ hdr,
                                                              double* __restrict__ y) {
  const int col = cols[j];
  const bool col_ok = col >= 0 && col < k;
  const unsigned int Nh = (unsigned int)(N / 2);
  const double q = kind == 3 ? 0.0 : reinterpret_cast<const double*>(hdr)[E_Q + kind - 1];
#pragma unroll 4
  for (int u = 0; u < RT_PER; u++) {
    const unsigned long long e = (unsigned long long)blockIdx.x * RT + (unsigned long long)u * RT_THREADS + threadIdx.x;
    if (e < M) {
      const unsigned int s = (unsigned int)e / Nh, r = (unsigned int)e - s * Nh;
      const long long row = row0 + ((s & 1u) ? N - Nh + r : (long long)r);
      const double x = col_ok ? samples[((long long)(s >> 1) * k + col) * S + row] : fmh_nan();
      y[e] = ess_indicator(kind, x, q);
    }
  }
}

typedef double ess_d4 __attribute__((ext_vector_type(4)));

// The 256 lags L0 - 15 .. L0 + 240 of one split chain by the RT_THREADS threads of a workgroup: x(g) = row g of the series,
// g in [0, nn); s_a [EA_T + 16], s_b [EA_B], s_p [RT_WAVES * 256] in LDS.  Returns c(lag) = the sum / nn and the lag of the
// calling thread.  Every barrier here is met by the whole workgroup: the trip counts depend on (nn, L0) alone.
template <typename Row>
__device__ __forceinline__ double ess_autocov_block(Row x, double mean, long long nn, long long L0, double* s_a, double* s_b,
                                                    double* s_p, long long* lag_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, col = lane & 15;
  const long long total = nn - L0 + EA_FRONT;        // rows of q: from there on B is zeros for every lag of the block
  ess_d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (long long tile = 0; tile < total; tile += EA_T) {
    __syncthreads();
    for (int i = tid; i < EA_T + 16; i += RT_THREADS) {
      const long long g = tile + i - EA_FRONT;
      s_a[i] = (g >= 0 && g < nn) ? x(g) - mean : 0.0;
    }
    for (int i = tid; i < EA_T + EA_LAGS; i += RT_THREADS) {
      const long long g = tile + L0 + i - EA_FRONT;
      s_b[i + 2 * (i >> 4)] = (g >= 0 && g < nn) ? x(g) - mean : 0.0;
    }
    __syncthreads();
    const long long left = total - tile;             // rows of q that are left: the rest of the tile multiplies zeros
    const int rows = left < EA_T ? (int)((left + 3) & ~3LL) : EA_T;
    const int q1 = (wave + 1) * (EA_T / RT_WAVES) < rows ? (wave + 1) * (EA_T / RT_WAVES) : rows;
    for (int q = wave * (EA_T / RT_WAVES); q < q1; q += 4) {
      const int ia = q + kk + col, ib = q + kk + 16 * col;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_a[ia], s_b[ib + 2 * (ib >> 4)], acc, 0, 0, 0);
    }
  }
  // D register r of lane l is row a = 4 r + l / 16, column b = l % 16: lag L0 + 16 b - a
#pragma unroll
  for (int r = 0; r < 4; r++) s_p[wave * 256 + lane * 4 + r] = acc[r];
  __syncthreads();
  const int l = tid >> 2, r = tid & 3;
  *lag_out = L0 + 16 * (l & 15) - (4 * r + (l >> 4));
  const double sum = ((s_p[tid] + s_p[256 + tid]) + s_p[512 + tid]) + s_p[768 + tid];
  return sum / (double)nn;
}

// c[s (T1 - T0) + t - T0] = c_s(t) for the lags t in [T0, T1) of split chain s = blockIdx.x / nblk, 256 lags a workgroup.
__global__ __launch_bounds__(RT_THREADS) void ess_autocov_kernel(const unsigned int* __restrict__ hdr,
                                                                 const double* __restrict__ y,
                                                                 const double* __restrict__ stats, unsigned int n,
                                                                 unsigned int T0, unsigned int T1, unsigned int nblk,
                                                                 double* __restrict__ c) {
  __shared__ double s_a[EA_T + 16];                  // up[tile + i]
  // up[tile + L0 + i] at i + 2 (i / 16): the lanes of a half wavefront read i = i0 + kk + 16 b, b < 16, kk < 2, which are the 32
  // double slots 18 b + kk + const: 18 b mod 32 runs through the even slots once, kk picks even or odd
  __shared__ double s_b[EA_B];
  __shared__ double s_p[RT_WAVES * 256];
  if (T0 != 0u && hdr[E_DONE]) return;
  const unsigned int s = blockIdx.x / nblk, jb = blockIdx.x - s * nblk;
  const long long L0 = (long long)T0 + (long long)EA_LAGS * jb + 15;
  const long long nn = n;
  const double* __restrict__ x = y + (long long)s * nn;
  long long lag;
  const double cv = ess_autocov_block([&](long long g) { return x[g]; }, stats[2 * (long long)s], nn, L0, s_a, s_b, s_p, &lag);
  if (lag < (long long)T1) c[(long long)s * (T1 - T0) + (lag - T0)] = cv;
}

// rho_t of the definition, plain IEEE operations in the written order (the unit is built without contraction): the same
// expression as summary.py: geyer_tau.
__device__ __forceinline__ double geyer_rho(const double* S, unsigned int t, double dm, double W, double V) {
  return t == 0u ? 1.0 : 1.0 - (W - S[t] / dm) / V;
}

// S(t) = sum_s c_s(t) of the lags of a round, one thread a lag.
__global__ __launch_bounds__(RT_THREADS) void ess_sum_kernel(const unsigned int* __restrict__ hdr, const double* __restrict__ c,
                                                             unsigned int m, unsigned int T0, unsigned int T1,
                                                             double* __restrict__ S) {
  if (T0 != 0u && hdr[E_DONE]) return;
  const unsigned int t = T0 + blockIdx.x * RT_THREADS + threadIdx.x, width = T1 - T0;
  if (t >= T1) return;
  double sum = 0.0;
  for (unsigned int s = 0; s < m; s++) sum += c[(long long)s * width + (t - T0)];
  S[t] = sum;
}

// The head of the pair test, by one thread: W, V of the series from the split chains' means and S(0); info: the column's
// {.., pooled mean, pooled sd, ..} when the series is the values themselves, else null.
__device__ __forceinline__ void geyer_head(const double* stats, unsigned int m, unsigned int n, double S0, double* W, double* V,
                                           double* info) {
  const double dm = (double)m, dn = (double)n;
  double grand = 0.0, d2 = 0.0;
  for (unsigned int s = 0; s < m; s++) grand += stats[2 * (long long)s];
  grand = grand / dm;
  for (unsigned int s = 0; s < m; s++) {
    const double d = stats[2 * (long long)s] - grand;
    d2 += d * d;
  }
  *W = S0 / dm * dn / (dn - 1.0);
  *V = S0 / dm + d2 / (dm - 1.0);
  if (info) {
    info[3] = grand;
    info[4] = sqrt((dn * S0 + dn * d2) / (dm * dn - 1.0));
  }
}

// The pairs whose lags lie in [T0, T1), a thread a pair: the first failing one into *first (LDS, an integer minimum).
__device__ __forceinline__ void geyer_pairs(const double* S, unsigned int T0, unsigned int T1, double dm, double W, double V,
                                            unsigned int* first) {
  const unsigned int j0 = T0 < 2u ? 1u : T0 / 2u;
  for (unsigned int j = j0 + threadIdx.x; 2u * j + 1u < T1; j += RT_THREADS) {
    const double P = geyer_rho(S, 2u * j, dm, W, V) + geyer_rho(S, 2u * j + 1u, dm, W, V);
    if (!(P >= 0.0)) atomicMin(first, j);
  }
}

// The cut after the round that ended at T1, 0: not known yet.  The cap: the first j with 2 j + 1 > n - 3.
__device__ __forceinline__ unsigned int geyer_cut(unsigned int first, unsigned int T1, unsigned int cap) {
  return first != 0xffffffffu ? first : (T1 == cap ? cap / 2u : 0u);
}

// One workgroup after every round: the pair test on the new lags.  kout = {L, K} of the series, S = its S(t); info as
// geyer_head takes it.
__global__ __launch_bounds__(RT_THREADS) void geyer_scan_kernel(unsigned int* hdr, const double* __restrict__ stats,
                                                                unsigned int m, unsigned int n, unsigned int T0,
                                                                unsigned int T1, unsigned int cap, double* kout,
                                                                const double* __restrict__ S, double* info) {
  __shared__ unsigned int s_k;
  if (T0 != 0u && hdr[E_DONE]) return;
  const int tid = threadIdx.x;
  double* hd = reinterpret_cast<double*>(hdr);
  if (tid == 0) s_k = 0xffffffffu;
  if (T0 == 0u && tid == 0) geyer_head(stats, m, n, S[0], hd + E_W, hd + E_V, info);
  __syncthreads();
  geyer_pairs(S, T0, T1, (double)m, hd[E_W], hd[E_V], &s_k);
  __syncthreads();
  if (tid == 0) {
    const unsigned int K = geyer_cut(s_k, T1, cap);
    hdr[E_DONE] = K ? 1u : 0u;
    kout[0] = (double)T1;
    if (K) kout[1] = (double)K;
  }
}

// The rounds of lags after [T0, T1): [0, 256), [256, 512), [512, 1024), ... up to the cap.
__host__ __device__ inline unsigned int ess_next_round(unsigned int T1, unsigned int cap) {
  unsigned int nx = T1 < 512u ? 512u : (T1 > cap / 2u ? cap : 2u * T1);
  return nx > cap ? cap : nx;
}

// stats, then every round, of the series in b.z; o: the series' part of `out`.
inline int ess_series(const char* who, unsigned int m, unsigned int n, const RankBufs& b, double* o, double* info,
                      hipStream_t st) {
  double* c = reinterpret_cast<double*>(b.key[0]);   // key[0], key[1]: 2 M doubles in a row; a round needs at most M of them
  const unsigned int cap = (unsigned int)ess_lag_cap(n);
  hipLaunchKernelGGL(split_stats_kernel, dim3(m), dim3(RT_THREADS), 0, st, b.z, (long long)n, o);
  for (unsigned int T0 = 0, T1 = cap < 256u ? cap : 256u;;) {
    const unsigned int nblk = (T1 - T0 + EA_LAGS - 1) / EA_LAGS;
    hipLaunchKernelGGL(ess_autocov_kernel, dim3(m * nblk), dim3(RT_THREADS), 0, st, b.hdr, b.z, o, n, T0, T1, nblk, c);
    hipLaunchKernelGGL(ess_sum_kernel, dim3(nblk), dim3(RT_THREADS), 0, st, b.hdr, c, m, T0, T1, o + 2 * (long long)m + 2);
    hipLaunchKernelGGL(geyer_scan_kernel, dim3(1), dim3(RT_THREADS), 0, st, b.hdr, o, m, n, T0, T1, cap, o + 2 * (long long)m,
                       o + 2 * (long long)m + 2, info);
    if (T1 == cap) break;
    T0 = T1;
    T1 = ess_next_round(T1, cap);
  }
  return rank_launched(who);
}

}  // namespace

extern "C" {

int64_t fmcmc_rank_ess_work_len(int64_t nchains, int32_t p, int64_t N) {
  if (N < 8) return 0;
  return fmcmc_rank_work_len(nchains, p, N);         // the rounds live in the sort's key buffers
}

int64_t fmcmc_rank_ess_out_len(int64_t nchains, int32_t p, int64_t N) {
  if (nchains < 1 || p < 1 || N < 8 || nchains > 0x7fffffffLL || N / 2 > 0xffffffffLL / (2 * nchains)) return 0;
  return (int64_t)p * ess_col_len(2 * nchains, N / 2);
}

int fmcmc_rank_ess_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                       const int32_t* cols, int32_t p, double* work, double* out, void* hip_stream) {
  const char* who = "fmcmc_rank_ess_dev";
  int rc = rank_check(who, samples, cols, work, out, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (N < 8) return fail(FMCMC_ERR_ARG, "%s: a window of N = %lld rows is too short: shorter than 8 rows", who, (long long)N);
  hipStream_t st = (hipStream_t)hip_stream;
  const long long Mll = 2 * nchains * (N / 2), n = N / 2;
  const unsigned int M = (unsigned int)Mll, m = (unsigned int)(2 * nchains), nt = (unsigned int)rank_tiles(Mll);
  const RankBufs b = rank_bufs(work, Mll);
  EssQuant t;
  for (int i = 0; i < 2; i++) {
    const Type7 r = type7_ranks(Mll, i ? 0.95 : 0.05);
    t.lo[i] = (unsigned int)r.lo; t.hi[i] = (unsigned int)r.hi; t.between[i] = r.between; t.h[i] = r.h;
  }
  const long long kl = ess_kind_len(m, n);
  for (int j = 0; j < p; j++) {
    double* o = out + (long long)j * ess_col_len(m, n);
    double* info = o + ESS_KINDS * kl;
    if ((rc = rank_sort_column(who, samples, k, S, row0, N, cols, j, 0, M, b, st)) != FMCMC_OK) return rc;
    hipLaunchKernelGGL(ess_quant_kernel, dim3(1), dim3(64), 0, st, b.hdr, b.key[0], b.key[1], M, t, info);
    if ((rc = rank_score_column(who, M, b, 0, b.z, st)) != FMCMC_OK) return rc;
    for (int kind = 0; kind < ESS_KINDS; kind++) {
      if (kind)
        hipLaunchKernelGGL(ess_fill_kernel, dim3(nt), dim3(RT_THREADS), 0, st, samples, (long long)S, (int)k, (long long)row0,
                           (long long)N, cols, j, kind, M, b.hdr, b.z);
      if ((rc = ess_series(who, m, (unsigned int)n, b, o + kind * kl, kind == 3 ? info : nullptr, st)) != FMCMC_OK) return rc;
    }
  }
  return FMCMC_OK;
}

}  // extern "C"
