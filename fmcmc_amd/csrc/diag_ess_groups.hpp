// diag_ess_groups.hpp — the rank-normalised bulk and tail effective sample size of diag_ess.hpp for many small groups of chains in
// ONE launch (one model on many datasets: a group = the chains of a dataset).  Included by raftery.hip alone, after diag_ess.hpp
// and diag_rank_groups.hpp.
//
// One workgroup of RT_THREADS threads takes one (group, column) and does everything fmcmc_rank_ess_dev does for that group's
// column, with no host involvement and no word shared between workgroups.  m = 2 cpg split chains of n = floor(N / 2) rows,
// M = m n <= RG_MAX_VALUES pooled values, element e = s n + r as rank_gather_kernel numbers them:
//   sort      key_of(x + 0.0) of every element into LDS, all-ones pads up to the power of two P, the bitonic network of
//             rank_groups_kernel; the non-finite values are counted on the way (an integer atomic in LDS);
//   info      q05, q95 (ess_quantile, the EssQuant ranks of M from the host), the least and the largest value;
//   scores    every element's key is formed again and looked up in the sorted keys (lower and upper bound among the first M),
//             z = fmh_qnorm((r - 0.375) / (M + 0.25)) as rank_groups_kernel has it, into `work` (M doubles a (group, column)):
//             written and read by this workgroup alone.  From here on the keys are dead and their LDS is used again;
//   series    bulk, q05, q95, mean, one after another.  A split chain's n rows are staged in LDS (s_y): the scores from `work`,
//             the indicators and the values formed from `samples` (ess_indicator, the row arithmetic of ess_fill_kernel).
//     stats   per split chain, the mean and variance in split_stats_kernel's order (walk_pairs<RT_THREADS, RS_LU> over s_y,
//             split_sum) into `out`;
//     rounds  the rounds of lags of ess_series.  In a round every split chain is staged once and passes block after block of 256
//             lags through ess_autocov_block (the body of ess_autocov_kernel: the same tiles, the same four wavefronts, the same
//             join); the thread that owns a lag adds c_s(t) to S(t) in LDS in the order s = 0, 1, ... from 0.0, which is
//             ess_sum_kernel's sum.  Then geyer_head (first round, one thread), geyer_pairs and geyer_cut: the expressions of
//             geyer_scan_kernel.  The loop ends when the cut is known: the word is read from LDS after a barrier, so the branch is
//             the same for the whole workgroup; workgroups leave at different rounds and share nothing.
// `out` of a (group, column) has the layout of fmcmc_rank_ess_dev's column (ess_col_len doubles), and every element the single
// form writes has the same bits here: the same expressions in the same order on the same values, all of them functions of the
// group's own rows.  LDS: max(8 P, 8 (EA_T + 16 + EA_B + 4 * 256 + n + (n - 2))) bytes: 64 KB at 4 x 2000 (two workgroups a CU),
// 108.4 KB at the limit n = 4096.  Nothing here writes `samples`.
#pragma once
#include "diag_ess.hpp"
#include "diag_rank_groups.hpp"

namespace {

inline size_t ess_groups_lds(unsigned int P, unsigned int n) {
  const size_t keys = (size_t)P * sizeof(unsigned long long);
  const size_t rest = ((size_t)(EA_T + 16) + EA_B + RT_WAVES * 256 + n + (n - 2)) * sizeof(double);
  return keys > rest ? keys : rest;
}

__global__ __launch_bounds__(RT_THREADS) void ess_groups_kernel(const double* __restrict__ samples, long long S, int k,
                                                                long long row0, long long N, long long cpg,
                                                                const int* __restrict__ cols, int p,
                                                                const int* __restrict__ active, unsigned int M, unsigned int P,
                                                                EssQuant t, double* work, double* out) {
  extern __shared__ unsigned long long s_k[];        // [P] keys; after the scores: s_a, s_b, s_p, s_y [n], s_S [n - 2]
  __shared__ double s_w[RT_WAVES];
  __shared__ double s_q[2], s_W, s_V;
  __shared__ unsigned int s_nf, s_first, s_cut;
  const long long g = (long long)blockIdx.x / p;
  const int j = (int)((long long)blockIdx.x % p);
  if (active && active[g] == 0) return;              // (uniform per workgroup: before the first barrier)
  const int tid = threadIdx.x;
  const int col = cols[j];
  const bool col_ok = col >= 0 && col < k;           // (a column outside k reads nothing: its values count as non-finite)
  const unsigned int n = (unsigned int)(N / 2), m = (unsigned int)(2 * cpg), cap = n - 2u;
  const double* __restrict__ x0 = samples + (g * cpg * k + (col_ok ? col : 0)) * S + row0;
  auto value = [&](unsigned int s, unsigned int r) -> double {   // row r of split chain s, as rank_gather_kernel reads it
    const long long row = (s & 1u) ? N - n + r : (long long)r;
    return col_ok ? x0[(long long)(s >> 1) * k * S + row] : fmh_nan();
  };
  const long long kl = 2LL * m + 2 + cap;
  double* o = out + (long long)blockIdx.x * (ESS_KINDS * kl + ESS_INFO);
  double* info = o + ESS_KINDS * kl;
  double* z = work + (long long)blockIdx.x * M;
  if (tid == 0) s_nf = 0u;
  __syncthreads();
  // ---------------------------------------------------------------------------------------------------------------- sort
  unsigned int nf = 0u;
  for (unsigned int e = tid; e < P; e += RT_THREADS) {
    unsigned long long kx = ~0ull;
    if (e < M) {
      const unsigned int s = e / n;
      const double x = value(s, e - s * n);
      nf += fmh_isfinite(x) ? 0u : 1u;
      kx = key_of(x + 0.0);
    }
    s_k[e] = kx;
  }
  if (nf) atomicAdd(&s_nf, nf);
  __syncthreads();
  for (unsigned int kk = 2; kk <= P; kk <<= 1) {     // ascending, the network of rank_groups_kernel
    for (unsigned int jj = kk >> 1; jj >= 1; jj >>= 1) {
      for (unsigned int q = tid; q < (P >> 1); q += RT_THREADS) {
        const unsigned int i = ((q & ~(jj - 1u)) << 1) | (q & (jj - 1u)), l = i | jj;
        const unsigned long long a = s_k[i], b = s_k[l];
        const bool up = (i & kk) == 0u;
        if ((a > b) == up) { s_k[i] = b; s_k[l] = a; }
      }
      __syncthreads();
    }
  }
  // ---------------------------------------------------------------------------------------------------------------- info
  if (tid == 0) {
    info[0] = (double)s_nf;
    for (int i = 0; i < 2; i++) {
      const double q = ess_quantile(s_k, t, i);
      s_q[i] = q;
      info[1 + i] = q;
    }
    info[5] = value_of(s_k[0]);
    info[6] = value_of(s_k[M - 1]);
  }
  // -------------------------------------------------------------------------------------------------------------- scores
  const double denom = (double)M + 0.25;
  for (unsigned int e = tid; e < M; e += RT_THREADS) {
    const unsigned int s = e / n;
    const unsigned long long kx = key_of(value(s, e - s * n) + 0.0);
    unsigned int lo = 0u, hi = M;                    // #less: the first position whose key is not below kx
    while (lo < hi) {
      const unsigned int mid = (lo + hi) >> 1;
      if (s_k[mid] < kx) lo = mid + 1u; else hi = mid;
    }
    const unsigned int less = lo;
    hi = M;                                          // #less-or-equal: the first position whose key is above kx
    while (lo < hi) {
      const unsigned int mid = (lo + hi) >> 1;
      if (s_k[mid] <= kx) lo = mid + 1u; else hi = mid;
    }
    const double twice = (double)((unsigned long long)less + (unsigned long long)lo + 1ull);   // 2 #less + #equal + 1
    z[e] = fmh_qnorm((0.5 * twice - 0.375) / denom);
  }
  __syncthreads();                                   // the keys are dead, z and s_q are written
  double* s_a = reinterpret_cast<double*>(s_k);
  double* s_b = s_a + (EA_T + 16);
  double* s_p = s_b + EA_B;
  double* s_y = s_p + RT_WAVES * 256;
  double* s_S = s_y + n;
  // -------------------------------------------------------------------------------------------------------------- series
  for (int kind = 0; kind < ESS_KINDS; kind++) {
    double* ok = o + kind * kl;                      // 2 m stats, L, K, S[0 .. cap)
    const double q = (kind == 1 || kind == 2) ? s_q[kind - 1] : 0.0;
    auto stage = [&](unsigned int s) {               // split chain s of the series into s_y (the caller's barrier follows)
      for (unsigned int r = tid; r < n; r += RT_THREADS)
        s_y[r] = kind == 0 ? z[(long long)s * n + r] : ess_indicator(kind, value(s, r), q);
    };
    for (unsigned int s = 0; s < m; s++) {           // split_stats_kernel
      stage(s);
      __syncthreads();
      double acc = 0.0;
      walk_pairs<RT_THREADS, RS_LU>(s_y, (long long)n, [&](long long, double a, double b, bool has_b) { acc += a; if (has_b) acc += b; });
      const double mean = split_sum(acc, s_w) / (double)(long long)n;
      acc = 0.0;
      walk_pairs<RT_THREADS, RS_LU>(s_y, (long long)n, [&](long long, double a, double b, bool has_b) {
        const double da = a - mean;
        acc += da * da;
        if (has_b) { const double db = b - mean; acc += db * db; }
      });
      const double var = split_sum(acc, s_w) / (double)((long long)n - 1);
      if (tid == 0) { ok[2 * s] = mean; ok[2 * s + 1] = var; }
      __syncthreads();                               // (s_y and s_w are written again; the stats are read below)
    }
    for (unsigned int T0 = 0, T1 = cap < 256u ? cap : 256u;;) {
      const unsigned int nblk = (T1 - T0 + EA_LAGS - 1) / EA_LAGS;
      for (unsigned int s = 0; s < m; s++) {
        stage(s);                                    // (ess_autocov_block starts with a barrier)
        const double mean = ok[2 * s];
        for (unsigned int jb = 0; jb < nblk; jb++) {
          long long lag;
          const double cv = ess_autocov_block([&](long long r) { return s_y[r]; }, mean, (long long)n,
                                              (long long)T0 + (long long)EA_LAGS * jb + 15, s_a, s_b, s_p, &lag);
          if (lag < (long long)T1) s_S[lag] = (s ? s_S[lag] : 0.0) + cv;     // ess_sum_kernel: from 0.0, s = 0, 1, ...
        }
        __syncthreads();                             // (s_y is staged again)
      }
      if (tid == 0) {
        s_first = 0xffffffffu;
        if (T0 == 0u) geyer_head(ok, m, n, s_S[0], &s_W, &s_V, kind == 3 ? info : nullptr);
      }
      for (unsigned int lag = T0 + tid; lag < T1; lag += RT_THREADS) ok[2 * m + 2 + lag] = s_S[lag];
      __syncthreads();
      geyer_pairs(s_S, T0, T1, (double)m, s_W, s_V, &s_first);
      __syncthreads();
      if (tid == 0) {
        const unsigned int K = geyer_cut(s_first, T1, cap);
        s_cut = K;
        ok[2 * m] = (double)T1;
        if (K) ok[2 * m + 1] = (double)K;
      }
      __syncthreads();
      if (s_cut != 0u || T1 == cap) break;           // (read from LDS after the barrier: the same for the whole workgroup)
      T0 = T1;
      T1 = ess_next_round(T1, cap);
    }
    __syncthreads();                                 // (s_cut and s_first are written again by the next series)
  }
}

}  // namespace

extern "C" {

int64_t fmcmc_rank_ess_groups_work_len(int64_t ngroups, int64_t chains_per_group, int32_t p, int64_t N) {
  if (ngroups < 1 || chains_per_group < 1 || p < 1 || N < 8) return 0;
  if (chains_per_group > RG_MAX_VALUES || 2 * chains_per_group * (N / 2) > RG_MAX_VALUES) return 0;
  if (ngroups > 0x7fffffffLL / p) return 0;
  return ngroups * (int64_t)p * (2 * chains_per_group * (N / 2));   // the scores of every (group, column)
}

int64_t fmcmc_rank_ess_groups_out_len(int64_t ngroups, int64_t chains_per_group, int32_t p, int64_t N) {
  if (fmcmc_rank_ess_groups_work_len(ngroups, chains_per_group, p, N) == 0) return 0;
  return ngroups * (int64_t)p * ess_col_len(2 * chains_per_group, N / 2);
}

int fmcmc_rank_ess_groups_dev(const double* samples, int64_t ngroups, int64_t chains_per_group, int32_t k, int64_t S, int64_t row0,
                              int64_t N, const int32_t* cols, int32_t p, const int32_t* active, double* work, double* out,
                              void* hip_stream) {
  const char* who = "fmcmc_rank_ess_groups_dev";
  if (!samples || !cols || !work || !out) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (ngroups < 1 || chains_per_group < 1)
    return fail(FMCMC_ERR_ARG, "%s: ngroups = %lld, chains_per_group = %lld: each must be at least 1", who, (long long)ngroups,
                (long long)chains_per_group);
  int rc = rank_check(who, samples, cols, work, out, chains_per_group, k, S, row0, N, p);   // (the 2^32 limit: of one group)
  if (rc != FMCMC_OK) return rc;
  if (N < 8) return fail(FMCMC_ERR_ARG, "%s: a window of N = %lld rows is too short: shorter than 8 rows", who, (long long)N);
  const long long Mll = 2 * chains_per_group * (N / 2);
  if (Mll > RG_MAX_VALUES)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: 2 x %lld split chains of %lld rows are %lld values in a group; a group's keys are "
                "sorted in LDS, at most %lld of them -- fmcmc_rank_ess_dev per group is the form for larger groups", who,
                (long long)chains_per_group, (long long)(N / 2), Mll, RG_MAX_VALUES);
  if (ngroups > 0x7fffffffLL / p || chains_per_group > 0x7fffffffLL / ngroups)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld groups x %lld chains x %d columns exceed one launch", who, (long long)ngroups,
                (long long)chains_per_group, (int)p);
  hipStream_t st = (hipStream_t)hip_stream;
  const unsigned int M = (unsigned int)Mll, P = rank_groups_pad(M);
  EssQuant t;
  for (int i = 0; i < 2; i++) {
    const Type7 r = type7_ranks(Mll, i ? 0.95 : 0.05);
    t.lo[i] = (unsigned int)r.lo; t.hi[i] = (unsigned int)r.hi; t.between[i] = r.between; t.h[i] = r.h;
  }
  const size_t lds = ess_groups_lds(P, (unsigned int)(N / 2));
  rc = allow_lds(who, ess_groups_kernel, lds);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(ess_groups_kernel, dim3((unsigned)(ngroups * p)), dim3(RT_THREADS), lds, st, samples, (long long)S, (int)k,
                     (long long)row0, (long long)N, (long long)chains_per_group, cols, (int)p, active, M, P, t, work, out);
  return rank_launched(who);
}

}  // extern "C"
