// diag_rank_groups.hpp — the rank-normalised split R-hat of diag_rank.hpp for many small groups of chains in ONE launch (one model
// on many datasets: a group = the chains of a dataset).  Included by raftery.hip alone, after diag_rank.hpp.
//
// A group's pooled values are few (4 chains x 2000 rows: 8000 doubles), so nothing is sorted through HBM: one workgroup takes one
// (group, column) and keeps the M = 2 cpg N' keys of the column in LDS, padded with all-ones keys to the power of two P >= M.
// Elements are numbered as rank_gather_kernel numbers them, e = s N' + r.  Per fold (0: x, 1: |x - med|):
//   gather    key_of(x + 0.0) of every element into LDS (the expressions of rank_gather_kernel); the bulk pass counts the
//             non-finite values (an integer atomic in LDS);
//   sort      a bitonic network over the P keys, in place.  Keys only: ranks of ties are averages, so neither stability nor
//             an index is needed.  A pad ties with a real all-ones key (a NaN); both are the same bits, and only the first M
//             positions are looked at afterwards;
//   median    the bulk pass reads med = (x_(M/2 - 1) + x_(M/2)) / 2 from the sorted keys;
//   rank      split chain after split chain: every element's own key is formed again from `samples` and looked up in the
//             sorted keys, #less = its lower bound and #less-or-equal = its upper bound among the first M, 2 r = their sum + 1,
//             z = fmh_qnorm((r - 0.375) / (M + 0.25)) with the expressions of rank_score_kernel.  The N' scores of the split
//             chain go to LDS (and to `scores` when it is given);
//   reduce    the first RT_THREADS threads reduce them to a mean and a variance in the order of split_stats_kernel: the same
//             walk_pairs<RT_THREADS, RS_LU>, the same butterfly, the four wavefront sums added in the order 0, 1, 2, 3.
// LDS: 8 P + 8 N' bytes, sized to the group: 72 KB at 4 x 2000 (two workgroups a CU), 96 KB at the limit M = 8192, N' = 4096.
// Every count is an integer and every sum has the order above: the same bits on every call and wherever a group sits in the
// launch.  Nothing here writes `samples`, and `work` is not touched.
#pragma once
#include "diag_rank.hpp"

namespace {

constexpr int RG_THREADS = 512;                    // threads of the workgroup (the reduction uses the first RT_THREADS of them)
constexpr long long RG_MAX_VALUES = 8192;          // largest M of a group: 64 KB of keys and at most 32 KB of scores

inline unsigned int rank_groups_pad(unsigned int M) {   // the power of two the keys of a group are padded to
  unsigned int P = 4u;
  while (P < M) P <<= 1;
  return P;
}

// split_sum of diag_rank.hpp for a workgroup of RG_THREADS threads of which the first RT_THREADS carry a value: the same
// butterfly, the same order of the RT_WAVES wavefront sums.
__device__ __forceinline__ double group_split_sum(double v, double* s_w) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x < RT_THREADS) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = 0.0;
#pragma unroll
  for (int w = 0; w < RT_WAVES; w++) total += s_w[w];
  return total;
}

// (at most 128 registers a thread: two workgroups of eight wavefronts a CU)
__global__ __launch_bounds__(RG_THREADS, 4) void rank_groups_kernel(const double* __restrict__ samples, long long S, int k,
                                                                 long long row0, long long N, long long cpg,
                                                                 const int* __restrict__ cols, int p,
                                                                 const int* __restrict__ active, unsigned int M, unsigned int P,
                                                                 double* __restrict__ scores, double* __restrict__ out) {
  extern __shared__ unsigned long long s_k[];        // [P] keys, then [N'] scores of one split chain
  __shared__ double s_w[RT_WAVES];
  __shared__ double s_med;
  __shared__ unsigned int s_nf;
  const long long g = (long long)blockIdx.x / p;
  const int j = (int)((long long)blockIdx.x % p);
  if (active && active[g] == 0) return;              // (uniform per workgroup: before the first barrier)
  double* s_z = reinterpret_cast<double*>(s_k + P);
  const int tid = threadIdx.x;
  const int col = cols[j];
  const bool col_ok = col >= 0 && col < k;           // (a column outside k reads nothing: its values count as non-finite)
  const unsigned int Nh = (unsigned int)(N / 2), m = (unsigned int)(2 * cpg);
  const double* __restrict__ x0 = samples + (g * cpg * k + (col_ok ? col : 0)) * S + row0;
  auto value = [&](unsigned int e) -> double {       // element e of the group's column, as rank_gather_kernel reads it
    const unsigned int s = e / Nh, r = e - s * Nh;
    const long long row = (s & 1u) ? N - Nh + r : (long long)r;
    return col_ok ? x0[(long long)(s >> 1) * k * S + row] : fmh_nan();
  };
  double* o = out + ((long long)blockIdx.x) * (4LL * m + 2);
  const double denom = (double)M + 0.25;
  if (tid == 0) s_nf = 0u;
  __syncthreads();

  for (int fold = 0; fold < 2; fold++) {
    const double med = fold ? s_med : 0.0;
    // ------------------------------------------------------------------------------------------------------------ gather
    unsigned int nf = 0u;
    for (unsigned int e = tid; e < P; e += RG_THREADS) {
      unsigned long long kx = ~0ull;
      if (e < M) {
        double x = value(e);
        nf += fmh_isfinite(x) ? 0u : 1u;
        if (fold) x = fmh_abs(x - med);
        kx = key_of(x + 0.0);
      }
      s_k[e] = kx;
    }
    if (!fold && nf) atomicAdd(&s_nf, nf);
    __syncthreads();
    // -------------------------------------------------------------------------------------------------------------- sort
    // ascending; pair q of a step = the q-th index with bit jj clear and its partner with bit jj set
    for (unsigned int kk = 2; kk <= P; kk <<= 1) {
      for (unsigned int jj = kk >> 1; jj >= 1; jj >>= 1) {
        for (unsigned int q = tid; q < (P >> 1); q += RG_THREADS) {
          const unsigned int i = ((q & ~(jj - 1u)) << 1) | (q & (jj - 1u)), l = i | jj;
          const unsigned long long a = s_k[i], b = s_k[l];
          const bool up = (i & kk) == 0u;
          if ((a > b) == up) { s_k[i] = b; s_k[l] = a; }
        }
        __syncthreads();
      }
    }
    if (!fold) {
      if (tid == 0) {
        const double md = (value_of(s_k[M / 2 - 1]) + value_of(s_k[M / 2])) / 2.0;
        s_med = md;
        o[4 * m] = (double)s_nf;
        o[4 * m + 1] = md;
      }
      __syncthreads();
    }
    // --------------------------------------------------------------------------------------------------- rank and reduce
    double* zs = scores ? scores + ((long long)blockIdx.x * 2 + fold) * (long long)M : nullptr;
    for (unsigned int s = 0; s < m; s++) {
      for (unsigned int r = tid; r < Nh; r += RG_THREADS) {
        const unsigned int e = s * Nh + r;
        double x = value(e);
        if (fold) x = fmh_abs(x - med);
        const unsigned long long kx = key_of(x + 0.0);
        unsigned int lo = 0u, hi = M;                // #less: the first position whose key is not below kx
        while (lo < hi) {
          const unsigned int mid = (lo + hi) >> 1;
          if (s_k[mid] < kx) lo = mid + 1u; else hi = mid;
        }
        const unsigned int less = lo;
        hi = M;                                      // #less-or-equal: the first position whose key is above kx
        while (lo < hi) {
          const unsigned int mid = (lo + hi) >> 1;
          if (s_k[mid] <= kx) lo = mid + 1u; else hi = mid;
        }
        const double twice = (double)((unsigned long long)less + (unsigned long long)lo + 1ull);   // 2 #less + #equal + 1
        const double z = fmh_qnorm((0.5 * twice - 0.375) / denom);
        s_z[r] = z;
        if (zs) zs[e] = z;
      }
      __syncthreads();
      // split_stats_kernel on the Nh scores in LDS, by the first RT_THREADS threads
      double acc = 0.0;
      if (tid < RT_THREADS)
        walk_pairs<RT_THREADS, RS_LU>(s_z, (long long)Nh, [&](long long, double a, double b, bool has_b) { acc += a; if (has_b) acc += b; });
      const double mean = group_split_sum(acc, s_w) / (double)(long long)Nh;
      acc = 0.0;
      if (tid < RT_THREADS)
        walk_pairs<RT_THREADS, RS_LU>(s_z, (long long)Nh, [&](long long, double a, double b, bool has_b) {
          const double da = a - mean;
          acc += da * da;
          if (has_b) { const double db = b - mean; acc += db * db; }
        });
      const double var = group_split_sum(acc, s_w) / (double)((long long)Nh - 1);
      if (tid == 0) { o[2 * m * fold + 2 * s] = mean; o[2 * m * fold + 2 * s + 1] = var; }
      __syncthreads();                               // (s_z and s_w are written again)
    }
  }
}

}  // namespace

extern "C" {

int64_t fmcmc_rank_groups_max_values(void) { return RG_MAX_VALUES; }

int64_t fmcmc_rank_rhat_groups_work_len(int64_t ngroups, int64_t chains_per_group, int32_t p, int64_t N) {
  if (ngroups < 1 || chains_per_group < 1 || p < 1 || N < 4) return 0;
  if (chains_per_group > RG_MAX_VALUES || 2 * chains_per_group * (N / 2) > RG_MAX_VALUES) return 0;
  if (ngroups > 0x7fffffffLL / p) return 0;
  return 1;                                          // (everything lives in LDS; 0 stays the answer to bad arguments)
}

int fmcmc_rank_rhat_groups_dev(const double* samples, int64_t ngroups, int64_t chains_per_group, int32_t k, int64_t S, int64_t row0,
                               int64_t N, const int32_t* cols, int32_t p, const int32_t* active, double* work, double* scores,
                               double* out, void* hip_stream) {
  const char* who = "fmcmc_rank_rhat_groups_dev";
  if (!samples || !cols || !work || !out) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (ngroups < 1 || chains_per_group < 1)
    return fail(FMCMC_ERR_ARG, "%s: ngroups = %lld, chains_per_group = %lld: each must be at least 1", who, (long long)ngroups,
                (long long)chains_per_group);
  int rc = rank_check(who, samples, cols, work, out, chains_per_group, k, S, row0, N, p);   // (the 2^32 limit: of one group)
  if (rc != FMCMC_OK) return rc;
  const long long Mll = 2 * chains_per_group * (N / 2);
  if (Mll > RG_MAX_VALUES)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: 2 x %lld split chains of %lld rows are %lld values in a group; a group's keys are "
                "sorted in LDS, at most %lld of them -- fmcmc_rank_rhat_dev per group is the form for larger groups", who,
                (long long)chains_per_group, (long long)(N / 2), Mll, RG_MAX_VALUES);
  if (ngroups > 0x7fffffffLL / p || chains_per_group > 0x7fffffffLL / ngroups)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld groups x %lld chains x %d columns exceed one launch", who, (long long)ngroups,
                (long long)chains_per_group, (int)p);
  hipStream_t st = (hipStream_t)hip_stream;
  const unsigned int M = (unsigned int)Mll, P = rank_groups_pad(M);
  const size_t lds = (size_t)P * sizeof(unsigned long long) + (size_t)(N / 2) * sizeof(double);
  rc = allow_lds(who, rank_groups_kernel, lds);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(rank_groups_kernel, dim3((unsigned)(ngroups * p)), dim3(RG_THREADS), lds, st, samples, (long long)S, (int)k,
                     (long long)row0, (long long)N, (long long)chains_per_group, cols, (int)p, active, M, P, scores, out);
  return rank_launched(who);
}

}  // extern "C"
