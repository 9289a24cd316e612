// raftery.hip — order statistics of every (chain, column) series on its own, and the device part of coda::raftery.diag
// (the algorithm is restated in fmcmc_amd/convergence.py: raftery_diag, and in INTEGRATION.md).
//
// One chain's column is N contiguous doubles (samples + (c k + col) S + row0), as in summary.hip.  One workgroup per series:
//   1. stage        the series is read once with 8-byte-aligned pair loads, its non-finite values are counted, and while it fits
//                   (N <= LDS_ROWS, the tile of summary_series_kernel) its order-preserving keys are kept in LDS;
//   2. select       exact order statistics at up to 32 ranks by the one-workgroup radix select of diag_common.hpp
//                   (stage_series / select_series, here over one segment: the series); a series too long for LDS is re-read
//                   every walk;
//   3. raftery      u = type-7 quantile from the two order statistics (two rounded products, one rounded sum), the indicator
//                   Z_t = (x_t <= u) bit-packed into `work` by wave ballots, then per thinning j (one wavefront each) the
//                   2x2x2 table of the consecutive triples of Z at rows 0, j, 2j, ... and its last pair.
//   4. hpd         coda::HPDinterval of a series (chain_hpd_kernel): the shortest interval between x_(i) and x_(i + gap) uses the
//                   T = N - gap smallest and the T largest values alone; the two order statistics that bound them are selected,
//                   both tails are compacted into LDS, sorted there, and the T widths are reduced to their first minimum.
// Every count is an integer, so neither the arrival order of the LDS atomics nor the launch changes a result.  Nothing here
// writes `samples`.
#include "diag_common.hpp"
#include "diag_rank.hpp"            // the sort through HBM, the pooled ranks and the split R-hat entries (fmcmc_rank_*)
#include "diag_ess.hpp"             // on top of it: the all-lag autocovariances and the bulk / tail ESS (fmcmc_rank_ess_*)
#include "diag_rank_groups.hpp"     // the split R-hat of many small groups of chains, sorted in LDS (fmcmc_rank_rhat_groups_*)
#include "diag_ess_groups.hpp"      // the bulk / tail ESS of many small groups, one workgroup a (group, column) (fmcmc_rank_ess_groups_*)

namespace {

constexpr int OT = SEL_T;           // threads of a series workgroup: that of the select (diag_common.hpp)
constexpr int OW = OT / 64;
constexpr int MAXRANKS = SEL_RANKS; // targets per call
constexpr int MAXNJ = 32;           // thinnings per launch
constexpr int LU = SEL_LU;          // pairs in flight per thread
constexpr int HEAD = 4;             // doubles per series at the head of the raftery output: u, x_(lo), x_(hi), non-finite count
constexpr int CNT = 10;             // integers per (series, thinning): T[a][b][c] at 4 a + 2 b + c, then Z_{m-2}, Z_{m-1}
constexpr int HPD_MAX_TAIL = 8192;  // rows of each tail of chain_hpd_kernel held in LDS (two tails of 64 KB)
constexpr int HPD_OUT = 4;          // doubles per series of the hpd output: lower, upper, i*, non-finite count

__global__ __launch_bounds__(OT) void chain_order_kernel(const double* __restrict__ samples, long long S, int k, long long row0,
                                                         long long N, const int* __restrict__ cols, int p, int nt,
                                                         OrderRanks ranks, int staged, double* __restrict__ nf_out,
                                                         double* __restrict__ out) {
  extern __shared__ unsigned long long s_k[];        // [N] when staged
  __shared__ SelectLds L;
  const int tid = threadIdx.x;
  const long long series = blockIdx.x, c = series / p;
  const int j = (int)(series % p);
  const double* __restrict__ x = samples + (c * (long long)k + cols[j]) * S + row0;
  stage_series(x, N, 1, 0, staged != 0, s_k, L);
  if (tid < nt) { L.prefix[tid] = 0ull; L.rank[tid] = ranks.r[tid]; }
  select_series(x, N, 1, 0, staged != 0, s_k, nt, L);
  if (tid < nt) out[series * nt + tid] = value_of(L.prefix[tid]);
  if (tid == 0) nf_out[series] = (double)L.nf;
}

__device__ __forceinline__ unsigned int bit_at(const unsigned long long* bits, long long row) {
  return (unsigned int)(bits[row >> 6] >> (row & 63)) & 1u;
}

__global__ __launch_bounds__(OT) void raftery_kernel(const double* __restrict__ samples, long long S, int k, long long row0,
                                                     long long N, const int* __restrict__ cols, int p, unsigned int rank_lo,
                                                     unsigned int rank_hi, int interpolate, double h, long long j0, int nj,
                                                     int staged, unsigned long long* bits_all, long long words,
                                                     double* __restrict__ head, long long* __restrict__ counts) {
  extern __shared__ unsigned long long s_k[];        // [N] when staged
  __shared__ SelectLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long series = blockIdx.x, c = series / p;
  const int col = (int)(series % p);
  const double* __restrict__ x = samples + (c * (long long)k + cols[col]) * S + row0;
  stage_series(x, N, 1, 0, staged != 0, s_k, L);
  if (tid < 2) { L.prefix[tid] = 0ull; L.rank[tid] = tid ? rank_hi : rank_lo; }
  select_series(x, N, 1, 0, staged != 0, s_k, 2, L);
  // the threshold: summary.type7_quantiles, operation for operation (two rounded products, one rounded sum)
  const double xlo = value_of(L.prefix[0]), xhi = value_of(L.prefix[1]);
  const double u = (interpolate && xhi != xlo) ? __dadd_rn(__dmul_rn(1.0 - h, xlo), __dmul_rn(h, xhi)) : xlo;
  // the indicator, 64 rows a word: the ballot of a wavefront over 64 consecutive rows (the IEEE comparison on the values)
  unsigned long long* bits = bits_all + series * words;   // (written, then read by other wavefronts: no __restrict__)
  for (long long base = (long long)wave * 64; base < N; base += OT) {
    const long long i = base + lane;
    double v = 0.0;
    if (i < N) v = staged ? value_of(s_k[i]) : x[i];
    const unsigned long long w = __ballot(i < N && v <= u);
    if (lane == 0) bits[base >> 6] = w;
  }
  if (tid == 0) {
    double* o = head + series * HEAD;
    o[0] = u; o[1] = xlo; o[2] = xhi; o[3] = (double)L.nf;
  }
  __threadfence_block();
  __syncthreads();
  // counts: one wavefront per thinning; lane l takes the triples l, l + 64, ... and keeps the eight counts in 16-bit fields
  // (a lane sees fewer than N / 64 < 2^16 triples)
  for (int jj = wave; jj < nj; jj += OW) {
    const long long j = j0 + jj, m = (N + j - 1) / j, ntri = m >= 3 ? m - 2 : 0;
    unsigned long long lo = 0ull, hi = 0ull;
    for (long long i = lane; i < ntri; i += 64) {
      const unsigned int a = bit_at(bits, i * j), b = bit_at(bits, (i + 1) * j), cc = bit_at(bits, (i + 2) * j);
      const unsigned long long inc = 1ull << (16 * (2 * b + cc));
      lo += a ? 0ull : inc;
      hi += a ? inc : 0ull;
    }
    unsigned int cnt[8];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      cnt[e] = (unsigned int)(lo >> (16 * e)) & 0xffffu;
      cnt[4 + e] = (unsigned int)(hi >> (16 * e)) & 0xffffu;
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) cnt[e] += __shfl_xor(cnt[e], o, 64);
    }
    if (lane == 0) {
      long long* o = counts + (series * nj + jj) * CNT;
#pragma unroll
      for (int e = 0; e < 8; e++) o[e] = (long long)cnt[e];
      o[8] = m >= 2 ? (long long)bit_at(bits, (m - 2) * j) : 0LL;
      o[9] = (long long)bit_at(bits, (m - 1) * j);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------- HPD
// coda::HPDinterval of one series: with x_(0) <= .. <= x_(N-1), the first minimum over i = 0 .. T - 1 (T = N - gap) of
// x_(i + gap) - x_(i).  Only x_(0) .. x_(T-1) (the low tail) and x_(gap) .. x_(N-1) (the high tail) enter, T values each; where
// gap < T the two overlap.  The keys of x_(T-1) and x_(gap) are selected; one more walk copies into each tail the keys strictly
// beyond its threshold (fewer than T: the threshold itself has a rank inside the tail) in the order they arrive, the rest of the
// T slots take the threshold key (ties are equal values), the slots up to the power of two P the maximum key; both tails are
// sorted by a bitonic network over P keys, which ends the dependence on the arrival order.  Then thread t forms the widths
// t, t + OT, ... (one float64 subtraction each) and keeps its first minimum; (width, index) pairs are joined lexicographically.
__global__ __launch_bounds__(OT) void chain_hpd_kernel(const double* __restrict__ samples, long long S, int k, long long row0,
                                                       long long N, const int* __restrict__ cols, int p, unsigned int gap,
                                                       int P, double* __restrict__ thresholds, double* __restrict__ out) {
  extern __shared__ unsigned long long s_k[];        // [2][P]: the low tail, the high tail
  __shared__ SelectLds L;
  __shared__ unsigned int s_n[2];                    // keys strictly beyond the threshold copied so far, per tail
  __shared__ double s_w[OW];
  __shared__ unsigned int s_i[OW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long series = blockIdx.x, c = series / p;
  const int col = (int)(series % p);
  const double* __restrict__ x = samples + (c * (long long)k + cols[col]) * S + row0;
  const unsigned int T = (unsigned int)N - gap;      // 1 <= T <= P <= HPD_MAX_TAIL
  unsigned long long* lo = s_k;
  unsigned long long* hi = s_k + P;
  stage_series(x, N, 1, 0, false, s_k, L);
  if (tid < 2) { L.prefix[tid] = 0ull; L.rank[tid] = tid ? gap : T - 1u; s_n[tid] = 0u; }
  select_series(x, N, 1, 0, false, s_k, 2, L);
  const unsigned long long klo = L.prefix[0], khi = L.prefix[1];
  walk_pairs<OT, LU>(x, N, [&](long long, double a, double b, bool has_b) {
    auto put = [&](unsigned long long kx) {
      if (kx < klo) { const unsigned int at = atomicAdd(&s_n[0], 1u); if (at < T) lo[at] = kx; }
      if (kx > khi) { const unsigned int at = atomicAdd(&s_n[1], 1u); if (at < T) hi[at] = kx; }
    };
    put(key_of(a));
    if (has_b) put(key_of(b));
  });
  __syncthreads();
  {
    const unsigned int nlo = s_n[0] < T ? s_n[0] : T, nhi = s_n[1] < T ? s_n[1] : T;
    for (unsigned int i = tid; i < (unsigned int)P; i += OT) {
      if (i >= nlo) lo[i] = i < T ? klo : ~0ull;
      if (i >= nhi) hi[i] = i < T ? khi : ~0ull;
    }
  }
  __syncthreads();
  // bitonic sort of both tails, ascending: P / 2 compare-exchanges per tail and step, pair q of a step = the q-th index with
  // bit j clear and its partner with bit j set
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j >= 1; j >>= 1) {
      for (int q = tid; q < P; q += OT) {            // q < P / 2: the low tail; beyond: the high tail
        unsigned long long* t = q < (P >> 1) ? lo : hi;
        const int r = q & ((P >> 1) - 1);
        const int i = ((r & ~(j - 1)) << 1) | (r & (j - 1)), l = i | j;
        const unsigned long long a = t[i], b = t[l];
        const bool up = (i & kk) == 0;
        if ((a > b) == up) { t[i] = b; t[l] = a; }
      }
      __syncthreads();
    }
  }
  // widths and their first minimum.  (Infinite widths compare equal: the first of them wins, as which.min has it.)
  double bw = 0.0;
  unsigned int bi = 0xffffffffu;
  for (unsigned int i = tid; i < T; i += OT) {
    const double w = value_of(hi[i]) - value_of(lo[i]);
    if (bi == 0xffffffffu || w < bw) { bw = w; bi = i; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ow = __shfl_xor(bw, o, 64);
    const unsigned int oi = __shfl_xor(bi, o, 64);
    if (oi != 0xffffffffu && (bi == 0xffffffffu || ow < bw || (ow == bw && oi < bi))) { bw = ow; bi = oi; }
  }
  if (lane == 0) { s_w[wave] = bw; s_i[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < OW; w++) {
      const double ow = s_w[w];
      const unsigned int oi = s_i[w];
      if (oi != 0xffffffffu && (bi == 0xffffffffu || ow < bw || (ow == bw && oi < bi))) { bw = ow; bi = oi; }
    }
    if (bi >= T) bi = 0u;                            // (a NaN width in every slot: the call is refused for its non-finite rows)
    double* o = out + series * HPD_OUT;
    o[0] = value_of(lo[bi]); o[1] = value_of(hi[bi]); o[2] = (double)bi; o[3] = (double)L.nf;
    thresholds[2 * series] = value_of(klo); thresholds[2 * series + 1] = value_of(khi);
  }
}

}  // namespace

extern "C" {

int64_t fmcmc_chain_order_work_len(int64_t nchains, int32_t p, int32_t nranks) {
  if (nchains < 1 || p < 1 || nranks < 1 || nchains > 0x7fffffffLL / p) return 0;
  return nchains * (int64_t)p;
}

int fmcmc_chain_order_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                          const int32_t* cols, int32_t p, const int64_t* ranks, int32_t nranks, double* work, double* out,
                          void* hip_stream) {
  const char* who = "fmcmc_chain_order_dev";
  int rc = check_window(who, samples, cols, work, out, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (!ranks) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (nranks < 1 || nranks > MAXRANKS) return fail(FMCMC_ERR_ARG, "%s: nranks = %d outside [1, %d]", who, (int)nranks, MAXRANKS);
  OrderRanks r;
  for (int t = 0; t < MAXRANKS; t++) {
    if (t < nranks && (ranks[t] < 0 || ranks[t] >= N))
      return fail(FMCMC_ERR_ARG, "%s: ranks[%d] = %lld is outside [0, %lld)", who, t, (long long)ranks[t], (long long)N);
    r.r[t] = (unsigned int)(t < nranks ? ranks[t] : 0);
  }
  hipStream_t st = (hipStream_t)hip_stream;
  const int staged = N <= LDS_ROWS;
  const size_t lds = staged ? (size_t)N * sizeof(unsigned long long) : 0;
  rc = allow_lds(who, chain_order_kernel, lds);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(chain_order_kernel, dim3((unsigned)(nchains * p)), dim3(OT), lds, st, samples, (long long)S, (int)k,
                     (long long)row0, (long long)N, cols, (int)p, (int)nranks, r, staged, work, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

int64_t fmcmc_raftery_work_len(int64_t nchains, int32_t p, int64_t N) {
  if (nchains < 1 || p < 1 || N < 1 || nchains > 0x7fffffffLL / p) return 0;
  return nchains * (int64_t)p * ((N + 63) / 64);
}

int64_t fmcmc_raftery_out_len(int64_t nchains, int32_t p, int32_t nj) {
  if (nchains < 1 || p < 1 || nj < 1 || nj > MAXNJ || nchains > 0x7fffffffLL / p) return 0;
  return nchains * (int64_t)p * (HEAD + (int64_t)nj * CNT);
}

int fmcmc_raftery_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                      const int32_t* cols, int32_t p, double q, int64_t j0, int32_t nj, double* work, double* out,
                      void* hip_stream) {
  const char* who = "fmcmc_raftery_dev";
  int rc = check_window(who, samples, cols, work, out, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (!(q >= 0.0 && q <= 1.0)) return fail(FMCMC_ERR_ARG, "%s: q = %g is outside [0, 1]", who, q);
  if (nj < 1 || nj > MAXNJ) return fail(FMCMC_ERR_ARG, "%s: nj = %d outside [1, %d]", who, (int)nj, MAXNJ);
  if (j0 < 1 || j0 > 0x7fffffffLL) return fail(FMCMC_ERR_ARG, "%s: j0 = %lld, the thinnings start at 1", who, (long long)j0);
  const Type7 r = type7_ranks(N, q);                 // on the N rows of one series
  hipStream_t st = (hipStream_t)hip_stream;
  const long long series = nchains * (long long)p;
  const int staged = N <= LDS_ROWS;
  const size_t lds = staged ? (size_t)N * sizeof(unsigned long long) : 0;
  rc = allow_lds(who, raftery_kernel, lds);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(raftery_kernel, dim3((unsigned)series), dim3(OT), lds, st, samples, (long long)S, (int)k, (long long)row0,
                     (long long)N, cols, (int)p, (unsigned int)r.lo, (unsigned int)r.hi, r.between, r.h,
                     (long long)j0, (int)nj, staged, reinterpret_cast<unsigned long long*>(work), (long long)((N + 63) / 64),
                     out, reinterpret_cast<long long*>(out + series * HEAD));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

int64_t fmcmc_hpd_work_len(int64_t nchains, int32_t p) {
  if (nchains < 1 || p < 1 || nchains > 0x7fffffffLL / p) return 0;
  return nchains * (int64_t)p * 2;
}

int fmcmc_hpd_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* cols,
                  int32_t p, int64_t gap, double* work, double* out, void* hip_stream) {
  const char* who = "fmcmc_hpd_dev";
  int rc = check_window(who, samples, cols, work, out, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (gap < 1 || gap > N - 1) return fail(FMCMC_ERR_ARG, "%s: gap = %lld is outside [1, %lld]", who, (long long)gap, (long long)(N - 1));
  const int64_t T = N - gap;
  if (T > HPD_MAX_TAIL)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: N - gap = %lld rows in each tail of a series; at most %d are held in LDS", who,
                (long long)T, HPD_MAX_TAIL);
  int P = 2;                                         // (the sort's pair index needs P / 2 >= 1)
  while (P < T) P <<= 1;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t lds = (size_t)2 * P * sizeof(unsigned long long);
  rc = allow_lds(who, chain_hpd_kernel, lds);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(chain_hpd_kernel, dim3((unsigned)(nchains * p)), dim3(OT), lds, st, samples, (long long)S, (int)k,
                     (long long)row0, (long long)N, cols, (int)p, (unsigned int)gap, P, work, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

}  // extern "C"
