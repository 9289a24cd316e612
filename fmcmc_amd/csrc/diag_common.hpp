// diag_common.hpp — what the device diagnostics share (summary.hip, raftery.hip, gelman.hip): the error text, the pair load, the
// order-preserving keys of the radix selects, the window checks of the windowed entries, the walk over one series and the
// one-workgroup radix select over the segments of a column (raftery.hip: one series; summary.hip: the chains of a group).  Kernels,
// reductions and the multi-workgroup select of fmcmc_summary_dev stay in their units.  Everything here is local to the unit that
// includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdio.h>
#include <stdarg.h>

#include "../../include/fmcmc_amd.h"
#include "../../include/fmh_detmath.h"

extern "C" void fmcmc_set_error_text_(const char* text);   // mh_engine.hip: the buffer behind fmcmc_last_error()

namespace {

constexpr int MAXM = 64;            // largest AR order (coda: floor(10 log10 N)); it bounds the rows of every window: N < 10^6.5
constexpr int LDS_ROWS = 19456;     // rows of a series staged in LDS at once (152 KB of the 160 KB; summary.hip adds its scratch)

inline int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  fmcmc_set_error_text_(buf);
  return code;
}

// Two consecutive rows of a column.  A pair is 8-byte aligned only: a window starts at any row of a history whose row stride may
// be odd.  The vector type says so; the load is still one global_load_dwordx4, which gfx950 serves at any 4-byte alignment.
typedef double dpair_t __attribute__((ext_vector_type(2), aligned(8)));

// Order-preserving 64-bit keys: x < y <=> key_of(x) < key_of(y), and value_of(key_of(x)) has the bits of x.
__device__ __forceinline__ unsigned long long key_of(double x) {
  const unsigned long long u = fmh_d2u(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(unsigned long long kx) {
  return fmh_u2d((kx >> 63) ? (kx & 0x7fffffffffffffffull) : ~kx);
}
// Pass d of a most-significant-digit radix select (8 passes of 8 bits) fixes bits [56 - 8 d, 64 - 8 d) of a key: its digit, and
// the bits above it, which are compared with the prefix found so far.
__device__ __forceinline__ unsigned int radix_digit(unsigned long long kx, int d) { return (unsigned int)(kx >> (56 - 8 * d)) & 255u; }
__device__ __forceinline__ unsigned long long radix_high(unsigned long long kx, int d) { return d == 0 ? 0ull : kx >> (64 - 8 * d); }

// One thread's share of a walk over the N rows of the series x by a workgroup of T threads: batches of 2 LU T rows, thread t
// takes the pairs t, t + T, ... of a batch.  The LU pair loads of a batch are issued back to back before the first use; then
// rows(i, x[i], x[i + 1], has_b) is called for pair 0, pair 1, ... of the batch, batch after batch, and takes x[i] before
// x[i + 1].  An odd last row comes with has_b false and 0.0 in place of x[i + 1].  (Stage 1 of summary_series_kernel is this
// loop written out: see there.)
template <int T, int LU, typename Rows>
__device__ __forceinline__ void walk_pairs(const double* __restrict__ x, long long N, Rows rows) {
  const int tid = threadIdx.x;
  for (long long base = 0; base < N; base += 2LL * LU * T) {
    double a[LU], b[LU];
#pragma unroll
    for (int u = 0; u < LU; u++) {
      const long long i = base + 2LL * (u * T + tid);
      a[u] = 0.0; b[u] = 0.0;
      if (i + 1 < N) {
        const dpair_t v = *reinterpret_cast<const dpair_t*>(x + i);
        a[u] = v[0]; b[u] = v[1];
      } else if (i < N) {
        a[u] = x[i];
      }
    }
#pragma unroll
    for (int u = 0; u < LU; u++) {
      const long long i = base + 2LL * (u * T + tid);
      if (i < N) rows(i, a[u], b[u], i + 1 < N);
    }
  }
}

inline long long ar_order_max(long long N) {
  const long long m = (long long)floor(10.0 * log10((double)N));
  return m < N - 1 ? m : N - 1;
}

// The checks every windowed entry makes of the window [row0, row0 + N) of nchains x p series and of its four buffers.  An entry
// calls this first and goes on with the checks of its own arguments; all of them come before the first device call.
inline int check_window(const char* who, const void* samples, const void* cols, const void* work, const void* out, int64_t nchains,
                        int32_t k, int64_t S, int64_t row0, int64_t N, int32_t p) {
  if (!samples || !cols || !work || !out) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (nchains < 1) return fail(FMCMC_ERR_ARG, "%s: nchains = %lld, need at least one chain", who, (long long)nchains);
  if (k < 1) return fail(FMCMC_ERR_ARG, "%s: k = %d, need at least one parameter", who, (int)k);
  if (p < 1) return fail(FMCMC_ERR_ARG, "%s: p = %d, need at least one column", who, (int)p);
  if (N < 3) return fail(FMCMC_ERR_ARG, "%s: a window of N = %lld rows is too short: shorter than 3 rows", who, (long long)N);
  if (row0 < 0 || row0 + N > S)
    return fail(FMCMC_ERR_ARG, "%s: the window [%lld, %lld) is outside the %lld rows of a chain", who, (long long)row0,
                (long long)(row0 + N), (long long)S);
  if (ar_order_max(N) > MAXM)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: N = %lld rows per chain ask for an AR order up to %lld; supported are orders up to %d "
                "(N < 3162278)", who, (long long)N, ar_order_max(N), MAXM);
  if (nchains > 0x7fffffffLL / p)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld chains x %d columns exceed one launch", who, (long long)nchains, (int)p);
  return FMCMC_OK;
}

// The 0-based ranks of x_(lo), x_(hi) of R's quantile type 7 among n values, clamped to [0, n - 1]: index = 1 + (n - 1) prob,
// lo = floor(index), hi = ceil(index) (1-based); the quantile is (1 - h) x_(lo) + h x_(hi) where `between`, else x_(lo).
struct Type7 { long long lo, hi; int between; double h; };
inline Type7 type7_ranks(long long n, double prob) {
  const double index = 1.0 + (double)(n - 1) * prob, flo = floor(index);
  const long long lo = (long long)flo - 1, hi = (long long)ceil(index) - 1;
  return {lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo), hi < 0 ? 0 : (hi > n - 1 ? n - 1 : hi), (int)(index > flo), index - flo};
}

template <typename Kernel>
inline int allow_lds(const char* who, Kernel kernel, size_t lds) {   // dynamic LDS beyond the 64 KB a kernel gets unasked
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return fail(FMCMC_ERR_DEVICE, "%s: %zu bytes of LDS refused", who, lds);
  return FMCMC_OK;
}

// --------------------------------------------------------------------------------------- the one-workgroup radix select
// Exact order statistics of the values of `nseg` segments of N rows each (segment c starts at x + c seg_stride; one series is
// one segment) by a workgroup of SEL_T threads: most-significant-digit radix select on the keys, 8 passes of 8 bits, the
// histograms in LDS.  Targets with the same prefix share one histogram (that of their "leader"), SEL_HG leaders are counted per
// walk over the values; while all nseg N keys fit in LDS (<= LDS_ROWS) they are staged there once, segment c at s_k + c N, else
// every walk re-reads the segments through walk_pairs.  Every count is an integer: neither the arrival order of the LDS
// atomics nor the launch changes a result.
constexpr int SEL_T = 512;          // threads of the workgroup
constexpr int SEL_RANKS = 32;       // targets per call: 2 x SUMMARY_MAX_PROBS
constexpr int SEL_HG = 4;           // histograms (leaders) per walk over the values
constexpr int SEL_LU = 4;           // pairs in flight per thread

struct OrderRanks { unsigned int r[SEL_RANKS]; };   // 0-based, each < nseg N < 2^32

struct SelectLds {
  unsigned int hist[SEL_HG][256];                   // counts of a walk, then their exclusive prefix sums
  unsigned long long prefix[SEL_RANKS];             // per target: the key bits fixed so far
  unsigned int rank[SEL_RANKS];                     // per target: its rank among the values that share its prefix
  int slot[SEL_RANKS];                              // per target: the position of its leader in `list`
  int list[SEL_RANKS];                              // the leaders of this pass
  int nlead;
  unsigned int nf;                                  // non-finite values of all segments
};

// Reads every segment once: counts the non-finite values of all of them into L.nf and, when `staged`, leaves key_of(row i of
// segment c) in s_k[c N + i].
__device__ __forceinline__ void stage_series(const double* __restrict__ x, long long N, long long nseg, long long seg_stride,
                                             bool staged, unsigned long long* s_k, SelectLds& L) {
  if (threadIdx.x == 0) L.nf = 0u;
  __syncthreads();
  unsigned int nf = 0u;
  for (long long c = 0; c < nseg; c++) {
    unsigned long long* kc = s_k + c * N;
    walk_pairs<SEL_T, SEL_LU>(x + c * seg_stride, N, [&](long long i, double a, double b, bool has_b) {
      nf += fmh_isfinite(a) ? 0u : 1u;
      if (staged) kc[i] = key_of(a);
      if (has_b) {
        nf += fmh_isfinite(b) ? 0u : 1u;
        if (staged) kc[i + 1] = key_of(b);
      }
    });
  }
  if (nf) atomicAdd(&L.nf, nf);
  __syncthreads();
}

// Radix select of the nt targets whose ranks (among the nseg N values) are in L.rank (L.prefix zeroed): on return L.prefix[t] is
// the key of the order statistic of target t.  Every thread of the workgroup calls it; it starts and ends with a barrier.
__device__ __forceinline__ void select_series(const double* __restrict__ x, long long N, long long nseg, long long seg_stride,
                                              bool staged, const unsigned long long* s_k, int nt, SelectLds& L) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int pass = 0; pass < 8; pass++) {
    __syncthreads();
    if (tid == 0) {                                  // leaders: the first target of every distinct prefix
      int n = 0;
      for (int t = 0; t < nt; t++) {
        int l = t;
        for (int u = 0; u < t; u++)
          if (L.prefix[u] == L.prefix[t]) { l = u; break; }
        if (l == t) { L.slot[t] = n; L.list[n] = t; n++; }
        else L.slot[t] = L.slot[l];
      }
      L.nlead = n;
    }
    __syncthreads();
    const int nlead = L.nlead;
    for (int g0 = 0; g0 < nlead; g0 += SEL_HG) {
      const int ng = nlead - g0 < SEL_HG ? nlead - g0 : SEL_HG;
      unsigned long long pg[SEL_HG];
#pragma unroll
      for (int g = 0; g < SEL_HG; g++) pg[g] = L.prefix[L.list[g0 + (g < ng ? g : 0)]];
      for (int e = tid; e < SEL_HG * 256; e += SEL_T) (&L.hist[0][0])[e] = 0u;
      __syncthreads();
      auto count = [&](unsigned long long kx) {
        const unsigned long long high = radix_high(kx, pass);
        const unsigned int digit = radix_digit(kx, pass);
#pragma unroll
        for (int g = 0; g < SEL_HG; g++)
          if (g < ng && high == pg[g]) atomicAdd(&L.hist[g][digit], 1u);
      };
      if (staged) {
        for (int i = tid; i < (int)(nseg * N); i += SEL_T) count(s_k[i]);
      } else {
        for (long long c = 0; c < nseg; c++)
          walk_pairs<SEL_T, SEL_LU>(x + c * seg_stride, N,
                                    [&](long long, double a, double b, bool has_b) { count(key_of(a)); if (has_b) count(key_of(b)); });
      }
      __syncthreads();
      if (wave < ng) {                               // one wavefront per histogram: exclusive prefix sums, four bins a lane
        unsigned int* h = &L.hist[wave][4 * lane];
        const unsigned int c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
        const unsigned int mine = c0 + c1 + c2 + c3;
        unsigned int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned int up = __shfl_up(incl, o, 64);
          if (lane >= o) incl += up;
        }
        const unsigned int excl = incl - mine;
        h[0] = excl; h[1] = excl + c0; h[2] = excl + c0 + c1; h[3] = excl + c0 + c1 + c2;
      }
      __syncthreads();
      if (tid < nt && L.slot[tid] >= g0 && L.slot[tid] < g0 + ng) {
        // the bin that holds the rank: the largest b whose exclusive sum is <= rank (the rank is below the total, so that
        // bin is not empty).  Only targets of this group change, and no later group of the pass reads their prefixes.
        const unsigned int* cum = L.hist[L.slot[tid] - g0];
        const unsigned int r = L.rank[tid];
        int b = 0;
#pragma unroll
        for (int step = 128; step >= 1; step >>= 1)
          if (cum[b + step] <= r) b += step;
        L.prefix[tid] = (L.prefix[tid] << 8) | (unsigned long long)b;
        L.rank[tid] = r - cum[b];
      }
      __syncthreads();
    }
  }
}

}  // namespace
