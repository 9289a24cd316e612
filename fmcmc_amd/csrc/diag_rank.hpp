// diag_rank.hpp — a device-wide stable radix sort through HBM, the average ranks of the pooled values of a column and the
// rank-normalised split R-hat of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) on top of them (the definition is
// INTEGRATION.md §2.2; the host restatement is fmcmc_amd/convergence.py: rhat_host).  Included by raftery.hip alone.
//
// A column's window of N rows of C chains is m = 2 C split chains of N' = floor(N / 2) rows: M = m N' values, element
// e = s N' + r is row r of split chain s.  The columns of a call are processed one after another on the same `work`:
//   gather    e -> (key, e): key_of(x + 0.0) (bulk) or key_of(|x - med| + 0.0) (fold), one tile of RT elements a workgroup; the
//             same walk counts the non-finite values and adds the tile's digit counts of all 8 bytes to one 8 x 256 table
//             (integer atomics);
//   plan      one workgroup: a byte whose table row holds M in one bin is the same in every key, its pass is skipped; the
//             buffer (A or B) each remaining pass reads from follows;
//   sort      least-significant-digit first, per pass that is not skipped: tile_hist (digit counts of every tile into
//             table[digit][tile]), scan_rows (one workgroup a digit: exclusive sums along its row, chunks of 256 tiles with a
//             carry, and the digit's total), scatter (a wavefront takes 1024 consecutive elements of the tile in rounds of 64:
//             the lanes that share a digit are found by 8 ballots, the lowest of them advances the wavefront's own counter of
//             the digit, a lane's place is that counter plus the number of lower lanes with its digit: equal digits keep their
//             order);
//   median    med = (x_(M/2 - 1) + x_(M/2)) / 2 from the sorted bulk keys, with the non-finite count into `info`;
//   rank      a run of equal keys starts at a head (i == 0 or key[i] != key[i - 1]).  run_heads leaves every tile's last and
//             first head, run_carry (one workgroup) turns them into the last head before and the first head after every tile,
//             rank_score scans its tile (16 consecutive elements a thread, then the threads of the workgroup) for every element's
//             run [start, end): 2 r = start + end + 1, z = fmh_qnorm((r - 0.375) / (M + 0.25)), written to dest[e];
//   reduce    split_stats: mean and unbiased variance of the N' scores of every split chain, in a fixed order (see there).
// Every count is an integer and every counter with more than one writer is only ever added to, or joined by max / min: no
// result depends on the arrival order of an atomic or on the launch.  Nothing here writes `samples`.
#pragma once
#include "diag_common.hpp"

namespace {

constexpr int RT_THREADS = 256;                    // threads of every workgroup here
constexpr int RT_WAVES = RT_THREADS / 64;
constexpr int RT_PER = 16;                         // elements per thread
constexpr int RT = RT_THREADS * RT_PER;            // elements per tile: 4096
constexpr int RT_WAVE = 64 * RT_PER;               // consecutive elements of a tile that one wavefront scatters
constexpr int RS_LU = 4;                           // pairs in flight per thread of split_stats_kernel

// The head of `work`, in 32-bit words.
constexpr int H_GH = 0;                            // [8][256] digit counts of all M keys, byte b of the key at row b
constexpr int H_TOT = 2048;                        // [256] digit totals of the pass under way (scan_rows -> scatter)
constexpr int H_SKIP = 2304;                       // [8] pass b is skipped
constexpr int H_SRC = 2312;                        // [8] pass b reads buffer A (0) or B (1)
constexpr int H_FINAL = 2320;                      // the buffer that holds the sorted pairs
constexpr int H_NF = 2321;                         // non-finite values of the column's window
constexpr int H_MED = 2324;                        // med, a double (8-byte aligned)
constexpr int H_WORDS64 = 1280;                    // 64-bit words kept for the head

struct RankBufs {
  unsigned int* hdr;
  unsigned long long* key[2];
  unsigned int* idx[2];
  unsigned int* table;                             // [256][ntiles]
  unsigned int* last_head;                         // [ntiles] 1 + the last head of the tile, 0: none
  unsigned int* first_head;                        // [ntiles] the first head of the tile, M: none
  unsigned int* carry_start;                       // [ntiles] 1 + the last head before the tile, 0: none
  unsigned int* carry_end;                         // [ntiles] the first head after the tile, M: none
  double* z;                                       // [M]
};

inline long long rank_tiles(long long M) { return (M + RT - 1) / RT; }
inline long long rank_work_words(long long M) {
  const long long nt = rank_tiles(M);
  return H_WORDS64 + 2 * M + 2 * ((M + 1) / 2) + 128 * nt + 4 * ((nt + 1) / 2) + M;
}
inline RankBufs rank_bufs(double* work, long long M) {
  const long long nt = rank_tiles(M), half = (M + 1) / 2, th = (nt + 1) / 2;
  unsigned long long* w = reinterpret_cast<unsigned long long*>(work);
  RankBufs b;
  b.hdr = reinterpret_cast<unsigned int*>(w); w += H_WORDS64;
  b.key[0] = w; w += M;
  b.key[1] = w; w += M;
  b.idx[0] = reinterpret_cast<unsigned int*>(w); w += half;
  b.idx[1] = reinterpret_cast<unsigned int*>(w); w += half;
  b.table = reinterpret_cast<unsigned int*>(w); w += 128 * nt;
  b.last_head = reinterpret_cast<unsigned int*>(w); w += th;
  b.first_head = reinterpret_cast<unsigned int*>(w); w += th;
  b.carry_start = reinterpret_cast<unsigned int*>(w); w += th;
  b.carry_end = reinterpret_cast<unsigned int*>(w); w += th;
  b.z = reinterpret_cast<double*>(w);
  return b;
}

// Exclusive prefix sum of one value a thread over the RT_THREADS threads of the workgroup; *total is the sum of all.  s: RT_WAVES
// words of LDS.  Starts and ends with a barrier.
__device__ __forceinline__ unsigned int block_excl_sum(unsigned int v, unsigned int* s, unsigned int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  __syncthreads();
  if (lane == 63) s[wave] = incl;
  __syncthreads();
  unsigned int before = 0u, all = 0u;
#pragma unroll
  for (int w = 0; w < RT_WAVES; w++) {
    const unsigned int t = s[w];
    if (w < wave) before += t;
    all += t;
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// ------------------------------------------------------------------------------------------------------------------ gather
__global__ __launch_bounds__(RT_THREADS) void rank_gather_kernel(const double* __restrict__ samples, long long S, int k,
                                                                 long long row0, long long N, const int* __restrict__ cols,
                                                                 int j, int fold, unsigned int M, unsigned int* hdr,
                                                                 unsigned long long* __restrict__ key,
                                                                 unsigned int* __restrict__ idx) {
  __shared__ unsigned int s_h[8][256];
  const int tid = threadIdx.x;
  for (int e = tid; e < 8 * 256; e += RT_THREADS) (&s_h[0][0])[e] = 0u;
  __syncthreads();
  const int col = cols[j];
  const bool col_ok = col >= 0 && col < k;           // (a column outside k reads nothing: its values count as non-finite)
  const unsigned int Nh = (unsigned int)(N / 2);
  const double med = fold ? *reinterpret_cast<const double*>(hdr + H_MED) : 0.0;
  unsigned int nf = 0u;
#pragma unroll 4
  for (int u = 0; u < RT_PER; u++) {
    const unsigned long long e = (unsigned long long)blockIdx.x * RT + (unsigned long long)u * RT_THREADS + tid;
    if (e < M) {
      const unsigned int s = (unsigned int)e / Nh, r = (unsigned int)e - s * Nh;
      const long long row = row0 + ((s & 1u) ? N - Nh + r : (long long)r);
      double x = col_ok ? samples[((long long)(s >> 1) * k + col) * S + row] : fmh_nan();
      nf += fmh_isfinite(x) ? 0u : 1u;
      if (fold) x = fmh_abs(x - med);
      const unsigned long long kx = key_of(x + 0.0);
      key[e] = kx;
      idx[e] = (unsigned int)e;
#pragma unroll
      for (int b = 0; b < 8; b++) atomicAdd(&s_h[b][(unsigned int)(kx >> (8 * b)) & 255u], 1u);
    }
  }
  __syncthreads();
  for (int e = tid; e < 8 * 256; e += RT_THREADS) {
    const unsigned int c = (&s_h[0][0])[e];
    if (c) atomicAdd(hdr + H_GH + e, c);
  }
  if (!fold) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) nf += __shfl_xor(nf, o, 64);
    if ((tid & 63) == 0 && nf) atomicAdd(hdr + H_NF, nf);
  }
}

__global__ __launch_bounds__(RT_THREADS) void rank_plan_kernel(unsigned int* hdr, unsigned int M) {
  __shared__ unsigned int s_skip[8];
  const int tid = threadIdx.x;
  if (tid < 8) s_skip[tid] = 0u;
  __syncthreads();
  for (int b = 0; b < 8; b++)
    if (hdr[H_GH + b * 256 + tid] == M) atomicOr(&s_skip[b], 1u);
  __syncthreads();
  if (tid == 0) {
    unsigned int cur = 0u;
    for (int b = 0; b < 8; b++) {
      hdr[H_SKIP + b] = s_skip[b];
      hdr[H_SRC + b] = cur;
      if (!s_skip[b]) cur ^= 1u;
    }
    hdr[H_FINAL] = cur;
  }
}

// -------------------------------------------------------------------------------------------------------------------- sort
__global__ __launch_bounds__(RT_THREADS) void rank_tile_hist_kernel(const unsigned int* __restrict__ hdr,
                                                                    const unsigned long long* keyA,
                                                                    const unsigned long long* keyB, unsigned int M,
                                                                    unsigned int ntiles, int pass,
                                                                    unsigned int* __restrict__ table) {
  __shared__ unsigned int s_h[256];
  if (hdr[H_SKIP + pass]) return;
  const unsigned long long* __restrict__ key = hdr[H_SRC + pass] ? keyB : keyA;
  const int tid = threadIdx.x;
  s_h[tid] = 0u;
  __syncthreads();
#pragma unroll 4
  for (int u = 0; u < RT_PER; u++) {
    const unsigned long long e = (unsigned long long)blockIdx.x * RT + (unsigned long long)u * RT_THREADS + tid;
    if (e < M) atomicAdd(&s_h[(unsigned int)(key[e] >> (8 * pass)) & 255u], 1u);
  }
  __syncthreads();
  table[(unsigned long long)tid * ntiles + blockIdx.x] = s_h[tid];
}

__global__ __launch_bounds__(RT_THREADS) void rank_scan_rows_kernel(unsigned int* hdr, unsigned int ntiles, int pass,
                                                                    unsigned int* table) {
  __shared__ unsigned int s_w[RT_WAVES];
  if (hdr[H_SKIP + pass]) return;
  unsigned int* row = table + (unsigned long long)blockIdx.x * ntiles;
  unsigned int carry = 0u;
  for (unsigned int base = 0; base < ntiles; base += RT_THREADS) {
    const unsigned int t = base + threadIdx.x;       // (base + 255 < 2^32: ntiles <= 2^20)
    const unsigned int v = t < ntiles ? row[t] : 0u;
    unsigned int total;
    const unsigned int excl = block_excl_sum(v, s_w, &total);
    if (t < ntiles) row[t] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) hdr[H_TOT + blockIdx.x] = carry;
}

__global__ __launch_bounds__(RT_THREADS) void rank_scatter_kernel(const unsigned int* __restrict__ hdr,
                                                                  unsigned long long* keyA, unsigned long long* keyB,
                                                                  unsigned int* idxA, unsigned int* idxB, unsigned int M,
                                                                  unsigned int ntiles, int pass,
                                                                  const unsigned int* __restrict__ table) {
  __shared__ unsigned int s_cnt[RT_WAVES][256];      // per wavefront and digit: its count, then the next place it writes
  __shared__ unsigned int s_w[RT_WAVES];
  if (hdr[H_SKIP + pass]) return;
  const unsigned int from = hdr[H_SRC + pass];
  const unsigned long long* __restrict__ kin = from ? keyB : keyA;
  unsigned long long* __restrict__ kout = from ? keyA : keyB;
  const unsigned int* __restrict__ iin = from ? idxB : idxA;
  unsigned int* __restrict__ iout = from ? idxA : idxB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int w = 0; w < RT_WAVES; w++) s_cnt[w][tid] = 0u;
  unsigned int total;
  const unsigned int dbase = block_excl_sum(hdr[H_TOT + tid], s_w, &total);   // keys with a smaller digit (its barriers order s_cnt)
  unsigned long long kx[RT_PER];
  unsigned int ix[RT_PER];
  const unsigned long long first = (unsigned long long)blockIdx.x * RT + (unsigned long long)wave * RT_WAVE + lane;
#pragma unroll
  for (int u = 0; u < RT_PER; u++) {
    const unsigned long long e = first + 64ull * u;
    kx[u] = 0ull; ix[u] = 0u;
    if (e < M) {
      kx[u] = kin[e]; ix[u] = iin[e];
      atomicAdd(&s_cnt[wave][(unsigned int)(kx[u] >> (8 * pass)) & 255u], 1u);
    }
  }
  __syncthreads();
  {
    unsigned int run = dbase + table[(unsigned long long)tid * ntiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < RT_WAVES; w++) {
      const unsigned int c = s_cnt[w][tid];
      s_cnt[w][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < RT_PER; u++) {
    const bool valid = first + 64ull * u < M;
    const unsigned int d = (unsigned int)(kx[u] >> (8 * pass)) & 255u;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long has = __ballot(bit);
      same &= bit ? has : ~has;
    }
    const bool in = valid && same != 0ull;           // (a valid lane is in its own set)
    const int leader = in ? __ffsll((long long)same) - 1 : lane;
    unsigned int place = 0u;
    if (in && lane == leader) place = atomicAdd(&s_cnt[wave][d], (unsigned int)__popcll(same));
    place = __shfl(place, leader, 64) + (unsigned int)__popcll(same & ((1ull << lane) - 1ull));
    if (in && place < M) { kout[place] = kx[u]; iout[place] = ix[u]; }
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ void rank_median_kernel(unsigned int* hdr, const unsigned long long* keyA, const unsigned long long* keyB,
                                   unsigned int M, double* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long* key = hdr[H_FINAL] ? keyB : keyA;
  const double med = (value_of(key[M / 2 - 1]) + value_of(key[M / 2])) / 2.0;
  *reinterpret_cast<double*>(hdr + H_MED) = med;
  info[0] = (double)hdr[H_NF];
  info[1] = med;
}

// -------------------------------------------------------------------------------------------------------------------- rank
__global__ __launch_bounds__(RT_THREADS) void rank_heads_kernel(const unsigned int* __restrict__ hdr,
                                                                const unsigned long long* keyA,
                                                                const unsigned long long* keyB, unsigned int M,
                                                                unsigned int* __restrict__ last_head,
                                                                unsigned int* __restrict__ first_head) {
  __shared__ unsigned int s_last, s_first;
  const unsigned long long* __restrict__ key = hdr[H_FINAL] ? keyB : keyA;
  if (threadIdx.x == 0) { s_last = 0u; s_first = M; }
  __syncthreads();
  unsigned int last = 0u, first = M;
#pragma unroll 4
  for (int u = 0; u < RT_PER; u++) {
    const unsigned long long e = (unsigned long long)blockIdx.x * RT + (unsigned long long)u * RT_THREADS + threadIdx.x;
    if (e < M && (e == 0 || key[e] != key[e - 1])) {
      last = last > (unsigned int)e + 1u ? last : (unsigned int)e + 1u;
      first = first < (unsigned int)e ? first : (unsigned int)e;
    }
  }
  if (last) { atomicMax(&s_last, last); atomicMin(&s_first, first); }
  __syncthreads();
  if (threadIdx.x == 0) { last_head[blockIdx.x] = s_last; first_head[blockIdx.x] = s_first; }
}

// One workgroup: carry_start[t] = max of last_head over the tiles before t, carry_end[t] = min of first_head over the tiles
// after t, in chunks of RT_THREADS tiles with a carry.
__global__ __launch_bounds__(RT_THREADS) void rank_carry_kernel(unsigned int M, unsigned int ntiles,
                                                                const unsigned int* __restrict__ last_head,
                                                                const unsigned int* __restrict__ first_head,
                                                                unsigned int* __restrict__ carry_start,
                                                                unsigned int* __restrict__ carry_end) {
  __shared__ unsigned int s_v[RT_THREADS];
  const int tid = threadIdx.x;
  unsigned int carry = 0u;
  for (unsigned int base = 0; base < ntiles; base += RT_THREADS) {
    const unsigned int t = base + tid;
    s_v[tid] = t < ntiles ? last_head[t] : 0u;
    __syncthreads();
    unsigned int best = carry;                       // heads ascend with the tiles: the nearest tile before t that has one
    for (int u = tid - 1; u >= 0; u--)
      if (s_v[u]) { best = s_v[u]; break; }
    if (t < ntiles) carry_start[t] = best;
    unsigned int next = carry;
    for (int u = RT_THREADS - 1; u >= 0; u--)
      if (s_v[u]) { next = s_v[u]; break; }
    carry = next;
    __syncthreads();
  }
  carry = M;
  const unsigned int chunks = (ntiles + RT_THREADS - 1) / RT_THREADS;
  for (unsigned int c = chunks; c-- > 0;) {
    const unsigned int t = c * RT_THREADS + tid;
    s_v[tid] = t < ntiles ? first_head[t] : M;
    __syncthreads();
    unsigned int best = carry;
    for (int u = tid + 1; u < RT_THREADS; u++)
      if (s_v[u] != M) { best = s_v[u]; break; }
    if (t < ntiles) carry_end[t] = best;
    unsigned int next = carry;
    for (int u = 0; u < RT_THREADS; u++)
      if (s_v[u] != M) { next = s_v[u]; break; }
    carry = next;
    __syncthreads();
  }
}

// what = 0: z, what = 1: 2 r, to dest[e] of the element e the sorted pair came from.
__global__ __launch_bounds__(RT_THREADS) void rank_score_kernel(const unsigned int* __restrict__ hdr,
                                                                const unsigned long long* keyA,
                                                                const unsigned long long* keyB, const unsigned int* idxA,
                                                                const unsigned int* idxB, unsigned int M,
                                                                const unsigned int* __restrict__ carry_start,
                                                                const unsigned int* __restrict__ carry_end, int what,
                                                                double* __restrict__ dest) {
  __shared__ unsigned int s_a[RT_THREADS];
  const unsigned int fin = hdr[H_FINAL];
  const unsigned long long* __restrict__ key = fin ? keyB : keyA;
  const unsigned int* __restrict__ idx = fin ? idxB : idxA;
  const int tid = threadIdx.x;
  const unsigned long long b0 = (unsigned long long)blockIdx.x * RT + (unsigned long long)tid * RT_PER;
  bool head[RT_PER];
  unsigned int start[RT_PER], end[RT_PER];
  unsigned long long prev = b0 > 0 && b0 - 1 < M ? key[b0 - 1] : 0ull;
#pragma unroll
  for (int u = 0; u < RT_PER; u++) {
    const unsigned long long e = b0 + u;
    const unsigned long long kx = e < M ? key[e] : 0ull;
    head[u] = e < M && (e == 0 || kx != prev);
    prev = kx;
  }
  // the last head at or before every element: within the thread, then from the threads before it, then from the tiles before
  unsigned int st = 0u;
#pragma unroll
  for (int u = 0; u < RT_PER; u++) {
    if (head[u]) st = (unsigned int)(b0 + u) + 1u;
    start[u] = st;
  }
  s_a[tid] = st;
  __syncthreads();
  unsigned int before = carry_start[blockIdx.x];
  for (int u = tid - 1; u >= 0; u--)
    if (s_a[u]) { before = s_a[u]; break; }
  __syncthreads();
  // the first head after every element
  unsigned int en = M;
#pragma unroll
  for (int u = RT_PER - 1; u >= 0; u--) {
    end[u] = en;
    if (head[u]) en = (unsigned int)(b0 + u);
  }
  s_a[tid] = en;
  __syncthreads();
  unsigned int after = carry_end[blockIdx.x];
  for (int u = tid + 1; u < RT_THREADS; u++)
    if (s_a[u] != M) { after = s_a[u]; break; }
  const double denom = (double)M + 0.25;
#pragma unroll
  for (int u = 0; u < RT_PER; u++) {
    const unsigned long long e = b0 + u;
    if (e < M) {
      const unsigned int s1 = start[u] ? start[u] : before;        // 1 + the start of the run (position 0 is a head: never 0)
      const unsigned int e1 = end[u] != M ? end[u] : after;
      const double twice = (double)((unsigned long long)(s1 - 1u) + (unsigned long long)e1 + 1ull);   // 2 #less + #equal + 1
      const unsigned int at = idx[e];
      if (at < M) dest[at] = what ? twice : fmh_qnorm((0.5 * twice - 0.375) / denom);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ reduce
// Mean and unbiased variance of the n = N' scores of split chain blockIdx.x, two passes over them, each sum in this order:
// thread t adds its values in the order walk_pairs<RT_THREADS, RS_LU> hands them out (the pairs t, t + 256, ... of every batch of
// 2048 rows, x[i] before x[i + 1]) to a sum that starts at 0; the 64 sums of a wavefront are joined by the xor butterfly at lane
// distances 32, 16, 8, 4, 2, 1; the 4 wavefront sums are added in the order 0, 1, 2, 3.  mean = sum / n; the second pass sums
// (z - mean)^2 (a rounded difference, a rounded product) in the same order, variance = sum / (n - 1).  No value passes through
// more than 8 ceil(n / 2048) + 6 + 4 additions.
__device__ __forceinline__ double split_sum(double v, double* s_w) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = 0.0;
#pragma unroll
  for (int w = 0; w < RT_WAVES; w++) total += s_w[w];
  return total;
}

__global__ __launch_bounds__(RT_THREADS) void split_stats_kernel(const double* __restrict__ z, long long n,
                                                                 double* __restrict__ out) {
  __shared__ double s_w[RT_WAVES];
  const double* __restrict__ x = z + (long long)blockIdx.x * n;
  double acc = 0.0;
  walk_pairs<RT_THREADS, RS_LU>(x, n, [&](long long, double a, double b, bool has_b) { acc += a; if (has_b) acc += b; });
  const double mean = split_sum(acc, s_w) / (double)n;
  acc = 0.0;
  walk_pairs<RT_THREADS, RS_LU>(x, n, [&](long long, double a, double b, bool has_b) {
    const double da = a - mean;
    acc += da * da;
    if (has_b) { const double db = b - mean; acc += db * db; }
  });
  const double var = split_sum(acc, s_w) / (double)(n - 1);
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = mean; out[2 * blockIdx.x + 1] = var; }
}

// ---------------------------------------------------------------------------------------------------------------- the host
inline int rank_check(const char* who, const void* samples, const void* cols, const void* work, const void* out,
                      int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N, int32_t p) {
  if (!samples || !cols || !work || !out) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (nchains < 1) return fail(FMCMC_ERR_ARG, "%s: nchains = %lld, need at least one chain", who, (long long)nchains);
  if (k < 1) return fail(FMCMC_ERR_ARG, "%s: k = %d, need at least one parameter", who, (int)k);
  if (p < 1) return fail(FMCMC_ERR_ARG, "%s: p = %d, need at least one column", who, (int)p);
  if (p > k) return fail(FMCMC_ERR_ARG, "%s: p = %d columns, one of them is outside the k = %d parameters", who, (int)p, (int)k);
  if (N < 4) return fail(FMCMC_ERR_ARG, "%s: a window of N = %lld rows is too short: shorter than 4 rows", who, (long long)N);
  if (row0 < 0 || N > S || row0 > S - N)
    return fail(FMCMC_ERR_ARG, "%s: the window [%lld, %lld) is outside the %lld rows of a chain", who, (long long)row0,
                (long long)(row0 + N), (long long)S);
  if (nchains > 0x7fffffffLL || N / 2 > 0xffffffffLL / (2 * nchains))
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: 2 x %lld split chains of %lld rows are 2^32 values or more; the index of a value "
                "is a 32-bit word", who, (long long)nchains, (long long)(N / 2));
  return FMCMC_OK;
}

inline int rank_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

// Gathers column j (folded around the med in the head when `fold`) and sorts its pairs; the head says where they end up.
inline int rank_sort_column(const char* who, const double* samples, int k, long long S, long long row0, long long N,
                            const int32_t* cols, int j, int fold, unsigned int M, const RankBufs& b, hipStream_t st) {
  const unsigned int nt = (unsigned int)rank_tiles(M);
  // the bulk gather starts from a cleared head; the fold keeps the non-finite count and med of the bulk
  if (hipMemsetAsync(b.hdr, 0, fold ? (size_t)H_TOT * 4 : (size_t)H_WORDS64 * 8, st) != hipSuccess)
    return fail(FMCMC_ERR_DEVICE, "%s: clearing the digit counts failed", who);
  hipLaunchKernelGGL(rank_gather_kernel, dim3(nt), dim3(RT_THREADS), 0, st, samples, S, k, row0, N, cols, j, fold, M, b.hdr,
                     b.key[0], b.idx[0]);
  hipLaunchKernelGGL(rank_plan_kernel, dim3(1), dim3(RT_THREADS), 0, st, b.hdr, M);
  for (int pass = 0; pass < 8; pass++) {
    hipLaunchKernelGGL(rank_tile_hist_kernel, dim3(nt), dim3(RT_THREADS), 0, st, b.hdr, b.key[0], b.key[1], M, nt, pass, b.table);
    hipLaunchKernelGGL(rank_scan_rows_kernel, dim3(256), dim3(RT_THREADS), 0, st, b.hdr, nt, pass, b.table);
    hipLaunchKernelGGL(rank_scatter_kernel, dim3(nt), dim3(RT_THREADS), 0, st, b.hdr, b.key[0], b.key[1], b.idx[0], b.idx[1], M,
                       nt, pass, b.table);
  }
  return rank_launched(who);
}

inline int rank_score_column(const char* who, unsigned int M, const RankBufs& b, int what, double* dest, hipStream_t st) {
  const unsigned int nt = (unsigned int)rank_tiles(M);
  hipLaunchKernelGGL(rank_heads_kernel, dim3(nt), dim3(RT_THREADS), 0, st, b.hdr, b.key[0], b.key[1], M, b.last_head,
                     b.first_head);
  hipLaunchKernelGGL(rank_carry_kernel, dim3(1), dim3(RT_THREADS), 0, st, M, nt, b.last_head, b.first_head, b.carry_start,
                     b.carry_end);
  hipLaunchKernelGGL(rank_score_kernel, dim3(nt), dim3(RT_THREADS), 0, st, b.hdr, b.key[0], b.key[1], b.idx[0], b.idx[1], M,
                     b.carry_start, b.carry_end, what, dest);
  return rank_launched(who);
}

inline int rank_median(const char* who, unsigned int M, const RankBufs& b, double* info, hipStream_t st) {
  hipLaunchKernelGGL(rank_median_kernel, dim3(1), dim3(64), 0, st, b.hdr, b.key[0], b.key[1], M, info);
  return rank_launched(who);
}

}  // namespace

extern "C" {

int64_t fmcmc_rank_work_len(int64_t nchains, int32_t p, int64_t N) {
  if (nchains < 1 || p < 1 || N < 4 || nchains > 0x7fffffffLL || N / 2 > 0xffffffffLL / (2 * nchains)) return 0;
  return rank_work_words(2 * nchains * (N / 2));
}

int64_t fmcmc_rank_rhat_out_len(int64_t nchains, int32_t p) {
  if (nchains < 1 || p < 1 || nchains > 0x7fffffffLL) return 0;
  return (int64_t)p * (8 * nchains + 2);
}

int fmcmc_rank_scores_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                          const int32_t* cols, int32_t p, int32_t fold, int32_t what, double* work, double* out, double* info,
                          void* hip_stream) {
  const char* who = "fmcmc_rank_scores_dev";
  int rc = rank_check(who, samples, cols, work, out, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (!info) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if ((fold != 0 && fold != 1) || (what != 0 && what != 1))
    return fail(FMCMC_ERR_ARG, "%s: fold = %d and what = %d must each be 0 or 1", who, (int)fold, (int)what);
  hipStream_t st = (hipStream_t)hip_stream;
  const long long Mll = 2 * nchains * (N / 2);
  const unsigned int M = (unsigned int)Mll;
  const RankBufs b = rank_bufs(work, Mll);
  for (int j = 0; j < p; j++) {
    if ((rc = rank_sort_column(who, samples, k, S, row0, N, cols, j, 0, M, b, st)) != FMCMC_OK) return rc;
    if ((rc = rank_median(who, M, b, info + 2 * j, st)) != FMCMC_OK) return rc;
    if (fold && (rc = rank_sort_column(who, samples, k, S, row0, N, cols, j, 1, M, b, st)) != FMCMC_OK) return rc;
    if ((rc = rank_score_column(who, M, b, what, out + (long long)j * Mll, st)) != FMCMC_OK) return rc;
  }
  return FMCMC_OK;
}

int fmcmc_rank_rhat_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                        const int32_t* cols, int32_t p, double* work, double* out, void* hip_stream) {
  const char* who = "fmcmc_rank_rhat_dev";
  int rc = rank_check(who, samples, cols, work, out, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  const long long Mll = 2 * nchains * (N / 2), m = 2 * nchains;
  const unsigned int M = (unsigned int)Mll;
  const RankBufs b = rank_bufs(work, Mll);
  for (int j = 0; j < p; j++) {
    double* o = out + (long long)j * (4 * m + 2);
    for (int fold = 0; fold < 2; fold++) {
      if ((rc = rank_sort_column(who, samples, k, S, row0, N, cols, j, fold, M, b, st)) != FMCMC_OK) return rc;
      if (!fold && (rc = rank_median(who, M, b, o + 4 * m, st)) != FMCMC_OK) return rc;
      if ((rc = rank_score_column(who, M, b, 0, b.z, st)) != FMCMC_OK) return rc;
      hipLaunchKernelGGL(split_stats_kernel, dim3((unsigned)m), dim3(RT_THREADS), 0, st, b.z, (long long)(N / 2),
                         o + 2 * m * fold);
      if ((rc = rank_launched(who)) != FMCMC_OK) return rc;
    }
  }
  return FMCMC_OK;
}

}  // extern "C"
