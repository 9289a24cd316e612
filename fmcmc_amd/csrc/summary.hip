// summary.hip — posterior summary of a call's kept rows, computed where the sweep left them (coda::summary.mcmc(.list),
// coda::effectiveSize, coda::spectrum0.ar; formulas restated in fmcmc_amd/convergence.py and INTEGRATION.md).
//
// One chain's column is N contiguous doubles (samples + (c k + col) S + row0), so every stage walks contiguous memory:
//   1. summary_series_kernel   one workgroup per (chain, column): mean, autocovariances r_0..r_M of the series centred on its
//                              own mean, residual sd of the straight-line fit, count of non-finite values;
//   2. summary_ar_kernel       one wavefront per series: Levinson-Durbin + AIC order + spectral density at zero;
//   3. summary_pool_kernel     fixed-order sums over the chains: pooled mean / variance, mean spec0, effective size;
//   4. select_*                exact order statistics of the pooled C N values of a column by a most-significant-digit radix
//                              select on order-preserving 64-bit keys (8 passes of 8 bits, integer counts only);
//   5. summary_cvm_kernel      coda::heidel.diag: stages 1-2 on the S0 window and on every candidate tail, then one workgroup
//                              per (series, candidate) scans the centred tail and sums the squares of its Brownian bridge.
//   6. summary_lag_kernel      coda::autocorr: autocovariances at up to 32 freely chosen row lags (stage 1 stops at lag M), one
//                              workgroup per series: the mean as in stage 1, then one walk per eight lags that reads x_{t+h} from global memory.
//   7. groups                  fmcmc_summary_groups_dev: the summary of every group of consecutive chains on its own (one model on
//                              many datasets).  Stages 1-2 once over all chains (summary_*_masked_kernel under a group mask: the
//                              same device bodies), summary_group_pool_kernel = stage 3's body per (group, column), and
//                              summary_group_select_kernel: the pooled order statistics of a (group, column) by ONE workgroup
//                              (the one-workgroup radix select of diag_common.hpp over the group's chains).
// Every sum has a fixed shape, so the results do not depend on the launch.  Nothing here writes `samples`.
#include "diag_common.hpp"

namespace {

constexpr int ACS = 72;             // doubles per series in work: r[0..64], 65 mean, 66 residual sd of x ~ 1 + t, 67 non-finite count
constexpr int SLOT_MEAN = 65, SLOT_RSD = 66, SLOT_NF = 67;
constexpr int ST = 512;             // threads of the series kernel
constexpr int SW = ST / 64;
constexpr int RED = 68;             // reduction scratch per wave ((LDS_ROWS + 72) rows of a tile + SW of these < 160 KB)
constexpr int LG = 8;               // lags per group of the product loop
constexpr int PAD = MAXM + LG;      // zero rows behind a tile
constexpr int MAXPROBS = 16;
constexpr int HT = 256;             // threads of the histogram kernel
constexpr int HP = 4;               // 16-byte loads in flight per thread of the histogram kernel
constexpr int TILE = 2 * HP * HT;   // rows of one chain a histogram block takes per step

__device__ __forceinline__ double wave_sum(double v) {   // butterfly: the same value, formed in the same order, in every lane
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum over the workgroup: lanes by butterfly, then the waves in wave order.  `red` holds one double per wave.
template <int NWAVES>
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NWAVES; w++) s += red[w];
  return s;
}

// ---------------------------------------------------------------------------------------------------------------- stage 1
// The series is staged in LDS once when it fits (N <= tile_rows): the mean, the centring, all M + 1 lags and the line fit are
// taken from there.  A longer series takes the mean from global memory and then walks tiles of tile_rows rows with an M-row
// halo.  Thread t owns the rows t, t + ST, ... of a tile (conflict-free 8-byte LDS reads for every lag) and keeps one
// accumulator per lag; the accumulators are joined over the lanes in a fixed pattern and then in wave order.
__device__ __forceinline__ void series_body(const double* __restrict__ samples, long long S, int k, long long row0, long long N,
                                            const int* __restrict__ cols, int p, int M, int tile_rows,
                                            double* __restrict__ acov) {
  extern __shared__ double smem[];
  double* s_x = smem;                          // [tile_rows + PAD]
  double* s_red = smem + tile_rows + PAD;      // [SW * RED]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long series = blockIdx.x, c = series / p;
  const int j = (int)(series % p);
  const double* __restrict__ x = samples + (c * (long long)k + cols[j]) * S + row0;
  double* out = acov + series * ACS;
  const bool single = N <= (long long)tile_rows;
  const double dn = (double)N;

  // mean (and the count of non-finite values); a short series is staged on the way
  double s = 0.0, nf = 0.0;
  // (written out, not walk_pairs of diag_common.hpp: through the template the same operations compile to another block layout
  //  of this loop, which measured 0.05 ms = 1 % more at 512 x 50 x 5000)
  constexpr int LU = 8;                        // pairs in flight per thread: the loads of a batch are issued back to back
  for (long long base = 0; base < N; base += 2LL * LU * ST) {
    double a[LU], b[LU];
#pragma unroll
    for (int u = 0; u < LU; u++) {
      const long long i = base + 2LL * (u * ST + tid);
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
      const long long i = base + 2LL * (u * ST + tid);
      if (i < N) {                             // (a missing second row of the pair adds 0)
        s += a[u]; s += b[u];
        nf += (fmh_isfinite(a[u]) ? 0.0 : 1.0) + (fmh_isfinite(b[u]) ? 0.0 : 1.0);
        if (single) { s_x[i] = a[u]; if (i + 1 < N) s_x[i + 1] = b[u]; }
      }
    }
  }
  const double mean = block_sum<SW>(s, s_red) / dn;
  nf = block_sum<SW>(nf, s_red);

  double acc[MAXM + 1];
#pragma unroll
  for (int l = 0; l <= MAXM; l++) acc[l] = 0.0;
  double sxt = 0.0;
  const double tbar = 0.5 * (dn - 1.0);        // rows are numbered 0 .. N - 1 (the fit's residuals do not depend on the origin)
  for (long long t0 = 0; t0 < N; t0 += tile_rows) {
    const int len = (int)((N - t0 < tile_rows) ? N - t0 : tile_rows);
    const int ext = (int)((N - t0 < (long long)tile_rows + M) ? N - t0 : (long long)tile_rows + M);
    __syncthreads();
    if (single) {
      for (int i = tid; i < len; i += ST) s_x[i] -= mean;
    } else {
      for (int i = tid; i < ext; i += ST) s_x[i] = x[t0 + i] - mean;
    }
    for (int i = ext + tid; i < len + PAD; i += ST) s_x[i] = 0.0;    // rows beyond the series multiply as 0
    __syncthreads();
    for (int i = tid; i < len; i += ST) {
      const double xi = s_x[i];
      sxt = __builtin_fma((double)(t0 + i) - tbar, xi, sxt);
      // lags in groups of LG: one uniform branch per group, its LDS reads issued together (a branch per lag left every read's
      // latency exposed: 1.0 ms instead of 0.6 at 1024 x 5 x 10^4); the lags of the last group beyond M are computed and dropped
#pragma unroll
      for (int g = 0; g < MAXM / LG; g++) {
        if (LG * g <= M) {
#pragma unroll
          for (int u = 0; u < LG; u++) acc[LG * g + u] = __builtin_fma(xi, s_x[i + LG * g + u], acc[LG * g + u]);
        }
      }
      if (M == MAXM) acc[MAXM] = __builtin_fma(xi, s_x[i + MAXM], acc[MAXM]);
    }
  }
  // join.  Lanes: a transposing reduction of the lags 0..63 -- at the step of distance h a lane keeps the half of its values
  // whose index has bit h equal to its own lane bit and adds the partner's copy of that half; after the six steps lane l holds
  // the wave's sum of lag l (63 exchanges instead of 64 butterflies of six).  Lag 64 and the line-fit sum by butterfly.
  __syncthreads();
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
    const bool up = (lane & h) != 0;
#pragma unroll
    for (int i = 0; i < h; i++) {
      const double keep = up ? acc[i + h] : acc[i];
      const double send = up ? acc[i] : acc[i + h];
      acc[i] = keep + __shfl_xor(send, h, 64);
    }
  }
  s_red[wave * RED + lane] = acc[0];
  {
    const double v64 = wave_sum(acc[MAXM]), vt = wave_sum(sxt);
    if (lane == 0) { s_red[wave * RED + MAXM] = v64; s_red[wave * RED + MAXM + 1] = vt; }
  }
  __syncthreads();
  if (tid <= MAXM + 1) {
    double v = s_red[tid];
    for (int w = 1; w < SW; w++) v += s_red[w * RED + tid];
    s_red[tid] = v;
    if (tid <= M) out[tid] = v / dn;           // acf(type = "covariance"): divisor N
    else if (tid <= MAXM) out[tid] = 0.0;
  }
  __syncthreads();
  // residual standard deviation of x ~ 1 + t, from the residuals themselves (the closed form N r_0 - sxt^2 / stt cancels to
  // noise of the size of the threshold for an exactly linear series)
  const double stt = dn * (dn * dn - 1.0) / 12.0;
  const double slope = s_red[MAXM + 1] / stt;
  double rs = 0.0, rss = 0.0;
  for (long long i = tid; i < N; i += ST) {
    const double xc = single ? s_x[i] : x[i] - mean;
    const double res = xc - slope * ((double)i - tbar);
    rs += res;
    rss = __builtin_fma(res, res, rss);
  }
  rs = block_sum<SW>(rs, s_red + SW * RED - SW);     // (the last SW doubles of the scratch: s_red[MAXM + 1] is still being read)
  rss = block_sum<SW>(rss, s_red + SW * RED - SW);
  if (tid == 0) {
    const double q = rss - rs * rs / dn;
    out[SLOT_MEAN] = mean;
    out[SLOT_RSD] = sqrt((q > 0.0 ? q : (q == q ? 0.0 : q)) / (dn - 1.0));
    out[SLOT_NF] = nf;
  }
}

__global__ __launch_bounds__(ST) void summary_series_kernel(const double* __restrict__ samples, long long S, int k, long long row0,
                                                            long long N, const int* __restrict__ cols, int p, int M,
                                                            int tile_rows, double* __restrict__ acov) {
  series_body(samples, S, k, row0, N, cols, p, M, tile_rows, acov);
}

// The same series under the mask of fmcmc_summary_groups_dev: the chains are groups of `cpg` consecutive chains, and the series
// of a group whose `active` entry is 0 return before they touch anything (the test is uniform per workgroup).
__global__ __launch_bounds__(ST) void summary_series_masked_kernel(const double* __restrict__ samples, long long S, int k,
                                                                   long long row0, long long N, const int* __restrict__ cols, int p,
                                                                   int M, int tile_rows, long long cpg,
                                                                   const int* __restrict__ active, double* __restrict__ acov) {
  if (active[((long long)blockIdx.x / p) / cpg] == 0) return;
  series_body(samples, S, k, row0, N, cols, p, M, tile_rows, acov);
}

// ---------------------------------------------------------------------------------------------------------------- stage 2
// stats::ar.yw (Levinson-Durbin, AIC, first minimum) and coda::spectrum0.ar for one series per wavefront.  Lane j holds the
// coefficient of lag j + 1 and r_{j+1}; step m needs coefficient m - i next to coefficient i and r_{m-i} next to it: both are
// the same lane reversal over the first m - 1 lanes.
template <bool MASKED>
__device__ __forceinline__ void ar_body(const double* __restrict__ acov, long long nseries, long long N, int M, int p, long long cpg,
                                        const int* __restrict__ active, double* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = w < nseries;
  if (!live) w = nseries - 1;
  if (MASKED && active[(w / p) / cpg] == 0) return;    // (uniform per wavefront, and nothing below crosses wavefronts)
  const double* a = acov + w * ACS;
  const double dn = (double)N;
  const double r0 = a[0];
  const double rj = (lane < M) ? a[lane + 1] : 0.0;
  const double mean = a[SLOT_MEAN], rsd = a[SLOT_RSD];
  double coef = 0.0, v = r0;
  double best_aic = (dn * fmh_log(r0) + 0.0) + 2.0, best_v = r0, best_coef = 0.0;
  int best_o = 0;
  for (int m = 1; m <= M; m++) {
    const bool below = lane < m - 1;
    const int src = below ? m - 2 - lane : lane;
    const double rrev = __shfl(rj, src, 64), crev = __shfl(coef, src, 64);
    const double acc = __shfl(rj, m - 1, 64) - wave_sum(below ? coef * rrev : 0.0);
    const double phi = acc / v;
    coef = below ? coef - phi * crev : (lane == m - 1 ? phi : coef);
    v = v * (1.0 - phi * phi);
    const double aic = (dn * fmh_log(v) + 2.0 * m) + 2.0;
    if (aic < best_aic) { best_aic = aic; best_v = v; best_coef = coef; best_o = m; }
  }
  const double sum_ar = wave_sum(best_coef);
  const double var_pred = best_v * dn / (dn - (double)(best_o + 1));
  const double one_m = 1.0 - sum_ar;
  double spec0 = var_pred / (one_m * one_m);
  double order = (double)best_o;
  if (rsd < 1.5e-8) { spec0 = 0.0; order = 0.0; }       // constant or exactly linear series (coda: all.equal(sd(residuals), 0))
  if (live && lane == 0) {
    double* o = stats + w * 4;
    o[0] = mean;
    o[1] = r0 * dn / (dn - 1.0);
    o[2] = spec0;
    o[3] = order;
  }
}

__global__ __launch_bounds__(256) void summary_ar_kernel(const double* __restrict__ acov, long long nseries, long long N, int M,
                                                         double* __restrict__ stats) {
  ar_body<false>(acov, nseries, N, M, 1, 1, nullptr, stats);
}

__global__ __launch_bounds__(256) void summary_ar_masked_kernel(const double* __restrict__ acov, long long nseries, long long N,
                                                                int M, int p, long long cpg, const int* __restrict__ active,
                                                                double* __restrict__ stats) {
  ar_body<true>(acov, nseries, N, M, p, cpg, active, stats);
}

// ---------------------------------------------------------------------------------------------------------------- stage 3
// Per column: pooled mean and centred sum of squares from the chains' {N, mean, M2} (all chains have N rows), sum of spec0,
// sum of the effective-size terms, non-finite count.  Thread g takes the chains g, g + 256, ... in chain order.
__device__ __forceinline__ void pool_body(const double* __restrict__ stats, const double* __restrict__ acov, long long C, int p,
                                          long long N, int j, double* __restrict__ pooled) {
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const double dn = (double)N, dc = (double)C;
  double s = 0.0;
  for (long long c = tid; c < C; c += 256) s += stats[(c * p + j) * 4];
  const double mean = block_sum<4>(s, s_red) / dc;
  double m2 = 0.0, ssp = 0.0, sess = 0.0, snf = 0.0;
  for (long long c = tid; c < C; c += 256) {
    const double* o = stats + (c * p + j) * 4;
    const double d = o[0] - mean;
    m2 += (dn - 1.0) * o[1] + dn * d * d;
    ssp += o[2];
    sess += (o[2] == 0.0) ? 0.0 : dn * o[1] / o[2];
    snf += acov[(c * p + j) * ACS + SLOT_NF];
  }
  m2 = block_sum<4>(m2, s_red);
  ssp = block_sum<4>(ssp, s_red);
  sess = block_sum<4>(sess, s_red);
  snf = block_sum<4>(snf, s_red);
  if (tid == 0) {
    double* o = pooled + (long long)j * 5;
    o[0] = mean;
    o[1] = m2 / (dc * dn - 1.0);
    o[2] = ssp / dc;
    o[3] = sess;
    o[4] = snf;
  }
}

__global__ __launch_bounds__(256) void summary_pool_kernel(const double* __restrict__ stats, const double* __restrict__ acov,
                                                           long long C, int p, long long N, double* __restrict__ pooled) {
  pool_body(stats, acov, C, p, N, blockIdx.x, pooled);
}

// The pool of every group of `cpg` consecutive chains on its own (fmcmc_summary_groups_dev): workgroup g p + j pools column j over
// the chains of group g into row g of `pooled` (rows of `plen` doubles), with C = cpg in every divisor -- pool_body on the
// group's slice of `stats` and `acov`, so the same sums in the same order as summary_pool_kernel on those chains alone.
__global__ __launch_bounds__(256) void summary_group_pool_kernel(const double* __restrict__ stats, const double* __restrict__ acov,
                                                                 long long cpg, int p, long long N, const int* __restrict__ active,
                                                                 long long plen, double* __restrict__ pooled) {
  const long long g = blockIdx.x / p;
  if (active && active[g] == 0) return;
  pool_body(stats + g * cpg * p * 4, acov + g * cpg * p * ACS, cpg, p, N, (int)(blockIdx.x % p), pooled + g * plen);
}

// ---------------------------------------------------------------------------------------------------------------- stage 4
// Radix select.  A target is (column, prob, lo | hi) with a 0-based rank among the C N pooled values of its column.  Pass d
// fixes bits [56 - 8 d, 64 - 8 d) of its key: the histogram of that digit over the values whose higher bits equal the target's
// prefix, then a walk over the 256 counts.  Targets of a column with the same prefix share one histogram (that of the first
// of them, their "leader"): in the first passes that is one histogram for all of them.  Counts are integers, so neither the
// arrival order of the atomic adds nor ties matter.
struct Ranks { long long lo[MAXPROBS], hi[MAXPROBS]; };

// state per target: prefix, rank, leader (index within the column); then the histograms [T][256]
__global__ __launch_bounds__(256) void select_init_kernel(unsigned long long* __restrict__ state, unsigned long long* __restrict__ hist,
                                                          int nprobs, Ranks ranks) {
  const int t = blockIdx.x, nt = 2 * nprobs, tl = t % nt;
  hist[(long long)t * 256 + threadIdx.x] = 0ull;
  if (threadIdx.x == 0) {
    state[3LL * t] = 0ull;
    state[3LL * t + 1] = (unsigned long long)((tl & 1) ? ranks.hi[tl >> 1] : ranks.lo[tl >> 1]);
    state[3LL * t + 2] = 0ull;
  }
}

__global__ __launch_bounds__(HT) void select_hist_kernel(const double* __restrict__ samples, long long S, int k, long long row0,
                                                         long long N, long long C, const int* __restrict__ cols, int nprobs,
                                                         int pass, const unsigned long long* __restrict__ state,
                                                         unsigned long long* __restrict__ hist) {
  extern __shared__ unsigned int s_h[][256];           // [2 nprobs][256]
  __shared__ unsigned long long s_prefix[2 * MAXPROBS];
  __shared__ int s_lead[2 * MAXPROBS];
  __shared__ int s_nlead;
  const int j = blockIdx.y, nt = 2 * nprobs, tid = threadIdx.x;
  const unsigned long long* st = state + 3LL * j * nt;
  if (tid == 0) {
    int n = 0;
    for (int t = 0; t < nt; t++)
      if ((int)st[3 * t + 2] == t) { s_lead[n] = t; s_prefix[n] = st[3 * t]; n++; }
    s_nlead = n;
  }
  for (int e = tid; e < nt * 256; e += HT) (&s_h[0][0])[e] = 0u;
  __syncthreads();
  const int nlead = s_nlead;
  const long long tiles_per_chain = (N + TILE - 1) / TILE, total = C * tiles_per_chain;
  const double* __restrict__ colbase = samples + (long long)cols[j] * S + row0;
  for (long long tile = blockIdx.x; tile < total; tile += gridDim.x) {
    const long long c = tile / tiles_per_chain, r0 = (tile % tiles_per_chain) * TILE;
    const double* __restrict__ x = colbase + c * (long long)k * S;
    double v[2 * HP];
    bool ok[2 * HP];
#pragma unroll
    for (int u = 0; u < HP; u++) {
      const long long r = r0 + u * (2 * HT) + 2 * tid;
      ok[2 * u] = r < N; ok[2 * u + 1] = r + 1 < N;
      if (ok[2 * u + 1]) {
        const dpair_t q = *reinterpret_cast<const dpair_t*>(x + r);
        v[2 * u] = q[0]; v[2 * u + 1] = q[1];
      } else {
        v[2 * u] = ok[2 * u] ? x[r] : 0.0; v[2 * u + 1] = 0.0;
      }
    }
#pragma unroll
    for (int u = 0; u < 2 * HP; u++) {
      if (!ok[u]) continue;
      const unsigned long long kx = key_of(v[u]);
      const unsigned long long high = radix_high(kx, pass);
      const unsigned int digit = radix_digit(kx, pass);
      for (int g = 0; g < nlead; g++)
        if (high == s_prefix[g]) atomicAdd(&s_h[s_lead[g]][digit], 1u);
    }
  }
  __syncthreads();
  for (int g = 0; g < nlead; g++) {
    const int t = s_lead[g];
    for (int b = tid; b < 256; b += HT) {
      const unsigned int cnt = s_h[t][b];
      if (cnt) atomicAdd(&hist[((long long)j * nt + t) * 256 + b], (unsigned long long)cnt);
    }
  }
}

// One wavefront per column.  Per target the 64 lanes take four counts each of its leader's histogram, a prefix sum over the
// lanes finds the lane and then the bin that holds the rank; then lane = target: extend the prefix, find the new leaders,
// clear the histograms for the next pass.  After the last pass the prefix is the key of the order statistic.
__global__ __launch_bounds__(64) void select_scan_kernel(unsigned long long* __restrict__ state, unsigned long long* __restrict__ hist,
                                                         int nprobs, int pass, double* __restrict__ out) {
  __shared__ unsigned long long s_p[2 * MAXPROBS], s_cum[2 * MAXPROBS];
  __shared__ int s_digit[2 * MAXPROBS];
  const int j = blockIdx.x, nt = 2 * nprobs, t = threadIdx.x;
  unsigned long long* st = state + 3LL * j * nt;
  unsigned long long* hs = hist + (long long)j * nt * 256;
  if (t < nt) { s_digit[t] = 255; s_cum[t] = 0ull; }
  __syncthreads();
  for (int g = 0; g < nt; g++) {
    const unsigned long long rank = st[3 * g + 1];
    const unsigned long long* h = hs + (long long)st[3 * g + 2] * 256 + 4 * t;
    const unsigned long long c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
    const unsigned long long mine = c0 + c1 + c2 + c3;
    unsigned long long incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long up = __shfl_up(incl, o, 64);
      if (t >= o) incl += up;
    }
    unsigned long long cum = incl - mine;
    if (rank >= cum && rank < incl) {            // exactly one lane: the ranks are below the total count
      int b = 0;
      if (rank >= cum + c0) { cum += c0; b = 1;
        if (rank >= cum + c1) { cum += c1; b = 2;
          if (rank >= cum + c2) { cum += c2; b = 3; } } }
      s_digit[g] = 4 * t + b;
      s_cum[g] = cum;
    }
  }
  __syncthreads();
  unsigned long long prefix = 0ull;
  if (t < nt) {
    prefix = (st[3 * t] << 8) | (unsigned long long)s_digit[t];
    s_p[t] = prefix;
  }
  __syncthreads();
  for (int e = t; e < nt * 256; e += 64) hs[e] = 0ull;
  if (t < nt) {
    int lead = t;
    for (int u = t - 1; u >= 0; u--)
      if (s_p[u] == prefix) lead = u;
    st[3 * t] = prefix;
    st[3 * t + 1] -= s_cum[t];
    st[3 * t + 2] = (unsigned long long)lead;
    if (pass == 7) out[(long long)j * nt + t] = value_of(prefix);
  }
}

// Grouped select (fmcmc_summary_groups_dev): the order statistics of the cpg N pooled values of (group g, column j) by ONE
// workgroup, g p + j -- the one-workgroup radix select of diag_common.hpp over the cpg segments of N rows that are the group's
// chains (stride k S).  All eight passes, their histograms and scans stay in LDS: no global atomics, no launches per pass.  The
// targets are those of select_init_kernel, (prob q, lo | hi) at 2 q + (hi); every group has cpg N values, so the ranks are the
// same for all of them and travel as a kernel argument.  The keys are exact, so the values are those of the select above.
__global__ __launch_bounds__(SEL_T) void summary_group_select_kernel(const double* __restrict__ samples, long long S, int k,
                                                                     long long row0, long long N, long long cpg,
                                                                     const int* __restrict__ cols, int p, int nt, OrderRanks ranks,
                                                                     int staged, const int* __restrict__ active, long long plen,
                                                                     double* __restrict__ pooled) {
  extern __shared__ unsigned long long s_k[];        // [cpg N] when staged
  __shared__ SelectLds L;
  const int tid = threadIdx.x;
  const long long g = blockIdx.x / p;
  const int j = (int)(blockIdx.x % p);
  if (active && active[g] == 0) return;
  const double* __restrict__ x = samples + (g * cpg * (long long)k + cols[j]) * S + row0;
  const long long stride = (long long)k * S;
  stage_series(x, N, cpg, stride, staged != 0, s_k, L);
  if (tid < nt) { L.prefix[tid] = 0ull; L.rank[tid] = ranks.r[tid]; }
  select_series(x, N, cpg, stride, staged != 0, s_k, nt, L);
  if (tid < nt) pooled[g * plen + (long long)p * 5 + (long long)j * nt + tid] = value_of(L.prefix[tid]);
}

// ------------------------------------------------------------------------------------------------------- Heidelberger-Welch
// Cramer-von Mises sum of the Brownian bridge of a tail (coda::heidel.diag): Q = sum_t B_t^2, B_t = sum_{u <= t} (y_u - m), for
// the rows lo .. N - 1 of the window; m is the mean stages 1-2 left in `stats` for that tail (the same bits).  The series is
// centred before it is scanned (cumsum(Y) - ybar t cancels).  One workgroup per (series, candidate) walks the tail in tiles
// of CT rows, staged in LDS with coalesced loads; thread t then owns the CR consecutive rows t CR .. t CR + CR - 1 of the tile
// (CR odd: the 8-byte LDS reads of a 32-lane half fall on 32 different bank pairs).  Scan: the thread's own sum, a shuffle
// scan over the lanes, the waves' totals in wave order, and the carry of the tiles before; then the thread walks its rows
// again and accumulates B^2.  The shape of every sum depends on the length of the tail alone.
constexpr int CR = 9;               // rows per thread of a tile
constexpr int CT = ST * CR;         // rows per tile (36 KB of LDS: four workgroups per CU)
constexpr int CVM_CANDS = 32;       // candidates per launch (their first rows travel as kernel arguments)
struct CvmCands { long long lo[CVM_CANDS]; };

__global__ __launch_bounds__(ST) void summary_cvm_kernel(const double* __restrict__ samples, long long S, int k, long long row0,
                                                         long long N, const int* __restrict__ cols, int p, CvmCands cands,
                                                         const double* __restrict__ stats, long long nseries,
                                                         double* __restrict__ q_out) {
  __shared__ double s_x[CT];
  __shared__ double s_w[SW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long series = blockIdx.x, c = series / p;
  const int j = (int)(series % p), s = blockIdx.y;
  const long long lo = cands.lo[s], n = N - lo;
  const double* __restrict__ x = samples + (c * (long long)k + cols[j]) * S + row0 + lo;
  const double mean = stats[((long long)s * nseries + series) * 4];
  double carry = 0.0, q = 0.0;
  for (long long t0 = 0; t0 < n; t0 += CT) {
    const int len = (int)((n - t0 < CT) ? n - t0 : CT);
    double v[CR];
#pragma unroll
    for (int u = 0; u < CR; u++) {
      const int i = u * ST + tid;
      v[u] = (i < len) ? x[t0 + i] : mean;     // (rows beyond the tail: centred to exactly 0)
    }
    __syncthreads();                           // the tile before has been read
#pragma unroll
    for (int u = 0; u < CR; u++) s_x[u * ST + tid] = v[u] - mean;
    __syncthreads();
    double d[CR], loc = 0.0;
#pragma unroll
    for (int u = 0; u < CR; u++) { d[u] = s_x[tid * CR + u]; loc += d[u]; }
    double incl = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.0;
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    double before = carry, total = carry;      // the tiles before, then the waves in wave order
#pragma unroll
    for (int w = 0; w < SW; w++) {
      const double tw = s_w[w];
      total += tw;
      if (w < wave) before += tw;
    }
    carry = total;
    double B = before + excl;
    const int first = tid * CR;
#pragma unroll
    for (int u = 0; u < CR; u++) {
      B += d[u];
      if (first + u < len) q = __builtin_fma(B, B, q);
    }
  }
  __syncthreads();
  q = block_sum<SW>(q, s_w);
  if (tid == 0) q_out[(long long)s * nseries + series] = q;
}

// ------------------------------------------------------------------------------------------------------------ free lags
// c_h = (1 / N) sum_{t < N - h} (x_t - m)(x_{t+h} - m) at the row lags h of the call (stats::acf, type "covariance"), and c_0.
// The mean is the sum of stage 1 (the same order, so the same bits).  Thread t then owns the rows t, t + ST, ... and keeps one
// accumulator per lag: xc_t is formed once, x_{t+h} is read from global memory (L2 serves it: a thread's rows were loaded by
// its neighbours h rows ago) and centred again; a partner beyond the series multiplies as 0.  The lags travel as a kernel
// argument and are taken in groups of LG, one walk per group with the loads of a row issued together.  The sum of a lag is the
// thread's rows in ascending order, then block_sum: it depends on (N, h) alone, not on the other lags of the call.
constexpr int MAXLAGS = 32;
constexpr int LAG_HEAD = 3;         // doubles per series before the lags: mean, c_0, non-finite count
struct LagList { int h[MAXLAGS]; };  // each < N < 2^22; slots beyond nlags hold N (no partner row)

__global__ __launch_bounds__(ST) void summary_lag_kernel(const double* __restrict__ samples, long long S, int k, long long row0,
                                                         long long N, const int* __restrict__ cols, int p, int nlags,
                                                         LagList lags, double* __restrict__ nf_out, double* __restrict__ out) {
  __shared__ double s_red[SW];
  const int tid = threadIdx.x;
  const long long series = blockIdx.x, c = series / p;
  const int j = (int)(series % p);
  const double* __restrict__ x = samples + (c * (long long)k + cols[j]) * S + row0;
  const double dn = (double)N;
  double s = 0.0, nf = 0.0;
  walk_pairs<ST, 8>(x, N, [&](long long, double a, double b, bool) {      // (a missing second row of the pair adds 0)
    s += a; s += b;
    nf += (fmh_isfinite(a) ? 0.0 : 1.0) + (fmh_isfinite(b) ? 0.0 : 1.0);
  });
  const double mean = block_sum<SW>(s, s_red) / dn;
  nf = block_sum<SW>(nf, s_red);

  // one walk per group of LG lags (a call with the default five lags walks once); the first also sums c_0
  double* o = out + series * (LAG_HEAD + nlags);
#pragma unroll
  for (int g = 0; g < MAXLAGS / LG; g++) {
    if (LG * g < nlags) {
      double acc0 = 0.0, acc[LG];
#pragma unroll
      for (int u = 0; u < LG; u++) acc[u] = 0.0;
      for (long long i = tid; i < N; i += ST) {
        const double xi = x[i] - mean;
        double v[LG];
#pragma unroll
        for (int u = 0; u < LG; u++) {
          const long long at = i + lags.h[LG * g + u];
          v[u] = at < N ? x[at] - mean : 0.0;
        }
        if (g == 0) acc0 = __builtin_fma(xi, xi, acc0);
#pragma unroll
        for (int u = 0; u < LG; u++) acc[u] = __builtin_fma(xi, v[u], acc[u]);
      }
      if (g == 0) {
        acc0 = block_sum<SW>(acc0, s_red);
        if (tid == 0) { o[0] = mean; o[1] = acc0 / dn; o[2] = nf; nf_out[series] = nf; }
      }
#pragma unroll
      for (int u = 0; u < LG; u++) {
        if (LG * g + u < nlags) {
          const double v = block_sum<SW>(acc[u], s_red);
          if (tid == 0) o[LAG_HEAD + LG * g + u] = v / dn;
        }
      }
    }
  }
}

// Stages 1 and 2 for the window [row0, row0 + N) of every series: acov [series][ACS], stats [series][4].  With `active` (one
// entry per group of `cpg` consecutive chains) the masked kernels run, which leave the series of inactive groups alone.
int launch_series_stats(const char* who, hipStream_t st, const double* samples, long long S, int k, long long row0, long long N,
                        const int* cols, int p, long long series, double* acov, double* stats, long long cpg = 1,
                        const int* active = nullptr) {
  const int M = (int)ar_order_max(N);
  const int tile_rows = (int)(N < LDS_ROWS ? N : LDS_ROWS);
  const size_t lds = (size_t)(tile_rows + PAD + SW * RED) * sizeof(double);
  const int rc = active ? allow_lds(who, summary_series_masked_kernel, lds) : allow_lds(who, summary_series_kernel, lds);
  if (rc != FMCMC_OK) return rc;
  const dim3 ar_grid((unsigned)((series + 3) / 4));
  if (active) {
    hipLaunchKernelGGL(summary_series_masked_kernel, dim3((unsigned)series), dim3(ST), lds, st, samples, S, k, row0, N, cols, p, M,
                       tile_rows, cpg, active, acov);
    hipLaunchKernelGGL(summary_ar_masked_kernel, ar_grid, dim3(256), 0, st, acov, series, N, M, p, cpg, active, stats);
  } else {
    hipLaunchKernelGGL(summary_series_kernel, dim3((unsigned)series), dim3(ST), lds, st, samples, S, k, row0, N, cols, p, M,
                       tile_rows, acov);
    hipLaunchKernelGGL(summary_ar_kernel, ar_grid, dim3(256), 0, st, acov, series, N, M, stats);
  }
  return FMCMC_OK;
}

}  // namespace

extern "C" {

int64_t fmcmc_summary_pooled_len(int32_t p, int32_t nprobs) {
  if (p < 1 || nprobs < 0) return 0;
  return (int64_t)p * 5 + (int64_t)p * nprobs * 2;
}

int64_t fmcmc_summary_work_len(int64_t nchains, int32_t p, int32_t nprobs) {
  if (nchains < 1 || p < 1 || nprobs < 0) return 0;
  const int64_t series = nchains * (int64_t)p, targets = (int64_t)p * nprobs * 2;
  return series * ACS + series * 4 + targets * (3 + 256);
}

int fmcmc_summary_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                      const int32_t* cols, int32_t p, const double* probs, int32_t nprobs, double* work,
                      double* chain_stats, double* pooled, void* hip_stream) {
  const char* who = "fmcmc_summary_dev";
  int rc = check_window(who, samples, cols, work, pooled, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (nprobs < 0 || nprobs > MAXPROBS) return fail(FMCMC_ERR_ARG, "%s: nprobs = %d outside [0, %d]", who, (int)nprobs, MAXPROBS);
  if (nprobs > 0 && !probs) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  for (int q = 0; q < nprobs; q++)
    if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return fail(FMCMC_ERR_ARG, "%s: probs[%d] = %g is outside [0, 1]", who, q, probs[q]);

  hipStream_t st = (hipStream_t)hip_stream;
  const long long series = nchains * (long long)p;
  double* acov = work;
  double* stats = chain_stats ? chain_stats : work + series * ACS;
  unsigned long long* state = reinterpret_cast<unsigned long long*>(work + series * ACS + series * 4);
  const long long targets = (long long)p * nprobs * 2;
  unsigned long long* hist = state + 3 * targets;

  rc = launch_series_stats(who, st, samples, S, k, row0, N, cols, p, series, acov, stats);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(summary_pool_kernel, dim3((unsigned)p), dim3(256), 0, st, stats, acov, (long long)nchains, (int)p,
                     (long long)N, pooled);
  if (nprobs > 0) {
    Ranks ranks;                                 // among the pooled values of a column
    for (int q = 0; q < MAXPROBS; q++) {
      const Type7 r = type7_ranks(nchains * (long long)N, q < nprobs ? probs[q] : 0.0);
      ranks.lo[q] = r.lo; ranks.hi[q] = r.hi;
    }
    hipLaunchKernelGGL(select_init_kernel, dim3((unsigned)targets), dim3(256), 0, st, state, hist, (int)nprobs, ranks);
    const long long tiles = nchains * ((N + TILE - 1) / TILE);
    long long nblk = 2048 / p;
    if (nblk < 1) nblk = 1;
    if (nblk > tiles) nblk = tiles;
    for (int pass = 0; pass < 8; pass++) {
      hipLaunchKernelGGL(select_hist_kernel, dim3((unsigned)nblk, (unsigned)p), dim3(HT), (size_t)(2 * nprobs) * 256 * sizeof(unsigned int), st, samples, (long long)S, (int)k,
                         (long long)row0, (long long)N, (long long)nchains, cols, (int)nprobs, pass, state, hist);
      hipLaunchKernelGGL(select_scan_kernel, dim3((unsigned)p), dim3(64), 0, st, state, hist, (int)nprobs, pass,
                         pooled + (long long)p * 5);
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

int64_t fmcmc_summary_groups_work_len(int64_t ngroups, int64_t chains_per_group, int32_t p, int32_t nprobs) {
  if (ngroups < 1 || chains_per_group < 1 || p < 1 || nprobs < 0 || nprobs > MAXPROBS) return 0;
  if (chains_per_group > 0x7fffffffLL / ngroups || ngroups * chains_per_group > 0x7fffffffLL / p) return 0;
  return ngroups * chains_per_group * (int64_t)p * (ACS + 4);      // (the select keeps its state in LDS)
}

// fmcmc_summary_dev for ngroups groups of chains_per_group consecutive chains, each on its own: stages 1-2 over all chains (under
// `active` their masked forms), one pool workgroup and one select workgroup per (group, column).
int fmcmc_summary_groups_dev(const double* samples, int64_t ngroups, int64_t chains_per_group, int32_t k, int64_t S, int64_t row0,
                             int64_t N, const int32_t* cols, int32_t p, const int32_t* active, const double* probs, int32_t nprobs,
                             double* work, double* chain_stats, double* pooled, void* hip_stream) {
  const char* who = "fmcmc_summary_groups_dev";
  if (!samples || !cols || !work || !pooled) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (ngroups < 1 || chains_per_group < 1)
    return fail(FMCMC_ERR_ARG, "%s: ngroups = %lld, chains_per_group = %lld: each must be at least 1", who, (long long)ngroups,
                (long long)chains_per_group);
  if (chains_per_group > 0x7fffffffLL / ngroups)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld groups x %lld chains exceed one launch", who, (long long)ngroups,
                (long long)chains_per_group);
  const long long nchains = ngroups * chains_per_group;
  int rc = check_window(who, samples, cols, work, pooled, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (nprobs < 0 || nprobs > MAXPROBS) return fail(FMCMC_ERR_ARG, "%s: nprobs = %d outside [0, %d]", who, (int)nprobs, MAXPROBS);
  if (nprobs > 0 && !probs) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  for (int q = 0; q < nprobs; q++)
    if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return fail(FMCMC_ERR_ARG, "%s: probs[%d] = %g is outside [0, 1]", who, q, probs[q]);
  if (chains_per_group > 0xffffffffLL / N)          // (N < 3162278 here: the product below cannot overflow)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld chains x %lld rows in a group; the select of a group ranks fewer than 2^32 values",
                who, (long long)chains_per_group, (long long)N);

  hipStream_t st = (hipStream_t)hip_stream;
  const long long series = nchains * (long long)p, cpg = chains_per_group;
  const long long plen = fmcmc_summary_pooled_len(p, nprobs);
  double* acov = work;
  double* stats = chain_stats ? chain_stats : work + series * ACS;
  rc = launch_series_stats(who, st, samples, S, k, row0, N, cols, p, series, acov, stats, cpg, active);
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(summary_group_pool_kernel, dim3((unsigned)(ngroups * p)), dim3(256), 0, st, stats, acov, cpg, (int)p,
                     (long long)N, active, plen, pooled);
  if (nprobs > 0) {
    OrderRanks ranks;                            // among the pooled values of a group's column
    for (int q = 0; q < MAXPROBS; q++) {
      const Type7 r = type7_ranks(cpg * (long long)N, q < nprobs ? probs[q] : 0.0);
      ranks.r[2 * q] = (unsigned int)r.lo; ranks.r[2 * q + 1] = (unsigned int)r.hi;
    }
    const int staged = cpg * (long long)N <= LDS_ROWS;
    const size_t lds = staged ? (size_t)(cpg * N) * sizeof(unsigned long long) : 0;
    rc = allow_lds(who, summary_group_select_kernel, lds);
    if (rc != FMCMC_OK) return rc;
    hipLaunchKernelGGL(summary_group_select_kernel, dim3((unsigned)(ngroups * p)), dim3(SEL_T), lds, st, samples, (long long)S,
                       (int)k, (long long)row0, (long long)N, cpg, cols, (int)p, 2 * (int)nprobs, ranks, staged, active, plen, pooled);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

int64_t fmcmc_heidel_work_len(int64_t nchains, int32_t p, int64_t ncand) {
  if (nchains < 1 || p < 1 || ncand < 1 || nchains > 0x7fffffffLL / p) return 0;
  return nchains * (int64_t)p * ACS;
}

int64_t fmcmc_heidel_out_len(int64_t nchains, int32_t p, int64_t ncand) {
  if (nchains < 1 || p < 1 || ncand < 1 || nchains > 0x7fffffffLL / p || ncand > 0x7fffffffLL) return 0;
  return (1 + ncand) * nchains * (int64_t)p * 4 + ncand * nchains * (int64_t)p;
}

int fmcmc_heidel_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                     const int32_t* cols, int32_t p, int64_t half_row, const int64_t* cand_rows, int64_t ncand, double* work,
                     double* out, void* hip_stream) {
  const char* who = "fmcmc_heidel_dev";
  int rc = check_window(who, samples, cols, work, out, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (!cand_rows) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (ncand < 1) return fail(FMCMC_ERR_ARG, "%s: ncand = %lld, need at least one candidate start", who, (long long)ncand);
  if (ncand > 0x7fffffffLL) return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld candidates exceed what one call takes", who, (long long)ncand);
  if (half_row < 0 || N - half_row < 3)
    return fail(FMCMC_ERR_ARG, "%s: half_row = %lld leaves %lld of the %lld rows (spectrum0.ar needs 3)", who,
                (long long)half_row, (long long)(N - half_row), (long long)N);
  for (int64_t s = 0; s < ncand; s++) {
    if (cand_rows[s] < 0 || N - cand_rows[s] < 3)
      return fail(FMCMC_ERR_ARG, "%s: cand_rows[%lld] = %lld leaves %lld of the %lld rows (spectrum0.ar needs 3)", who,
                  (long long)s, (long long)cand_rows[s], (long long)(N - cand_rows[s]), (long long)N);
    if (s > 0 && cand_rows[s] < cand_rows[s - 1])
      return fail(FMCMC_ERR_ARG, "%s: cand_rows must ascend (cand_rows[%lld] = %lld after %lld)", who, (long long)s,
                  (long long)cand_rows[s], (long long)cand_rows[s - 1]);
  }
  if (half_row < cand_rows[0])
    return fail(FMCMC_ERR_ARG, "%s: half_row = %lld lies before cand_rows[0] = %lld (the S0 window must be part of "
                "the longest tail, whose non-finite count covers it)", who, (long long)half_row, (long long)cand_rows[0]);

  hipStream_t st = (hipStream_t)hip_stream;
  const long long series = nchains * (long long)p;
  double* q_out = out + (1 + ncand) * series * 4;
  // the S0 window, then the tails from the shortest to the longest: `work` is left holding the series work of cand_rows[0]
  rc = launch_series_stats(who, st, samples, S, k, row0 + half_row, N - half_row, cols, p, series, work, out);
  for (int64_t s = ncand - 1; s >= 0 && rc == FMCMC_OK; s--)
    rc = launch_series_stats(who, st, samples, S, k, row0 + cand_rows[s], N - cand_rows[s], cols, p, series, work,
                             out + (1 + s) * series * 4);
  if (rc != FMCMC_OK) return rc;
  for (int64_t s0 = 0; s0 < ncand; s0 += CVM_CANDS) {
    const int ns = (int)(ncand - s0 < CVM_CANDS ? ncand - s0 : CVM_CANDS);
    CvmCands cands;
    for (int s = 0; s < CVM_CANDS; s++) cands.lo[s] = cand_rows[s0 + (s < ns ? s : 0)];
    hipLaunchKernelGGL(summary_cvm_kernel, dim3((unsigned)series, (unsigned)ns), dim3(ST), 0, st, samples, (long long)S, (int)k,
                       (long long)row0, (long long)N, cols, (int)p, cands, out + (1 + s0) * series * 4, series,
                       q_out + s0 * series);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

int64_t fmcmc_autocov_out_len(int64_t nchains, int32_t p, int32_t nlags) {
  if (nchains < 1 || p < 1 || nlags < 1 || nlags > MAXLAGS || nchains > 0x7fffffffLL / p) return 0;
  return nchains * (int64_t)p * (LAG_HEAD + (int64_t)nlags);
}

int fmcmc_autocov_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* cols,
                      int32_t p, const int64_t* lags, int32_t nlags, double* work, double* out, void* hip_stream) {
  const char* who = "fmcmc_autocov_dev";
  int rc = check_window(who, samples, cols, work, out, nchains, k, S, row0, N, p);
  if (rc != FMCMC_OK) return rc;
  if (!lags) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (nlags < 1 || nlags > MAXLAGS) return fail(FMCMC_ERR_ARG, "%s: nlags = %d outside [1, %d]", who, (int)nlags, MAXLAGS);
  LagList ll;
  for (int l = 0; l < MAXLAGS; l++) {
    if (l < nlags) {
      if (lags[l] < 0 || lags[l] >= N)
        return fail(FMCMC_ERR_ARG, "%s: lags[%d] = %lld is outside [0, %lld)", who, l, (long long)lags[l], (long long)N);
      for (int u = 0; u < l; u++)
        if (lags[u] == lags[l]) return fail(FMCMC_ERR_ARG, "%s: lags[%d] = %lld repeats lags[%d]", who, l, (long long)lags[l], u);
    }
    ll.h[l] = (int)(l < nlags ? lags[l] : N);
  }
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(summary_lag_kernel, dim3((unsigned)(nchains * p)), dim3(ST), 0, st, samples, (long long)S, (int)k,
                     (long long)row0, (long long)N, cols, (int)p, (int)nlags, ll, work, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

}  // extern "C"

#include "diag_waic.hpp"   // fmcmc_waic_dev, fmcmc_waic_groups_dev (block_sum and diag_common.hpp come from above)
#include "diag_loo.hpp"    // fmcmc_loo_dev, fmcmc_loo_groups_dev (the plan, the draw kernel and the checks of diag_waic.hpp)
#include "diag_loo_predictive.hpp"   // fmcmc_loo_predictive_dev (the whole call of diag_loo.hpp, then one more sweep of its tiles)
#include "diag_pointwise.hpp"   // fmcmc_waic_fun_dev, fmcmc_loo_fun_dev (the plans, merges and finishing kernels of the two above)
#include "diag_predict.hpp"     // fmcmc_predict_dev (the split into parts of diag_waic.hpp, the keys of diag_common.hpp)
#include "diag_predictive.hpp"  // fmcmc_predictive_dev (the parts of diag_waic.hpp, the Chan merges and the checks of diag_predict.hpp)
#include "diag_ppc.hpp"         // fmcmc_ppc_dev, fmcmc_ppc_yrep_dev, fmcmc_ppc_elem_host (the checks and the draw kernel of diag_predict.hpp)
