// gelman.hip — cross-chain reduction behind convergence_gelman (R/convergence.R:191-246 ->
// coda::gelman.diag; formula restated in SURVEY.md App. A-4).
//
// Device side: per-chain window mean / covariance straight from the samples the sweep kernel left
// in HBM ([C][k][S], one chain = one column-major S x k matrix), then a fixed-order sum over the
// local chains into a small "partial" vector.  Partials of different GPUs ADD, so the only
// collective of the whole engine is one all-reduce(sum) of 1 + 5p + 2p^2 doubles per check.
// Host side: fmcmc_gelman_finish turns the reduced partial into psrf / mpsrf.
#include <vector>

#include "diag_common.hpp"

namespace {

constexpr int GT = 256;  // threads per block

// Per-chain window mean and covariance: work[c] = { xbar[p] - center, S_c[p*p] } of the window [row0, row0 + N).
//
// The window of one chain is a column-major N x p matrix D; its covariance is the rank-N update D'D -- the one GEMM-shaped
// piece of the whole engine besides the log-posterior, and at config C4 (512 chains x p = 50 x 5,000 rows: 1 GB, 13 GFLOP)
// it is as much arithmetic as memory traffic.  So it runs on the matrix cores: v_mfma_f64_16x16x4 with M = N = a block of
// 16 columns and K = 4 consecutive rows.  Both operands have the SAME lane layout (lane l holds row t0 + l / 16 of column
// 16 cb + l % 16), so a K-step loads one double per lane and column block and feeds every tile that holds the block.
// ONE pass over the data: rows are shifted by the chain's first window row (d = x - x[row0]).  The shift is a row of the
// window, so sum d_a^2 = (N - 1) E_a with E_a = S_aa + N / (N - 1) (x[row0] - mean)_a^2 <= N S_aa (the first row is at most
// sqrt(N - 1) window standard deviations from the window mean), and sum d d' - N dbar dbar' stays within (N + 32) u sqrt(E_a E_b) of S_ab, u = 2^-53
// (tests/gelman_ref.py derives it, tests/test_gpu_gelman_narrow.py holds the device to it).  The column sums ride along on
// the VALU.  The four waves take four contiguous row ranges and are combined through LDS in wave order; the result does
// not depend on the launch.  (The previous VALU version: one thread per column for the means, LDS-tiled pair products:
// 4.8 ms = 215 GB/s at C4's width.)
//
// The columns form super-blocks of 64 (four 16-column blocks), nsb = ceil(p / 64) of them, and one workgroup serves one
// (chain, super-block pair A <= B): above 64 columns the tiles of a whole chain no longer fit one wave's registers (136 tiles
// = 544 doubles per lane at p = 256), so the OUTPUT is tiled.  NA is the number of column blocks of A.  DIAG = true: the nsb
// pairs A == B, the NA (NA + 1) / 2 tiles ab <= bb; p <= 64 is nsb = 1 with NA = ceil(p / 16).  DIAG = false (NA = 4): the
// nsb (nsb - 1) / 2 pairs A < B, 16 tiles = 128 accumulator registers, eight column blocks per row group.  The column sums of
// a super-block are formed by every pair that holds it, by the same operations in the same order, so they agree to the bit
// between workgroups; the diagonal pair writes xbar.  Every tile is written with its mirror from one value, so S_c is
// exactly symmetric.  Three row groups are buffered (two loads in flight behind the one being multiplied) at four and at
// eight column blocks -- 128 accumulator registers + 3 x 64 of buffers, 440 of the 512 a lane has at one wave per SIMD, no
// scratch; two stages at eight blocks measured 5 to 7 % slower.  The window is read nsb times per chain (a
// super-block once by its diagonal pair and once by each of the nsb - 1 others).
typedef double gd4_t __attribute__((ext_vector_type(4)));
template <int NA, bool DIAG>
__global__ __launch_bounds__(GT) void gelman_cov_mfma(const double* __restrict__ samples, long long S, int k, long long row0,
                                                      long long N, const int* __restrict__ cols, int p, int nsb,
                                                      const double* __restrict__ center, double* __restrict__ work) {
  static_assert(DIAG || NA == 4, "an off-diagonal pair holds two whole super-blocks");
  constexpr int DEPTH = 3;                          // buffered row groups
  constexpr int NB = DIAG ? NA : 2 * NA;            // column blocks in flight: A's, then B's
  constexpr int NT = DIAG ? NA * (NA + 1) / 2 : NA * NA;   // tiles
  __shared__ double s_acc[NT * 256];                // [tile][lane * 4 + r]
  __shared__ double s_sum[NB * 16];                 // column sums of d
  __shared__ double s_shift[NB * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kk = lane >> 4, j = lane & 15;
  const int npairs = DIAG ? nsb : nsb * (nsb - 1) / 2;
  const long long c = blockIdx.x / npairs;
  int sa = (int)(blockIdx.x % npairs), sb = sa;
  if (!DIAG) {                                      // pairs in the order (0,1) (0,2) .. (0,nsb-1) (1,2) ..
    int rem = sa;
    sa = 0;
    while (rem >= nsb - 1 - sa) { rem -= nsb - 1 - sa; sa++; }
    sb = sa + 1 + rem;
  }
  const double* base = samples + c * (long long)k * S + row0;
  // this lane's column of every block (a padded column reads column 0 and is multiplied by 0)
  const double* colp[NB];
  double shift[NB], msk[NB], csum[NB];
#pragma unroll
  for (int cb = 0; cb < NB; cb++) {
    const int a = (cb < NA ? sa : sb) * 64 + (cb % NA) * 16 + j;
    colp[cb] = base + (long long)cols[a < p ? a : 0] * S;
    shift[cb] = colp[cb][0];
    msk[cb] = a < p ? 1.0 : 0.0;
    csum[cb] = 0.0;
  }
  gd4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = (gd4_t){0.0, 0.0, 0.0, 0.0};
  // Rows of this wave: a contiguous quarter of the window, in groups of 16.  Lane (kk, j) loads rows 4 kk .. 4 kk + 3 of the
  // group for its column -- 32 contiguous bytes, the four kk classes together a full 128-byte line per column -- and K-step s
  // of the group multiplies rows {4 kk + s}: which four rows share a K-step only changes the order of a sum.  DEPTH - 1 groups
  // are in flight behind the one being multiplied (the loads come from HBM: ~2 us, a group's 40 MFMAs are ~1 us).
  const long long groups = (N + 15) / 16, per = (groups + 3) / 4;
  const long long g_lo = wave * per, g_hi = (g_lo + per < groups) ? g_lo + per : groups;
  double buf[DEPTH][NB][4];
  auto load = [&](long long gi, double (&v)[NB][4]) {
    const long long t = 16 * gi + 4 * kk;
    if (t + 3 < N) {
#pragma unroll
      for (int cb = 0; cb < NB; cb++) {
        const dpair_t lo = *reinterpret_cast<const dpair_t*>(colp[cb] + t), hi = *reinterpret_cast<const dpair_t*>(colp[cb] + t + 2);
        v[cb][0] = lo[0]; v[cb][1] = lo[1]; v[cb][2] = hi[0]; v[cb][3] = hi[1];
      }
    } else {
#pragma unroll
      for (int cb = 0; cb < NB; cb++)
#pragma unroll
        for (int u = 0; u < 4; u++) v[cb][u] = (t + u < N) ? colp[cb][t + u] : shift[cb];   // (a row beyond the window: d = 0)
    }
  };
#pragma unroll
  for (int i = 0; i < DEPTH - 1; i++)
    if (g_lo + i < g_hi) load(g_lo + i, buf[i]);
  for (long long gi = g_lo; gi < g_hi; gi += DEPTH) {
#pragma unroll
    for (int ph = 0; ph < DEPTH; ph++) {       // buffer roles rotate statically
      if (gi + ph < g_hi) {
        if (gi + ph + DEPTH - 1 < g_hi) load(gi + ph + DEPTH - 1, buf[(ph + DEPTH - 1) % DEPTH]);
        double (&cur)[NB][4] = buf[ph];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          double d[NB];
#pragma unroll
          for (int cb = 0; cb < NB; cb++) { d[cb] = (cur[cb][u] - shift[cb]) * msk[cb]; csum[cb] += d[cb]; }
          int t = 0;                           // tiles in the order of (ab, bb): B's blocks start at NB - NA
#pragma unroll
          for (int ab = 0; ab < NA; ab++)
#pragma unroll
            for (int bb = DIAG ? ab : 0; bb < NA; bb++, t++)
              acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(d[ab], d[NB - NA + bb], acc[t], 0, 0, 0);
        }
      }
    }
  }
  // column sums: the four kk classes of a column sit in lanes j, j + 16, j + 32, j + 48
#pragma unroll
  for (int cb = 0; cb < NB; cb++) {
    double v = csum[cb];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    csum[cb] = v;
  }
  // waves combine in wave order
  for (int w = 0; w < 4; w++) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          double* d = &s_acc[t * 256 + lane * 4 + r];
          *d = (w == 0) ? acc[t][r] : *d + acc[t][r];
        }
      if (lane < 16) {
#pragma unroll
        for (int cb = 0; cb < NB; cb++) {
          double* d = &s_sum[cb * 16 + lane];
          *d = (w == 0) ? csum[cb] : *d + csum[cb];
          if (w == 0) s_shift[cb * 16 + lane] = shift[cb];
        }
      }
    }
    __syncthreads();
  }
  // finish: D register r of lane l is row 4 r + l / 16, column l % 16 of its tile; la / lb index s_sum, a / b2 the p columns
  double* wout = work + c * (long long)(p + p * p);
  const double dn = (double)N;
  if (DIAG && tid < NA * 16 && sa * 64 + tid < p)
    wout[sa * 64 + tid] = (s_shift[tid] + s_sum[tid] / dn) - (center ? center[sa * 64 + tid] : 0.0);
  for (int e = tid; e < NT * 256; e += GT) {
    const int t = e >> 8, q = e & 255, l = q >> 2, r = q & 3;
    int ab, bb;
    if (DIAG) {
      int rem = t;
      ab = 0;
      while (rem >= NA - ab) { rem -= NA - ab; ab++; }
      bb = ab + rem;
    } else {
      ab = (unsigned)t / NA;
      bb = (unsigned)t % NA;
    }
    const int la = ab * 16 + 4 * r + (l >> 4), lb = (NB - NA) * 16 + bb * 16 + (l & 15);
    const int a = sa * 64 + la, b2 = sb * 64 + lb - (NB - NA) * 16;
    if (a < p && b2 < p && (!DIAG || ab < bb || a <= b2)) {
      const double v = (s_acc[e] - s_sum[la] * s_sum[lb] / dn) / (dn - 1.0);
      wout[p + a * p + b2] = v;
      wout[p + b2 * p + a] = v;
    }
  }
}

// Fixed-order sum over the local chains -> partial.  64 elements of the partial per block, four threads per element: thread
// g sums the chains g, g + 4, g + 8, ... in chain order, the four sums are joined as ((g0 + g1) + g2) + g3.  (One block for
// everything -- 21 elements per thread, each a serial walk over 512 chains -- took 2.5 of the 3.0 ms of a check at C4.)
__global__ __launch_bounds__(GT) void gelman_sum_kernel(const double* __restrict__ work, long long C, int p,
                                                        double* __restrict__ partial) {
  __shared__ double s_g[4][64];
  const int el = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int stride = p + p * p;
  const int len = 1 + 5 * p + 2 * p * p;
  const int e = blockIdx.x * 64 + el;
  double s = 0.0;
  if (e < len) {
    if (e == 0) {
      s = (g == 0) ? (double)C : 0.0;
    } else if (e < 1 + p) {  // sum xbar
      int a = e - 1;
      for (long long c = g; c < C; c += 4) s += work[c * stride + a];
    } else if (e < 1 + p + p * p) {  // sum xbar xbar^T
      int ab = e - 1 - p, a = ab / p, b = ab % p;
      for (long long c = g; c < C; c += 4) s = __builtin_fma(work[c * stride + a], work[c * stride + b], s);
    } else if (e < 1 + p + 2 * p * p) {  // sum S_c
      int ab = e - 1 - p - p * p;
      for (long long c = g; c < C; c += 4) s += work[c * stride + p + ab];
    } else {
      int r = e - 1 - p - 2 * p * p, which = r / p, a = r % p;
      for (long long c = g; c < C; c += 4) {
        double s2 = work[c * stride + p + a * p + a], xb = work[c * stride + a];
        double v = (which == 0) ? s2 : (which == 1) ? s2 * s2 : (which == 2) ? s2 * xb : s2 * xb * xb;
        s += v;
      }
    }
  }
  s_g[g][el] = s;
  __syncthreads();
  if (g == 0 && e < len) partial[e] = ((s_g[0][el] + s_g[1][el]) + s_g[2][el]) + s_g[3][el];
}

// gelman_sum_kernel per GROUP of Cm consecutive chains (fmcmc_gelman_groups_dev: one model on many datasets, a group = the chains
// of one dataset): row grp of `partials` is, bit for bit, what gelman_sum_kernel leaves for the Cm chains of the group alone,
// centred on the window's first row of the group's first chain.  `work` holds the PLAIN window means (gelman_cov_mfma with
// center == NULL: xbar - 0.0 is xbar), so the one subtraction that kernel would have made is made here, where the group is known:
// xb = work - centre, with the centre read from the samples.  One block per (group, 64 elements of the row), four threads per
// element; thread g walks the chains g, g + 4, ... of the group, the four sums are joined as ((g0 + g1) + g2) + g3.
// A row has two more doubles than a partial: the sum and the sum of squares of every entry of the group's window, from the
// chains' means and variances (rm_invariant, R/convergence.R:171-173; convergence_gelman.check_device forms them with torch
// reductions), summed chain by chain and column by column within a chain: N sum xbar and sum ((N - 1) s2 + N xbar^2), xbar =
// xb + centre.  A group whose `active` entry is 0 leaves its row as it was; the test is uniform per block and comes first.
__global__ __launch_bounds__(GT) void gelman_group_sum_kernel(const double* __restrict__ work, const double* __restrict__ samples,
                                                              long long S, int k, long long row0, long long N,
                                                              const int* __restrict__ cols, long long Cm, int p, int nslices,
                                                              const int* __restrict__ active, double* __restrict__ partials) {
  __shared__ double s_g[4][64];
  const long long grp = blockIdx.x / nslices;
  if (active && active[grp] == 0) return;
  const int el = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int stride = p + p * p;
  const int len = 1 + 5 * p + 2 * p * p;
  const int e = (int)(blockIdx.x % nslices) * 64 + el;
  const double* w = work + grp * Cm * stride;                            // the group's chains
  const double* ctr = samples + grp * Cm * (long long)k * S + row0;       // centre of column a: ctr[cols[a] * S]
  const double dn = (double)N;
  double s = 0.0;
  if (e < len) {
    if (e == 0) {
      s = (g == 0) ? (double)Cm : 0.0;
    } else if (e < 1 + p) {  // sum xbar
      const int a = e - 1;
      const double ca = ctr[(long long)cols[a] * S];
      for (long long c = g; c < Cm; c += 4) s += w[c * stride + a] - ca;
    } else if (e < 1 + p + p * p) {  // sum xbar xbar^T
      const int ab = e - 1 - p, a = ab / p, b = ab % p;
      const double ca = ctr[(long long)cols[a] * S], cb = ctr[(long long)cols[b] * S];
      for (long long c = g; c < Cm; c += 4) s = __builtin_fma(w[c * stride + a] - ca, w[c * stride + b] - cb, s);
    } else if (e < 1 + p + 2 * p * p) {  // sum S_c
      const int ab = e - 1 - p - p * p;
      for (long long c = g; c < Cm; c += 4) s += w[c * stride + p + ab];
    } else {
      const int r = e - 1 - p - 2 * p * p, which = r / p, a = r % p;
      const double ca = ctr[(long long)cols[a] * S];
      for (long long c = g; c < Cm; c += 4) {
        double s2 = w[c * stride + p + a * p + a], xb = w[c * stride + a] - ca;
        double v = (which == 0) ? s2 : (which == 1) ? s2 * s2 : (which == 2) ? s2 * xb : s2 * xb * xb;
        s += v;
      }
    }
  } else if (e < len + 2) {  // every entry of the window: the sum (len), the sum of squares (len + 1)
    for (long long c = g; c < Cm; c += 4)
      for (int a = 0; a < p; a++) {
        const double ca = ctr[(long long)cols[a] * S];
        const double x = (w[c * stride + a] - ca) + ca, s2 = w[c * stride + p + a * p + a];
        s += (e == len) ? x : (dn - 1.0) * s2 + dn * x * x;
      }
  }
  s_g[g][el] = s;
  __syncthreads();
  if (g == 0 && e < len + 2) {
    const double v = ((s_g[0][el] + s_g[1][el]) + s_g[2][el]) + s_g[3][el];
    partials[grp * (len + 2) + e] = (e == len) ? dn * v : v;
  }
}

// Largest eigenvalue of a symmetric matrix (row-major, destroyed): Householder reduction to tridiagonal form, then the QL
// iteration with implicit shifts on the diagonal / sub-diagonal pair (eigenvalues only, nothing accumulated): O(p^3) once and
// O(p^2) per eigenvalue.  (The cyclic Jacobi sweeps this replaces ran until the off-diagonal norm was below 1e-300:
// 1.3-3 ms per check at p = 50, more than the device reduction of a 1 GB window.)  NaN when the iteration does not converge.
double top_eigenvalue_sym(std::vector<double>& a, int n) {
  std::vector<double> d(n), e(n);
  if (n == 1) return a[0];
  for (int i = n - 1; i >= 1; i--) {          // reduce row i with a Householder reflector built from a[i][0..i-1]
    const int l = i - 1;
    double h = 0.0, scale = 0.0;
    if (l > 0) {
      for (int k2 = 0; k2 <= l; k2++) scale += fabs(a[i * n + k2]);
      if (scale == 0.0) {
        e[i] = a[i * n + l];
      } else {
        for (int k2 = 0; k2 <= l; k2++) {
          a[i * n + k2] /= scale;
          h += a[i * n + k2] * a[i * n + k2];
        }
        double f = a[i * n + l];
        const double g = (f >= 0.0) ? -sqrt(h) : sqrt(h);
        e[i] = scale * g;
        h -= f * g;
        a[i * n + l] = f - g;
        f = 0.0;
        for (int j = 0; j <= l; j++) {
          double gg = 0.0;
          for (int k2 = 0; k2 <= j; k2++) gg += a[j * n + k2] * a[i * n + k2];
          for (int k2 = j + 1; k2 <= l; k2++) gg += a[k2 * n + j] * a[i * n + k2];
          e[j] = gg / h;
          f += e[j] * a[i * n + j];
        }
        const double hh = f / (h + h);
        for (int j = 0; j <= l; j++) {
          const double fj = a[i * n + j];
          const double gj = e[j] - hh * fj;
          e[j] = gj;
          for (int k2 = 0; k2 <= j; k2++) a[j * n + k2] -= fj * e[k2] + gj * a[i * n + k2];
        }
      }
    } else {
      e[i] = a[i * n + l];
    }
    d[i] = h;
  }
  e[0] = 0.0;
  for (int i = 0; i < n; i++) d[i] = a[i * n + i];
  // QL with implicit shifts
  for (int i = 1; i < n; i++) e[i - 1] = e[i];
  e[n - 1] = 0.0;
  for (int l = 0; l < n; l++) {
    int iter = 0, m2;
    do {
      for (m2 = l; m2 < n - 1; m2++) {
        const double dd = fabs(d[m2]) + fabs(d[m2 + 1]);
        if (fabs(e[m2]) <= 2.220446049250313e-16 * dd) break;
      }
      if (m2 != l) {
        if (iter++ == 60) return NAN;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = hypot(g, 1.0);
        g = d[m2] - d[l] + e[l] / (g + (g >= 0.0 ? fabs(r) : -fabs(r)));
        double s2 = 1.0, c2 = 1.0, p2 = 0.0;
        int i;
        for (i = m2 - 1; i >= l; i--) {
          double f = s2 * e[i];
          const double b2 = c2 * e[i];
          r = hypot(f, g);
          e[i + 1] = r;
          if (r == 0.0) {
            d[i + 1] -= p2;
            e[m2] = 0.0;
            break;
          }
          s2 = f / r;
          c2 = g / r;
          g = d[i + 1] - p2;
          r = (d[i] - g) * s2 + 2.0 * c2 * b2;
          p2 = s2 * r;
          d[i + 1] = g + p2;
          g = c2 * r - b2;
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p2;
        e[l] = g;
        e[m2] = 0.0;
      }
    } while (m2 != l);
  }
  double emax = d[0];
  for (int i = 1; i < n; i++)
    if (d[i] > emax) emax = d[i];
  return emax;
}

}  // namespace

extern "C" {

int64_t fmcmc_gelman_partial_len(int32_t p) { return 1 + 5 * (int64_t)p + 2 * (int64_t)p * p; }
int64_t fmcmc_gelman_work_len(int64_t nchains, int32_t p) { return nchains * ((int64_t)p + (int64_t)p * p); }

// 1 <= p <= FMCMC_MAX_K.  One workgroup per (chain, pair of 64-column super-blocks) of gelman_cov_mfma: the diagonal pairs (up to
// FMCMC_MAX_K_WAVE columns there is one, with ceil(p / 16) column blocks, and nothing else), then the off-diagonal ones.
int fmcmc_gelman_partial_dev(const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0,
                             int64_t N, const int32_t* cols, int32_t p, const double* center,
                             double* work, double* partial, void* hip_stream) {
  if (!samples || !cols || !work || !partial || p < 1 || p > FMCMC_MAX_K || nchains < 1 || N < 2 ||
      row0 < 0 || row0 + N > S)
    return FMCMC_ERR_ARG;
  hipStream_t st = (hipStream_t)hip_stream;
  const int nsb = (p + 63) / 64;                   // 1 .. 4
  if (p > FMCMC_MAX_K_WAVE && nchains > 0x7fffffff / 6) return FMCMC_ERR_ARG;
#define GELMAN_LAUNCH(NA, DIAG, NPAIRS)                                                                                      \
  hipLaunchKernelGGL((gelman_cov_mfma<NA, DIAG>), dim3((unsigned)(nchains * (NPAIRS))), dim3(GT), 0, st, samples, (long long)S, \
                     (int)k, (long long)row0, (long long)N, cols, (int)p, nsb, center, work)
  switch (nsb > 1 ? 4 : (p + 15) / 16) {
    case 1: GELMAN_LAUNCH(1, true, nsb); break;
    case 2: GELMAN_LAUNCH(2, true, nsb); break;
    case 3: GELMAN_LAUNCH(3, true, nsb); break;
    default: GELMAN_LAUNCH(4, true, nsb); break;
  }
  if (nsb > 1) GELMAN_LAUNCH(4, false, nsb * (nsb - 1) / 2);
#undef GELMAN_LAUNCH
  const int plen = 1 + 5 * (int)p + 2 * (int)p * (int)p;
  hipLaunchKernelGGL(gelman_sum_kernel, dim3((unsigned)((plen + 63) / 64)), dim3(GT), 0, st, work, (long long)nchains, (int)p, partial);
  return hipGetLastError() == hipSuccess ? FMCMC_OK : FMCMC_ERR_DEVICE;
}

int64_t fmcmc_gelman_groups_work_len(int64_t ngroups, int64_t chains_per_group, int32_t p) {
  return fmcmc_gelman_work_len(ngroups * chains_per_group, p);
}

// The reduction of fmcmc_gelman_partial_dev for ngroups groups of chains_per_group consecutive chains in two launches: the
// window means and covariances of ALL chains (gelman_cov_mfma, uncentred), then gelman_group_sum_kernel.  p <= FMCMC_MAX_K_WAVE.
int fmcmc_gelman_groups_dev(const double* samples, int64_t ngroups, int64_t chains_per_group, int32_t k, int64_t S, int64_t row0,
                            int64_t N, const int32_t* cols, int32_t p, const int32_t* active, double* work, double* partials,
                            void* hip_stream) {
  const char* who = "fmcmc_gelman_groups_dev";
  if (!samples || !cols || !work || !partials) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (ngroups < 1 || chains_per_group < 1 || k < 1 || p < 1)
    return fail(FMCMC_ERR_ARG, "%s: ngroups = %lld, chains_per_group = %lld, k = %d, p = %d: each must be at least 1", who,
                (long long)ngroups, (long long)chains_per_group, (int)k, (int)p);
  if (N < 2 || row0 < 0 || row0 + N > S)
    return fail(FMCMC_ERR_ARG, "%s: the window [%lld, %lld) needs at least two of the %lld rows of a chain", who, (long long)row0,
                (long long)(row0 + N), (long long)S);
  if (p > FMCMC_MAX_K_WAVE)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: p = %d columns; the grouped reduction takes up to FMCMC_MAX_K_WAVE = %d", who, (int)p,
                FMCMC_MAX_K_WAVE);
  const int plen = 1 + 5 * (int)p + 2 * (int)p * (int)p;
  const int nslices = (plen + 2 + 63) / 64;
  if (chains_per_group > 0x7fffffffLL / ngroups || ngroups > 0x7fffffffLL / nslices)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld groups x %lld chains exceed one launch", who, (long long)ngroups,
                (long long)chains_per_group);
  hipStream_t st = (hipStream_t)hip_stream;
  const long long nchains = ngroups * chains_per_group;
#define GELMAN_LAUNCH(NA)                                                                                                  \
  hipLaunchKernelGGL((gelman_cov_mfma<NA, true>), dim3((unsigned)nchains), dim3(GT), 0, st, samples, (long long)S, (int)k,  \
                     (long long)row0, (long long)N, cols, (int)p, 1, (const double*)nullptr, work)
  switch ((p + 15) / 16) {
    case 1: GELMAN_LAUNCH(1); break;
    case 2: GELMAN_LAUNCH(2); break;
    case 3: GELMAN_LAUNCH(3); break;
    default: GELMAN_LAUNCH(4); break;
  }
#undef GELMAN_LAUNCH
  hipLaunchKernelGGL(gelman_group_sum_kernel, dim3((unsigned)(ngroups * nslices)), dim3(GT), 0, st, work, samples, (long long)S,
                     (int)k, (long long)row0, (long long)N, cols, (long long)chains_per_group, (int)p, nslices, active, partials);
  return hipGetLastError() == hipSuccess ? FMCMC_OK : fail(FMCMC_ERR_DEVICE, "%s: the launch failed", who);
}

// Host finish. partial is the (all-reduced) vector; xbar sums are relative to `center`.
// psrf[p] point estimates (coda's "Point est."), *mpsrf multivariate (NaN when p == 1).
int fmcmc_gelman_finish(const double* P, int32_t p, int64_t N, double* psrf, double* mpsrf) {
  if (!P || p < 1 || p > FMCMC_MAX_K || N < 2) return FMCMC_ERR_ARG;   // (the host finish is general in p)
  const double m = P[0];
  if (m < 2) return FMCMC_ERR_ARG;
  const double* sx = P + 1;
  const double* sxx = sx + p;
  const double* sS = sxx + p * p;
  const double* s_s2 = sS + p * p;
  const double* s_s2s2 = s_s2 + p;
  const double* s_s2x = s_s2s2 + p;
  const double* s_s2xx = s_s2x + p;
  std::vector<double> W(p * p), B(p * p), mu(p);
  for (int a = 0; a < p; a++) mu[a] = sx[a] / m;
  for (int a = 0; a < p; a++)
    for (int b = 0; b < p; b++) {
      W[a * p + b] = sS[a * p + b] / m;
      B[a * p + b] = (double)N * (sxx[a * p + b] - m * mu[a] * mu[b]) / (m - 1);
    }
  for (int a = 0; a < p; a++) {
    double w = W[a * p + a], b = B[a * p + a];
    double ms2 = s_s2[a] / m;
    double var_s2 = (s_s2s2[a] - m * ms2 * ms2) / (m - 1);
    double mx2 = sxx[a * p + a] / m;
    double cov_s2_x2 = (s_s2xx[a] - m * ms2 * mx2) / (m - 1);
    double cov_s2_x = (s_s2x[a] - m * ms2 * mu[a]) / (m - 1);
    double var_w = var_s2 / m;
    double var_b = (2 * b * b) / (m - 1);
    double cov_wb = ((double)N / m) * (cov_s2_x2 - 2 * mu[a] * cov_s2_x);
    double V = (N - 1) * w / N + (1 + 1.0 / m) * b / N;
    double var_V = ((double)(N - 1) * (N - 1) * var_w + (1 + 1.0 / m) * (1 + 1.0 / m) * var_b +
                    2.0 * (N - 1) * (1 + 1.0 / m) * cov_wb) / ((double)N * N);
    double df_V = (2 * V * V) / var_V;
    double df_adj = (df_V + 3) / (df_V + 1);
    psrf[a] = sqrt(df_adj * ((double)(N - 1) / N + (1 + 1.0 / m) * (1.0 / N) * (b / w)));
  }
  *mpsrf = NAN;
  if (p > 1) {
    // L = chol(W) lower; Z = L^-1 B L^-T; largest eigenvalue by Householder tridiagonalisation and QL (top_eigenvalue_sym)
    std::vector<double> L(p * p, 0.0), Y(p * p), Z(p * p);
    for (int j = 0; j < p; j++) {
      double d = W[j * p + j];
      for (int b = 0; b < j; b++) d -= L[j * p + b] * L[j * p + b];
      if (!(d > 0.0)) return FMCMC_ERR_CHAIN;  // gelman.diag fails -> "not converged" (R/convergence.R:207-217)
      L[j * p + j] = sqrt(d);
      for (int i = j + 1; i < p; i++) {
        double s = W[i * p + j];
        for (int b = 0; b < j; b++) s -= L[i * p + b] * L[j * p + b];
        L[i * p + j] = s / L[j * p + j];
      }
    }
    for (int col = 0; col < p; col++)
      for (int a = 0; a < p; a++) {
        double s = B[a * p + col];
        for (int b = 0; b < a; b++) s -= L[a * p + b] * Y[b * p + col];
        Y[a * p + col] = s / L[a * p + a];
      }
    for (int col = 0; col < p; col++)
      for (int a = 0; a < p; a++) {
        double s = Y[col * p + a];
        for (int b = 0; b < a; b++) s -= L[a * p + b] * Z[b * p + col];
        Z[a * p + col] = s / L[a * p + a];
      }
    for (int a = 0; a < p; a++)
      for (int b = a + 1; b < p; b++) Z[a * p + b] = Z[b * p + a] = 0.5 * (Z[a * p + b] + Z[b * p + a]);
    const double emax = top_eigenvalue_sym(Z, p);
    if (!(emax == emax)) return FMCMC_ERR_CHAIN;
    *mpsrf = sqrt((1.0 - 1.0 / N) + (1.0 + 1.0 / p) * emax / N);
  }
  return FMCMC_OK;
}

}  // extern "C"
