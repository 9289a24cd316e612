// diag_loo.hpp — Pareto-smoothed importance-sampling leave-one-out (Vehtari, Gelman, Gabry 2017; Vehtari, Simpson, Gelman, Yao,
// Gabry 2024; loo::loo with r_eff = 1) of the three closed-form families from the kept rows where the sweep left them (the
// definition is INTEGRATION.md §2.2, the host restatement fmcmc_amd/summary.py: loo_host, the kernels, the miss probability and the
// times DESIGN.md §5.10).  Included by summary.hip behind diag_waic.hpp, whose plan of parts, draw kernel (a, w and the bad
// counts), layout of the partials and checks it reuses; the tile evaluation is WAIC's, restated here so that WAIC's object code
// is not touched.
//
// For every observation PSIS needs the M largest r = -l of the S draws, sorted, and the (M + 1)-th largest (the cutoff); the
// S x n matrix is never stored.  All order decisions are taken on the order-preserving 64-bit keys of the device's own r
// (diag_common.hpp: key_of), so "larger", "equal" and "smaller" are exact and total.
//   loo_tile_kernel<., SAMPLE>   evaluates the subsample (every `ustride`-th unit of 16 rows) into HBM: keys [n][ns16].
//   loo_thresh_kernel            a workgroup an observation: the key t of the `rank`-th largest of its subsample (radix select, 8
//                                passes of 8 bits, LDS histogram); zeroes the observation's counters and histogram.
//   loo_tile_kernel<., COLLECT>  one pass over all draws in WAIC's part structure: keys above t are counted (integer atomics) and
//                                appended to the observation's buffer of `cap` keys (beyond cap: counted only), keys equal to t
//                                are counted, r below t folds into sum exp(r - t) and sum exp(2 (r - t)) per lane, merged in the
//                                fixed lane-group order and written per (part, observation) next to the running (max, sum exp)
//                                of l that lppd needs.
//   loo_flag_kernel              an observation is a HIT when n_gt <= cap and n_gt + n_eq >= M + 1: then the buffer, followed by
//                                n_eq copies of t, holds the M + 1 largest.  Otherwise it is flagged.
//   8 x (loo_tile_kernel<., HIST>, loo_scan_kernel)   the fallback, which needs no luck: a most-significant-digit radix select
//                                over ALL draws for the exact key of the (M + 1)-th largest of every flagged observation
//                                (integer histogram in HBM); workgroups without a flagged observation leave at once.
//   loo_tile_kernel<., COLLECT>  again, for the flagged observations only, with t = that key: n_gt <= M and n_gt + n_eq >= M + 1
//                                hold by construction.
//   loo_finish_kernel            a workgroup an observation: bitonic sort of the buffer (descending, keys, in place), so that
//                                nothing depends on the order in which the atomics appended; the tail, the cutoff, the
//                                leftovers folded in sorted order, the generalised-Pareto fit (G x M log1p terms, the tail in
//                                LDS), the smoothing and the six numbers of `point`; where the internal launcher is given `lw`
//                                (diag_loo_predictive.hpp), the capped log weights of the tail ranks as well.
//   loo_total_kernel             a workgroup a group: sums, standard errors, the Pareto-k counts.
// The plan (loo_plan) is a function of (chains per group, N, n) alone; counts are integers; every floating sum has a fixed
// order: the same bits on every call, wherever the window sits and whichever groups share the call.
#pragma once

namespace {

constexpr int LOO_T = 256;              // threads of every kernel here
constexpr int LOO_RANK = 96;            // the least rank of the threshold in the subsample while the subsample is not everything
constexpr int LOO_MAX_M = 16384;        // the longest tail (S <= ~2.9e7)
constexpr int LOO_SUB_UNITS = 32;       // subsample units a workgroup of the sample pass
constexpr int LOO_STATE = 8;            // 8-byte slots per observation: t, n_gt, n_eq, flag, prefix, remaining rank, -, -
constexpr int LOO_MAX_G = 160;          // 30 + floor(sqrt(LOO_MAX_M)) = 158 candidates of the fit
enum { LOO_SAMPLE = 0, LOO_COLLECT = 1, LOO_HIST = 2 };
enum { LOO_ST_T = 0, LOO_ST_GT = 1, LOO_ST_EQ = 2, LOO_ST_FLAG = 3, LOO_ST_PREFIX = 4, LOO_ST_REM = 5 };

struct LooPlan {
  long long M, cap, target, ustride, nsu, ns16, ns_rows, rank, sparts;
  long long off_sub, off_buf, off_state, off_hist, len;
};

__host__ __device__ inline long long loo_isqrt(long long v) {   // floor(sqrt(v)), exact
  long long r = (long long)sqrt((double)v);
  while (r * r > v) r--;
  while ((r + 1) * (r + 1) <= v) r++;
  return r;
}

// M = ceil(min(0.2 S, 3 sqrt(S))), in integers
inline long long loo_tail_len(long long S) {
  const long long a = (S + 4) / 5;
  long long b = loo_isqrt(9 * S);
  if (b * b < 9 * S) b++;
  return a < b ? a : b;
}

// cap = the power of two >= 3 M; target = the expected count above the threshold = sqrt(M cap) (the geometric middle of the
// window [M + 1, cap]); the subsample = the units u = 0, ustride, 2 ustride, ... with ustride = max(1, target / LOO_RANK), so
// the threshold sits at rank ~ target / ustride >= LOO_RANK of the subsample, or the subsample is every draw and the threshold
// is exact.
inline LooPlan loo_plan(const WaicPlan& W, long long G, long long cpg, long long N, long long n) {
  LooPlan L;
  const long long S = cpg * N;
  L.M = loo_tail_len(S);
  L.cap = 4;
  while (L.cap < 3 * L.M) L.cap *= 2;
  long long t = loo_isqrt(L.M * L.cap);
  if (t < L.M + 1) t = L.M + 1;
  L.target = t < S ? t : S;
  L.ustride = L.target / LOO_RANK > 1 ? L.target / LOO_RANK : 1;
  L.nsu = (W.U + L.ustride - 1) / L.ustride;
  L.ns16 = 16 * L.nsu;
  long long rows = 0;
  for (long long c = 0; c < cpg; c++) {
    const long long lo = c * W.T, hi = lo + W.T - 1, first = (lo + L.ustride - 1) / L.ustride * L.ustride;
    if (first > hi) continue;
    const long long cnt = (hi - first) / L.ustride + 1;
    rows += 16 * cnt - ((first + (cnt - 1) * L.ustride == hi) ? 16 * W.T - N : 0);
  }
  L.ns_rows = rows;
  long long rk = (rows * L.target + S / 2) / S;
  L.rank = rk < 1 ? 1 : (rk > rows ? rows : rk);
  L.sparts = (L.nsu + LOO_SUB_UNITS - 1) / LOO_SUB_UNITS;
  L.off_sub = W.len;
  L.off_buf = L.off_sub + G * n * L.ns16;
  L.off_state = L.off_buf + G * n * L.cap;
  L.off_hist = L.off_state + G * n * LOO_STATE;
  L.len = L.off_hist + G * n * 128;
  return L;
}

struct LooArgs {
  WaicArgs W;
  LooPlan L;
  double* point; double* tail; double* total;
  double* lw = nullptr;                 // [n][M] or null: the capped log weights of the tail ranks, ascending (diag_loo_predictive.hpp)
  double tau;
  int pass, only;
};

// (max, sum exp) of a, then of b; a side with E == 0 is empty and leaves the other as it is
__device__ __forceinline__ void loo_lse_merge(double& aM, double& aE, double bM, double bE) {
  if (bE == 0.0) return;
  if (aE == 0.0) { aM = bM; aE = bE; return; }
  const double m = aM > bM ? aM : bM;
  aE = fmh_fma(aE, fmh_exp(aM - m), bE * fmh_exp(bM - m));
  aM = m;
}

// The tile evaluation of waic_tile_kernel (diag_waic.hpp) with another use of every l.  NQR: the steps of four operand columns
// whose B values a lane keeps in registers; 0: the B tile lives in LDS.
template <int NQR, int MODE>
__global__ __launch_bounds__(LOO_T) void loo_tile_kernel(LooArgs Q) {
  constexpr bool LDSB = NQR == 0;
  constexpr int NB = NQR ? NQR : 1;
  extern __shared__ double s_b[];
  const WaicArgs& A = Q.W;
  const WaicPlan& P = A.P;
  const LooPlan& L = Q.L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, col = lane & 15;
  const long long g = blockIdx.x / P.tiles, tile = blockIdx.x - g * P.tiles, part = blockIdx.y;
  if (A.active && !A.active[g]) return;
  const long long obs = tile * 64 + wave * 16 + col;
  const bool obs_ok = obs < A.n;
  const long long go = g * A.n + (obs_ok ? obs : 0);
  unsigned long long* __restrict__ st = reinterpret_cast<unsigned long long*>(A.work + L.off_state) + go * LOO_STATE;
  bool mine = obs_ok;
  unsigned long long tkey = 0ull, prefix = 0ull;
  if (MODE != LOO_SAMPLE) {
    if (MODE == LOO_HIST || Q.only) {
      mine = obs_ok && st[LOO_ST_FLAG] != 0ull;
      if (!__syncthreads_or(mine ? 1 : 0)) return;
    }
    if (mine) { tkey = st[LOO_ST_T]; prefix = st[LOO_ST_PREFIX]; }
  }
  const double tval = value_of(tkey);
  const double* __restrict__ X = A.X + g * A.x_stride;
  const double* __restrict__ y = A.y + g * A.y_stride;
  const int nq = P.nq, ncoef = P.ncoef, onecol = P.onecol;
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

  long long i0, i1;
  if (MODE == LOO_SAMPLE) {
    i0 = part * LOO_SUB_UNITS;
    i1 = i0 + LOO_SUB_UNITS < L.nsu ? i0 + LOO_SUB_UNITS : L.nsu;
  } else {
    i0 = part * P.upp;
    i1 = i0 + P.upp < P.U ? i0 + P.upp : P.U;
  }
  const double* __restrict__ smp = A.samples + g * A.cpg * A.k * A.S + A.row0;
  const double* __restrict__ av = A.work + g * A.cpg * A.N;
  const double* __restrict__ wv = av + P.off_w;
  unsigned long long* __restrict__ sub = reinterpret_cast<unsigned long long*>(A.work + L.off_sub) + go * L.ns16;
  unsigned long long* __restrict__ buf = reinterpret_cast<unsigned long long*>(A.work + L.off_buf) + go * L.cap;
  unsigned int* __restrict__ hist = reinterpret_cast<unsigned int*>(A.work + L.off_hist) + go * 256;
  double Mx = -fmh_inf(), E = 0.0, a1 = 0.0, a2 = 0.0;
  unsigned long long neq = 0ull;
  for (long long idx = i0; idx < i1; idx++) {
    const long long u = MODE == LOO_SAMPLE ? idx * L.ustride : idx;
    const long long c = u / P.T, t = u - c * P.T;
    const long long rb = 16 * t;
    const int valid = A.N - rb < 16 ? (int)(A.N - rb) : 16;
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
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int rr = 4 * r + kk;
      if (!mine) continue;
      if (rr >= valid) {
        if (MODE == LOO_SAMPLE) sub[idx * 16 + rr] = 0ull;      // (below every key: a row that does not exist)
        continue;
      }
      const double eta = acc[r];
      double l;
      if (P.gauss) {
        const long long di = c * A.N + rb + rr;
        l = fmh_fma(-wv[di], eta * eta, av[di]);
      } else {
        const double ts = ypos ? eta : -eta;
        l = (ts < 0.0 ? ts : 0.0) - fmh_log1p(fmh_exp(-fmh_abs(ts)));
      }
      const double rv = -l;
      const unsigned long long key = key_of(rv);
      if (MODE == LOO_SAMPLE) {
        sub[idx * 16 + rr] = key;
      } else if (MODE == LOO_HIST) {
        if (radix_high(key, Q.pass) == prefix) atomicAdd(&hist[radix_digit(key, Q.pass)], 1u);
      } else {
        const double x = l - Mx, ex = fmh_exp(-fmh_abs(x));
        if (x > 0.0) { E = fmh_fma(E, ex, 1.0); Mx = l; }
        else E += ex;
        if (key > tkey) {
          const unsigned long long slot = atomicAdd(&st[LOO_ST_GT], 1ull);
          if (slot < (unsigned long long)L.cap) buf[slot] = key;
        } else if (key == tkey) {
          neq++;
        } else {
          const double e = fmh_exp(rv - tval);
          a1 += e;
          a2 = fmh_fma(e, e, a2);
        }
      }
    }
  }
  if (MODE == LOO_COLLECT) {
    if (mine && neq) atomicAdd(&st[LOO_ST_EQ], neq);
    double mM = 0.0, mE = 0.0, m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int gs = 0; gs < 4; gs++) {                   // the four lane groups of an observation, ((0 + 1) + 2) + 3
      const int src = col + 16 * gs;
      const double oM = __shfl(Mx, src, 64), oE = __shfl(E, src, 64), o1 = __shfl(a1, src, 64), o2 = __shfl(a2, src, 64);
      if (gs == 0) { mM = oM; mE = oE; m1 = o1; m2 = o2; }
      else { loo_lse_merge(mM, mE, oM, oE); m1 += o1; m2 += o2; }
    }
    if (kk == 0 && mine) {
      double* o = A.work + P.off_part + ((g * P.nparts + part) * A.n + obs) * 4;
      o[0] = mM; o[1] = mE; o[2] = m1; o[3] = m2;
    }
  }
}

// The key of the `rank`-th largest (1-based) of the subsample of an observation; the observation's counters start at zero.
__global__ __launch_bounds__(LOO_T) void loo_thresh_kernel(LooArgs Q) {
  __shared__ unsigned int h[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned int s_rank;
  const WaicArgs& A = Q.W;
  const LooPlan& L = Q.L;
  const long long g = blockIdx.y, obs = blockIdx.x, go = g * A.n + obs;
  if (A.active && !A.active[g]) return;
  const int tid = threadIdx.x;
  const unsigned long long* __restrict__ sub = reinterpret_cast<const unsigned long long*>(A.work + L.off_sub) + go * L.ns16;
  if (tid == 0) { s_prefix = 0ull; s_rank = (unsigned int)L.rank; }
  for (int pass = 0; pass < 8; pass++) {
    h[tid] = 0u;
    __syncthreads();
    const unsigned long long prefix = s_prefix;
    for (long long i = tid; i < L.ns16; i += LOO_T) {
      const unsigned long long key = sub[i];
      if (radix_high(key, pass) == prefix) atomicAdd(&h[radix_digit(key, pass)], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned int r = s_rank;
      int bin = 255;
      for (; bin > 0; bin--) {
        if (r <= h[bin]) break;
        r -= h[bin];
      }
      s_prefix = (prefix << 8) | (unsigned long long)bin;
      s_rank = r;
    }
    __syncthreads();
  }
  unsigned long long* __restrict__ st = reinterpret_cast<unsigned long long*>(A.work + L.off_state) + go * LOO_STATE;
  unsigned int* __restrict__ hist = reinterpret_cast<unsigned int*>(A.work + L.off_hist) + go * 256;
  hist[tid] = 0u;
  if (tid < LOO_STATE) st[tid] = tid == LOO_ST_T ? s_prefix : 0ull;
}

__global__ __launch_bounds__(LOO_T) void loo_flag_kernel(LooArgs Q) {
  const WaicArgs& A = Q.W;
  const LooPlan& L = Q.L;
  const long long g = blockIdx.y, obs = (long long)blockIdx.x * LOO_T + threadIdx.x;
  if (A.active && !A.active[g]) return;
  if (obs >= A.n) return;
  unsigned long long* __restrict__ st = reinterpret_cast<unsigned long long*>(A.work + L.off_state) + (g * A.n + obs) * LOO_STATE;
  const unsigned long long ngt = st[LOO_ST_GT], neq = st[LOO_ST_EQ];
  const bool hit = ngt <= (unsigned long long)L.cap && ngt + neq >= (unsigned long long)(L.M + 1);
  st[LOO_ST_FLAG] = hit ? 0ull : 1ull;
  st[LOO_ST_PREFIX] = 0ull;
  st[LOO_ST_REM] = (unsigned long long)(L.M + 1);
}

// Pass Q.pass of the fallback's radix select: the digit of the (M + 1)-th largest key among those that share the prefix.
__global__ __launch_bounds__(LOO_T) void loo_scan_kernel(LooArgs Q) {
  const WaicArgs& A = Q.W;
  const LooPlan& L = Q.L;
  const long long g = blockIdx.y, obs = (long long)blockIdx.x * LOO_T + threadIdx.x;
  if (A.active && !A.active[g]) return;
  if (obs >= A.n) return;
  unsigned long long* __restrict__ st = reinterpret_cast<unsigned long long*>(A.work + L.off_state) + (g * A.n + obs) * LOO_STATE;
  if (st[LOO_ST_FLAG] == 0ull) return;
  unsigned int* __restrict__ hist = reinterpret_cast<unsigned int*>(A.work + L.off_hist) + (g * A.n + obs) * 256;
  unsigned long long r = st[LOO_ST_REM];
  int bin = 255;
  for (; bin > 0; bin--) {
    const unsigned long long c = hist[bin];
    if (r <= c) break;
    r -= c;
  }
  for (int q = 0; q < 256; q++) hist[q] = 0u;
  const unsigned long long prefix = (st[LOO_ST_PREFIX] << 8) | (unsigned long long)bin;
  st[LOO_ST_PREFIX] = prefix;
  st[LOO_ST_REM] = r;
  if (Q.pass == 7) { st[LOO_ST_T] = prefix; st[LOO_ST_GT] = 0ull; st[LOO_ST_EQ] = 0ull; }
}

__global__ __launch_bounds__(LOO_T) void loo_finish_kernel(LooArgs Q) {
  extern __shared__ double s_x[];                    // [M]: x of the fit, then the log weights of the tail
  __shared__ double red[LOO_T / 64];
  __shared__ double s_theta[LOO_MAX_G], s_ell[LOO_MAX_G];
  __shared__ double s_part[4];
  constexpr int NW = LOO_T / 64;
  const WaicArgs& A = Q.W;
  const WaicPlan& P = A.P;
  const LooPlan& L = Q.L;
  const long long g = blockIdx.y, obs = blockIdx.x, go = g * A.n + obs;
  if (A.active && !A.active[g]) return;
  const int tid = threadIdx.x;
  const long long M = L.M;
  const unsigned long long* __restrict__ st = reinterpret_cast<const unsigned long long*>(A.work + L.off_state) + go * LOO_STATE;
  unsigned long long* buf = reinterpret_cast<unsigned long long*>(A.work + L.off_buf) + go * L.cap;
  double* __restrict__ out = Q.point + go * 6;
  const unsigned long long ngt_u = st[LOO_ST_GT], neq_u = st[LOO_ST_EQ];
  const double tval = value_of(st[LOO_ST_T]);
  if (!(ngt_u <= (unsigned long long)L.cap && ngt_u + neq_u >= (unsigned long long)(M + 1))) {
    if (tid < 6) out[tid] = fmh_nan();               // (only draws that are not numbers bring this about)
    return;
  }
  const long long ngt = (long long)ngt_u, neq = (long long)neq_u;
  // the buffer, descending: a bitonic network on the keys, padded with the key below every key
  long long n2 = 1;
  while (n2 < ngt) n2 *= 2;
  for (long long i = ngt + tid; i < n2; i += LOO_T) buf[i] = 0ull;
  __syncthreads();
  for (long long k2 = 2; k2 <= n2; k2 <<= 1) {
    for (long long j = k2 >> 1; j > 0; j >>= 1) {
      for (long long i = tid; i < n2; i += LOO_T) {
        const long long p = i ^ j;
        if (p > i) {
          const unsigned long long a = buf[i], c = buf[p];
          const bool desc = (i & k2) == 0;
          if (desc ? a < c : a > c) { buf[i] = c; buf[p] = a; }
        }
      }
      __syncthreads();
    }
  }
  auto v = [&](long long j) -> double { return j < ngt ? value_of(buf[j]) : tval; };   // the j-th largest r, 0-based
  const double R = v(0), cutoff = v(M), cut = cutoff - R;
  if (Q.tail)
    for (long long j = tid; j < M; j += LOO_T) Q.tail[go * M + j] = v(M - 1 - j);
  // the draws below the tail: the rest of the buffer in sorted order, the copies of t the tail did not take, the folded parts
  double f1 = 0.0, f2 = 0.0;
  for (long long j = M + tid; j < ngt; j += LOO_T) {
    const double e = fmh_exp(v(j) - R);
    f1 += e;
    f2 = fmh_fma(e, e, f2);
  }
  f1 = block_sum<NW>(f1, red);
  f2 = block_sum<NW>(f2, red);
  if (tid == 0) {
    double mM = 0.0, mE = 0.0, m1 = 0.0, m2 = 0.0;
    for (long long part = 0; part < P.nparts; part++) {
      const double* __restrict__ o = A.work + P.off_part + ((g * P.nparts + part) * A.n + obs) * 4;
      if (part == 0) { mM = o[0]; mE = o[1]; m1 = o[2]; m2 = o[3]; }
      else { loo_lse_merge(mM, mE, o[0], o[1]); m1 += o[2]; m2 += o[3]; }
    }
    s_part[0] = mM; s_part[1] = mE; s_part[2] = m1; s_part[3] = m2;
  }
  __syncthreads();
  const double draws = (double)(A.cpg * A.N);
  const double lppd = s_part[0] + fmh_log(s_part[1] / draws);
  long long in_tail = M - ngt;
  in_tail = in_tail < 0 ? 0 : (in_tail > neq ? neq : in_tail);
  const double rest = (double)(neq - in_tail), et = fmh_exp(tval - R);
  const double low1 = et * (s_part[2] + rest) + f1, low2 = et * et * (s_part[3] + rest) + f2;

  // the tail, ascending: tl_j = v(M - j) - R, j = 1 .. M
  double kpar = fmh_inf();
  bool smooth = false;
  double sigma = 0.0;
  const double ecut = fmh_exp(cut);
  if (M >= 5 && -(v(M - 1) - R) >= 2.220446049250313e-16 / 100.0) {
    for (long long j = tid; j < M; j += LOO_T) s_x[j] = ecut * expm1((v(M - 1 - j) - R) - cut);
    __syncthreads();
    const int G = 30 + (int)loo_isqrt(M);
    const double xM = s_x[M - 1], xstar = s_x[(M + 2) / 4 - 1], dM = (double)M;
    for (int jt = 1; jt <= G; jt++) {
      const double theta = 1.0 / xM + (1.0 - fmh_sqrt((double)G / ((double)jt - 0.5))) / (3.0 * xstar);
      double s = 0.0;
      for (long long i = tid; i < M; i += LOO_T) s += fmh_log1p(-theta * s_x[i]);
      const double kappa = block_sum<NW>(s, red) / dM;
      if (tid == 0) {
        s_theta[jt - 1] = theta;
        s_ell[jt - 1] = dM * (fmh_log(-theta / kappa) - kappa - 1.0);
      }
    }
    __syncthreads();
    double top = s_ell[0];
    for (int jt = 1; jt < G; jt++) top = s_ell[jt] > top ? s_ell[jt] : top;
    double den = 0.0, num = 0.0;
    for (int jt = 0; jt < G; jt++) {
      const double w = fmh_exp(s_ell[jt] - top);
      den += w;
      num = fmh_fma(s_theta[jt], w, num);
    }
    const double that = num / den;
    double s = 0.0;
    for (long long i = tid; i < M; i += LOO_T) s += fmh_log1p(-that * s_x[i]);
    const double kraw = block_sum<NW>(s, red) / dM;
    sigma = -kraw / that;
    const double kk = (dM * kraw + 5.0) / (dM + 10.0);
    if (fmh_isfinite(kk)) { kpar = kk; smooth = true; }
    __syncthreads();
  }
  // the log weights of the tail into s_x
  const double dM = (double)M;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  for (long long j = tid; j < M; j += LOO_T) {
    const double tl = v(M - 1 - j) - R;
    double lw = tl;
    if (smooth) {
      const double p = ((double)(j + 1) - 0.5) / dM;
      lw = fmh_log(ecut + sigma * expm1(-kpar * fmh_log1p(-p)) / kpar);
    }
    lw = lw < 0.0 ? lw : 0.0;
    if (Q.lw) Q.lw[go * M + j] = lw;
    const double e = fmh_exp(lw);
    t0 += fmh_exp(lw - tl);
    t1 += e;
    t2 = fmh_fma(e, e, t2);
  }
  t0 = block_sum<NW>(t0, red);
  t1 = block_sum<NW>(t1, red);
  t2 = block_sum<NW>(t2, red);
  if (tid == 0) {
    const double den = low1 + t1;
    const double elpd = -R + fmh_log((draws - dM) + t0) - fmh_log(den);
    out[0] = elpd; out[1] = lppd - elpd; out[2] = lppd; out[3] = kpar; out[4] = den * den / (low2 + t2); out[5] = cutoff;
  }
}

__global__ __launch_bounds__(LOO_T) void loo_total_kernel(LooArgs Q) {
  __shared__ double red[LOO_T / 64];
  const WaicArgs& A = Q.W;
  const long long g = blockIdx.x;
  if (A.active && !A.active[g]) return;
  const double* __restrict__ pt = Q.point + g * A.n * 6;
  constexpr int NW = LOO_T / 64;
  double s[3] = {0.0, 0.0, 0.0}, nbad = 0.0, nvery = 0.0, badp = 0.0, badd = 0.0, kmax = -fmh_inf();
  for (long long i = threadIdx.x; i < A.n; i += LOO_T) {
    const double e = pt[6 * i], pl = pt[6 * i + 1], l = pt[6 * i + 2], kp = pt[6 * i + 3], ne = pt[6 * i + 4];
    s[0] += e; s[1] += pl; s[2] += l;
    nbad += kp > Q.tau ? 1.0 : 0.0;
    nvery += kp > 1.0 ? 1.0 : 0.0;
    kmax = kp > kmax ? kp : kmax;
    badp += (fmh_isfinite(e) && fmh_isfinite(pl) && fmh_isfinite(l) && fmh_isfinite(ne) && kp == kp) ? 0.0 : 1.0;
  }
  for (long long i = threadIdx.x; i < A.P.nblk; i += LOO_T) badd += A.work[A.P.off_bad + g * A.P.nblk + i];
  const double dn = (double)A.n;
  double sum[3], var[3];
  for (int q = 0; q < 3; q++) sum[q] = block_sum<NW>(s[q], red);
  double vv[3] = {0.0, 0.0, 0.0};
  for (long long i = threadIdx.x; i < A.n; i += LOO_T)
    for (int q = 0; q < 3; q++) {
      const double d = pt[6 * i + q] - sum[q] / dn;
      vv[q] = fmh_fma(d, d, vv[q]);
    }
  for (int q = 0; q < 3; q++) var[q] = block_sum<NW>(vv[q], red) / (dn - 1.0);
  nbad = block_sum<NW>(nbad, red);
  nvery = block_sum<NW>(nvery, red);
  badp = block_sum<NW>(badp, red);
  badd = block_sum<NW>(badd, red);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const double w = __shfl_xor(kmax, o, 64); kmax = w > kmax ? w : kmax; }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = kmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; w++) kmax = red[w] > kmax ? red[w] : kmax;
    double* o = Q.total + g * 12;
    o[0] = sum[0]; o[1] = sum[1]; o[2] = sum[2]; o[3] = -2.0 * sum[0];
    for (int q = 0; q < 3; q++) o[4 + q] = fmh_sqrt(dn * var[q]);
    o[7] = nbad; o[8] = nvery; o[9] = kmax; o[10] = badd; o[11] = badp;
  }
}

// Every check of the entries, before any device call.
inline int loo_check(const char* who, const fmcmc_model* m, int64_t x_stride, int64_t y_stride, const void* samples, int64_t G,
                     int64_t cpg, int32_t k, int64_t S, int64_t row0, int64_t N) {
  if (!m || !samples) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  if (cpg == 1 && N == 1) return fail(FMCMC_ERR_ARG, "%s: S = 1 draw: LOO needs at least 2", who);
  const int rc = waic_check(who, m, x_stride, y_stride, samples, G, cpg, k, S, row0, N);
  if (rc != FMCMC_OK) return rc;
  if (loo_tail_len(cpg * N) > LOO_MAX_M)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld draws ask for a tail of %lld; supported are tails up to %d (S <= 29826161)", who,
                (long long)(cpg * N), loo_tail_len(cpg * N), LOO_MAX_M);
  if (m->n > 0x7fffffffLL) return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld observations exceed one launch", who, (long long)m->n);
  return FMCMC_OK;
}

template <int MODE>
int loo_launch_tiles(const char* who, const LooArgs& Q, unsigned G, unsigned gy, hipStream_t st) {
  const WaicPlan& P = Q.W.P;
  const dim3 grid((unsigned)(P.tiles * G), gy);
  if (P.nq <= 4) {
    hipLaunchKernelGGL((loo_tile_kernel<4, MODE>), grid, dim3(LOO_T), 0, st, Q);
  } else {
    const size_t lds = (size_t)P.nq * LOO_T * sizeof(double);
    const int rc = allow_lds(who, loo_tile_kernel<0, MODE>, lds);
    if (rc != FMCMC_OK) return rc;
    hipLaunchKernelGGL((loo_tile_kernel<0, MODE>), grid, dim3(LOO_T), lds, st, Q);
  }
  return FMCMC_OK;
}

int loo_run(const char* who, const fmcmc_model* m0, int64_t x_stride, int64_t y_stride, const double* samples, int64_t ngroups,
            int64_t chains_per_group, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* active, double* work,
            double* point, double* tail, double* lw, double* total, void* hip_stream) {
  if (!work || !point || !total) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = loo_check(who, m0, x_stride, y_stride, samples, ngroups, chains_per_group, k, S, row0, N);
  if (rc != FMCMC_OK) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  LooArgs Q;
  WaicArgs& A = Q.W;
  A.samples = samples; A.X = m0->X; A.y = m0->y; A.active = active; A.work = work;
  A.x_stride = x_stride; A.y_stride = y_stride; A.S = S; A.row0 = row0; A.N = N; A.n = m0->n; A.cpg = chains_per_group;
  A.k = k;
  A.P = waic_plan(m0, ngroups, chains_per_group, N);
  Q.L = loo_plan(A.P, ngroups, chains_per_group, N, m0->n);
  Q.point = point; Q.tail = tail; Q.lw = lw; Q.total = total;
  const double dS = (double)(chains_per_group * N), tau = 1.0 - 1.0 / log10(dS);
  Q.tau = tau < 0.7 ? tau : 0.7;
  Q.pass = 0; Q.only = 0;
  const WaicPlan& P = A.P;
  const LooPlan& L = Q.L;
  const unsigned G = (unsigned)ngroups;
  const dim3 per_obs((unsigned)((A.n + LOO_T - 1) / LOO_T), G), wg_obs((unsigned)A.n, G);
  const size_t lds = (size_t)L.M * sizeof(double);
  if (lds > 65536 && (rc = allow_lds(who, loo_finish_kernel, lds)) != FMCMC_OK) return rc;
  hipLaunchKernelGGL(waic_draw_kernel, dim3((unsigned)P.nblk, G), dim3(WAIC_T), 0, st, A);
  if ((rc = loo_launch_tiles<LOO_SAMPLE>(who, Q, G, (unsigned)L.sparts, st)) != FMCMC_OK) return rc;
  hipLaunchKernelGGL(loo_thresh_kernel, wg_obs, dim3(LOO_T), 0, st, Q);
  if ((rc = loo_launch_tiles<LOO_COLLECT>(who, Q, G, (unsigned)P.nparts, st)) != FMCMC_OK) return rc;
  hipLaunchKernelGGL(loo_flag_kernel, per_obs, dim3(LOO_T), 0, st, Q);
  for (int pass = 0; pass < 8; pass++) {
    Q.pass = pass;
    if ((rc = loo_launch_tiles<LOO_HIST>(who, Q, G, (unsigned)P.nparts, st)) != FMCMC_OK) return rc;
    hipLaunchKernelGGL(loo_scan_kernel, per_obs, dim3(LOO_T), 0, st, Q);
  }
  Q.only = 1;
  if ((rc = loo_launch_tiles<LOO_COLLECT>(who, Q, G, (unsigned)P.nparts, st)) != FMCMC_OK) return rc;
  hipLaunchKernelGGL(loo_finish_kernel, wg_obs, dim3(LOO_T), lds, st, Q);
  hipLaunchKernelGGL(loo_total_kernel, dim3(G), dim3(LOO_T), 0, st, Q);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

inline fmcmc_model loo_plan_model(int64_t n) {
  fmcmc_model m;
  m.family = FMCMC_FAM_IID_NORMAL; m.p = 0; m.n = n; m.X = nullptr; m.y = nullptr; m.intercept = 1; m.guard = 0; m.prior_div = 0.0;
  return m;
}

}  // namespace

extern "C" {

int64_t fmcmc_loo_tail_len(int64_t S) { return S < 1 || S > (1LL << 40) ? 0 : loo_tail_len(S); }

int fmcmc_loo_plan(int64_t chains_per_group, int64_t N, int64_t n, int64_t out[FMCMC_LOO_PLAN_LEN]) {
  if (!out) return fail(FMCMC_ERR_ARG, "fmcmc_loo_plan: null argument");
  if (chains_per_group < 1 || N < 1 || n < 1 || N > (1LL << 40) / chains_per_group || chains_per_group * N < 2)
    return fail(FMCMC_ERR_ARG, "fmcmc_loo_plan: chains_per_group = %lld, N = %lld, n = %lld", (long long)chains_per_group,
                (long long)N, (long long)n);
  if (loo_tail_len(chains_per_group * N) > LOO_MAX_M)
    return fail(FMCMC_ERR_UNSUPPORTED, "fmcmc_loo_plan: %lld draws ask for a tail beyond %d", (long long)(chains_per_group * N),
                LOO_MAX_M);
  const fmcmc_model m = loo_plan_model(n);
  const WaicPlan W = waic_plan(&m, 1, chains_per_group, N);
  const LooPlan L = loo_plan(W, 1, chains_per_group, N, n);
  out[0] = L.M; out[1] = L.ustride; out[2] = L.nsu; out[3] = L.ns_rows; out[4] = L.rank; out[5] = L.target; out[6] = L.cap;
  out[7] = 2; out[8] = 5; out[9] = 8193;
  for (int i = 10; i < FMCMC_LOO_PLAN_LEN; i++) out[i] = 0;
  return FMCMC_OK;
}

int64_t fmcmc_loo_work_len(const fmcmc_model* m, int64_t ngroups, int64_t chains_per_group, int64_t N) {
  static const double nothing = 0.0;
  if (!m) return 0;
  if (loo_check("fmcmc_loo_work_len", m, (int64_t)m->p * m->n, m->n, &nothing, ngroups, chains_per_group, waic_family_k(m), N, 0,
                N) != FMCMC_OK)
    return 0;
  const WaicPlan W = waic_plan(m, ngroups, chains_per_group, N);
  return loo_plan(W, ngroups, chains_per_group, N, m->n).len;
}

int64_t fmcmc_loo_state_offset(const fmcmc_model* m, int64_t ngroups, int64_t chains_per_group, int64_t N) {
  if (fmcmc_loo_work_len(m, ngroups, chains_per_group, N) == 0) return -1;
  const WaicPlan W = waic_plan(m, ngroups, chains_per_group, N);
  return loo_plan(W, ngroups, chains_per_group, N, m->n).off_state;
}

int fmcmc_loo_groups_dev(const fmcmc_model* m0, int64_t x_stride, int64_t y_stride, const double* samples, int64_t ngroups,
                         int64_t chains_per_group, int32_t k, int64_t S, int64_t row0, int64_t N, const int32_t* active,
                         double* work, double* point, double* tail, double* total, void* hip_stream) {
  return loo_run("fmcmc_loo_groups_dev", m0, x_stride, y_stride, samples, ngroups, chains_per_group, k, S, row0, N, active, work,
                 point, tail, nullptr, total, hip_stream);
}

int fmcmc_loo_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                  double* work, double* point, double* tail, double* total, void* hip_stream) {
  return loo_run("fmcmc_loo_dev", m, 0, 0, samples, 1, nchains, k, S, row0, N, nullptr, work, point, tail, nullptr, total,
                 hip_stream);
}

}  // extern "C"
