// diag_ppc.hpp — posterior predictive checks from replicated data for the two regression families, from the kept rows where the
// sweep left them (the definition is INTEGRATION.md §2.2, the host restatement fmcmc_amd/summary.py: ppc_host, the kernel, its
// registers and scratch DESIGN.md §5.10).  Included by summary.hip behind diag_predictive.hpp; it reuses diag_predict.hpp's checks
// and its count of the bad draws (pred_check, pred_draw_kernel) and restates the tile evaluation with the roles of the operands
// exchanged, so that the object code of the other diagnostics is not touched.
//
// The S' x n matrix y_rep[s][i] is never stored:
//   pred_draw_kernel     (diag_predict.hpp) a thread a draw: the count of bad draws, a workgroup's sum into `work`.
//   ppc_tile_kernel<., PPC_FOLD>   a wavefront = one unit of 16 consecutive rows of one chain (waic_plan's unit; the last of a
//                        chain may be partial).  It loads its draws once as the A operand of v_mfma_f64_16x16x4 (registers up to
//                        64 operand columns, LDS beyond) and walks all ceil(n / 16) observation tiles with X as the B operand
//                        (ones for the intercept, zeros past n and past the columns).  D register r of lane l is draw 4 r + l / 16,
//                        observation l % 16: every element gets its Philox block, its variate and its y_rep (ppc_elem) and goes
//                        into the lane's fold of that draw.  The lanes l and l ^ 1 hold the observations i and i ^ 1 of the same
//                        four draws, which share a Philox block: each computes two of the four blocks and they exchange halves.
//                        The fold of a draw over i = 0 .. n - 1 is a function of n alone: lane c of the draw's row group takes
//                        i = c, c + 16, c + 32, ... in that order (sums shifted by the first value: K + sum(v - K) / cnt, M2 =
//                        sum (v - K)^2 - (sum(v - K))^2 / cnt, the chi-square terms added as they come, min and max by comparison);
//                        the 16 lanes are merged in lane order 0, 1, .. 15 (ppc_merge: Chan's update, plain sums, comparisons).
//                        The observations are not cut into chunks.  stats[c][q][r], q = mean, sd, min, max, chisq_rep, chisq_obs.
//   ppc_tile_kernel<., PPC_YREP>   the same text on tiles of 16 SELECTED draws, one observation tile a wavefront: writes y_rep itself.
//   ppc_count_kernel     a thread a draw: T_rep against T_obs per statistic, ballots and integer atomics into `work`.
//   ppc_total_kernel     one workgroup: the bad partials in index order and the counts, total[17].
// No floating-point atomics; a draw's six numbers depend on its own theta, its two ids, the model and the seed alone.
#pragma once

#include "../../include/fmh_philox.h"

namespace {

constexpr int PPC_T = 256;              // threads of every kernel here: four wavefronts, four units
constexpr int PPC_NSTAT = 6;            // mean, sd, min, max, chisq_rep, chisq_obs
constexpr int PPC_NCOUNT = 15;          // {gt, eq, non-finite} of mean, sd, min, max, chisq
constexpr int PPC_TOTAL = 2 + PPC_NCOUNT;
constexpr int PPC_MAX_SEL = 65535;      // selected draws of one fmcmc_ppc_yrep_dev call
constexpr int PPC_SEL_BATCH = 128;      // ... of one launch: they travel as a kernel argument
enum { PPC_FOLD = 0, PPC_YREP = 1 };

struct PpcSel { long long row[PPC_SEL_BATCH]; int chain[PPC_SEL_BATCH]; };
struct PpcTobs { double t[4]; };

struct PpcArgs {
  const double* samples; const double* X; const double* y; double* work; double* stats; double* yrep;
  long long S, row0, N, n, cpg, U, T, ntiles, nblk, chain_base, id0, id_step;
  unsigned long long seed;
  int k, gauss, ic, ncoef, nq, nsel;
};

// What one element (draw s, observation i) is, given its uniform u: the variate (Gaussian: z = qnorm(u), logistic: u itself),
// y_rep, and its two chi-square terms.  Host and device build this one text (fmcmc_ppc_elem_host).
struct PpcElem { double yrep, variate, crep, cobs; };

__host__ __device__ __forceinline__ PpcElem ppc_elem(int gauss, double u, double eta, double sigma, double rsigma, double y) {
  PpcElem e;
  if (gauss) {
    const double z = fmh_qnorm(u);
    e.variate = z;
    e.yrep = fmh_fma(sigma, z, eta);
    e.crep = z * z;
    const double r = (y - eta) * rsigma;
    e.cobs = r * r;
  } else {
    // pred_expit's branch form: fmh_exp(-|eta|) is fmh_exp(-eta) for eta >= 0 and fmh_exp(eta) below, fmh_exp(|eta|) the other
    const double a = fmh_abs(eta);
    const double en = fmh_exp(-a), ep = fmh_exp(a);
    const double p = eta >= 0.0 ? 1.0 / (1.0 + en) : en / (1.0 + en);
    const int v = u < p;
    e.variate = u;
    e.yrep = v ? 1.0 : 0.0;
    const double e_minus = eta >= 0.0 ? en : ep, e_plus = eta >= 0.0 ? ep : en;   // fmh_exp(-eta), fmh_exp(eta)
    e.crep = v ? e_minus : e_plus;
    e.cobs = y != 0.0 ? e_minus : e_plus;
  }
  return e;
}

// {count, mean, M2, min, max, chisq_rep, chisq_obs} of a set of observations of one draw; a, then b.  An empty side leaves the
// other as it is, bit for bit.  A NaN, once seen, stays the min and the max.
struct PpcAcc { double cnt, mean, M2, mn, mx, cr, co; };

__device__ __forceinline__ PpcAcc ppc_merge(const PpcAcc& a, const PpcAcc& b) {
  if (b.cnt == 0.0) return a;
  if (a.cnt == 0.0) return b;
  PpcAcc o;
  o.cnt = a.cnt + b.cnt;
  const double delta = b.mean - a.mean;
  o.mean = a.mean + delta * (b.cnt / o.cnt);
  o.M2 = (a.M2 + b.M2) + delta * delta * (a.cnt * b.cnt / o.cnt);
  o.mn = (b.mn < a.mn || b.mn != b.mn) ? b.mn : a.mn;
  o.mx = (b.mx > a.mx || b.mx != b.mx) ? b.mx : a.mx;
  o.cr = a.cr + b.cr;
  o.co = a.co + b.co;
  return o;
}

// NQR: the steps of four operand columns whose A values a lane keeps in registers; 0: the A tile lives in LDS.
template <int NQR, int MODE>
__global__ __launch_bounds__(PPC_T) void ppc_tile_kernel(PpcArgs A, PpcSel sel) {
  constexpr bool LDSA = NQR == 0;
  constexpr int NA = NQR ? NQR : 1;
  extern __shared__ double s_a[];                    // LDSA: [nq][4 wavefronts][64 lanes], a lane reads what it wrote
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, col = lane & 15;
  const int nq = A.nq, ncoef = A.ncoef;

  if (MODE == PPC_FOLD && blockIdx.x == 0 && tid < PPC_NCOUNT + 1)   // the counts of ppc_count_kernel, which runs behind this one
    reinterpret_cast<unsigned long long*>(A.work + 2 * A.nblk)[tid] = 0ull;

  // my 16 draws: draw d of the tile is row rb + d of chain c (FOLD) or selection base + d (YREP); `th` is draw `col`
  long long c = 0, rb = 0, t0, t1, base = 0;
  int valid;
  const double* __restrict__ th = A.samples;
  unsigned int id[4], ch[4];
  if (MODE == PPC_FOLD) {
    const long long u = (long long)blockIdx.x * (PPC_T / 64) + wave;
    if (u >= A.U) return;                            // (no barrier below: a wavefront works alone)
    c = u / A.T;
    rb = 16 * (u - c * A.T);
    valid = A.N - rb < 16 ? (int)(A.N - rb) : 16;
    th = A.samples + c * A.k * A.S + A.row0 + rb + (col < valid ? col : 0);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      id[r] = (unsigned int)(A.id0 + A.id_step * (rb + 4 * r + kk));
      ch[r] = (unsigned int)(A.chain_base + c);
    }
    t0 = 0; t1 = A.ntiles;
  } else {
    base = 16LL * blockIdx.y;
    valid = A.nsel - base < 16 ? (int)(A.nsel - base) : 16;
    const int mine = (int)base + (col < valid ? col : 0);
    th = A.samples + (long long)sel.chain[mine] * A.k * A.S + sel.row[mine];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int j = (int)base + (4 * r + kk < valid ? 4 * r + kk : 0);
      id[r] = (unsigned int)(A.id0 + A.id_step * sel.row[j]);
      ch[r] = (unsigned int)(A.chain_base + sel.chain[j]);
    }
    t0 = (long long)blockIdx.x * (PPC_T / 64) + wave;
    t1 = t0 + 1 < A.ntiles ? t0 + 1 : A.ntiles;
  }
  const bool aok = col < valid;

  // the A operand of lane l, step q: draw l % 16 of the tile, column 4 q + l / 16
  auto aval = [&](int q) -> double {
    const int j = 4 * q + kk;
    return (j < ncoef && aok) ? th[(long long)j * A.S] : 0.0;
  };
  double a[NA];
  if (LDSA) {
    for (int q = 0; q < nq; q++) s_a[(q * 4 + wave) * 64 + lane] = aval(q);
  } else {
#pragma unroll
    for (int q = 0; q < NA; q++) a[q] = q < nq ? aval(q) : 0.0;
  }
  // sigma of the draws 4 r + kk of my D registers: lane d (< 16) holds draw d
  const double sig_mine = (A.gauss && aok) ? th[(long long)(A.k - 1) * A.S] : 1.0;
  double sigma[4], rsigma[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    sigma[r] = __shfl(sig_mine, 4 * r + kk, 64);
    rsigma[r] = 1.0 / sigma[r];
  }

  const int odd = col & 1;                            // I compute the blocks of the draws r = 2 odd, 2 odd + 1; my partner the others
  const unsigned int ida = odd ? id[2] : id[0], idb = odd ? id[3] : id[1];
  const unsigned int cha = odd ? ch[2] : ch[0], chb = odd ? ch[3] : ch[1];
  const unsigned int k0 = (unsigned int)A.seed, k1 = (unsigned int)(A.seed >> 32);

  double K[4], sd[4], sdd[4], mn[4], mx[4], cr[4], co[4];
#pragma unroll
  for (int r = 0; r < 4; r++) { K[r] = 0.0; sd[r] = 0.0; sdd[r] = 0.0; mn[r] = 0.0; mx[r] = 0.0; cr[r] = 0.0; co[r] = 0.0; }
  int cnt = 0;

  for (long long tt = t0; tt < t1; tt++) {
    const long long obs = tt * 16 + col;
    const bool ok = obs < A.n;
    // the B operand of lane l, step q: row 4 q + l / 16 (a coefficient's covariate, ones for the intercept), column = the
    // observation l % 16 of the tile; zeros beyond n and beyond the columns
    waic_d4 acc = {0.0, 0.0, 0.0, 0.0};
    if (LDSA) {
      for (int q = 0; q < nq; q++) {
        const int j = 4 * q + kk;
        const double b = (!ok || j >= ncoef) ? 0.0 : ((A.ic && j == 0) ? 1.0 : A.X[(long long)(j - A.ic) * A.n + obs]);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s_a[(q * 4 + wave) * 64 + lane], b, acc, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < NA; q++) {
        if (q < nq) {
          const int j = 4 * q + kk;
          const double b = (!ok || j >= ncoef) ? 0.0 : ((A.ic && j == 0) ? 1.0 : A.X[(long long)(j - A.ic) * A.n + obs]);
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b, acc, 0, 0, 0);
        }
      }
    }
    const double yv = (MODE == PPC_FOLD && ok) ? A.y[obs] : 0.0;

    // the Philox block (id, chain, i >> 1, FMH_STREAM_PPC) of the pair (i, i ^ 1): lane i & 1 of fmh_uniform2
    const unsigned int blk = (unsigned int)(obs >> 1);
    const fmh_u32x4 pa = fmh_philox4x32_10(ida, cha, blk, FMH_STREAM_PPC, k0, k1);
    const fmh_u32x4 pb = fmh_philox4x32_10(idb, chb, blk, FMH_STREAM_PPC, k0, k1);
    const unsigned int keep_a_hi = odd ? pa.v[2] : pa.v[0], keep_a_lo = odd ? pa.v[3] : pa.v[1];
    const unsigned int keep_b_hi = odd ? pb.v[2] : pb.v[0], keep_b_lo = odd ? pb.v[3] : pb.v[1];
    const unsigned int got_a_hi = __shfl_xor(odd ? pa.v[0] : pa.v[2], 1, 64), got_a_lo = __shfl_xor(odd ? pa.v[1] : pa.v[3], 1, 64);
    const unsigned int got_b_hi = __shfl_xor(odd ? pb.v[0] : pb.v[2], 1, 64), got_b_lo = __shfl_xor(odd ? pb.v[1] : pb.v[3], 1, 64);
    const double u_keep_a = fmh_u01(keep_a_hi, keep_a_lo), u_keep_b = fmh_u01(keep_b_hi, keep_b_lo);
    const double u_got_a = fmh_u01(got_a_hi, got_a_lo), u_got_b = fmh_u01(got_b_hi, got_b_lo);
    double u[4];
    u[0] = odd ? u_got_a : u_keep_a; u[1] = odd ? u_got_b : u_keep_b;
    u[2] = odd ? u_keep_a : u_got_a; u[3] = odd ? u_keep_b : u_got_b;

    if (!ok) continue;
    // D register r of lane l is draw 4 r + l / 16, observation l % 16
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const PpcElem e = ppc_elem(A.gauss, u[r], acc[r], sigma[r], rsigma[r], yv);
      if (MODE == PPC_YREP) {
        if (4 * r + kk < valid) A.yrep[(base + 4 * r + kk) * A.n + obs] = e.yrep;
      } else {
        const double v = e.yrep;
        if (cnt == 0) { K[r] = v; mn[r] = v; mx[r] = v; }
        const double d = v - K[r];
        sd[r] += d;
        sdd[r] += d * d;
        mn[r] = (v < mn[r] || v != v) ? v : mn[r];
        mx[r] = (v > mx[r] || v != v) ? v : mx[r];
        cr[r] += e.crep;
        co[r] += e.cobs;
      }
    }
    cnt++;
  }
  if (MODE == PPC_YREP) return;

  const double fn = (double)A.n;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    PpcAcc mine;
    mine.cnt = (double)cnt;
    mine.mean = cnt ? K[r] + sd[r] / (double)cnt : 0.0;
    mine.M2 = cnt ? sdd[r] - sd[r] * sd[r] / (double)cnt : 0.0;
    if (mine.M2 < 0.0) mine.M2 = 0.0;                // (a rounding of the difference; a NaN stays)
    mine.mn = mn[r]; mine.mx = mx[r]; mine.cr = cr[r]; mine.co = co[r];
    PpcAcc all;
    for (int s = 0; s < 16; s++) {                   // the 16 lanes of my row group, in lane order
      const int src = 16 * kk + s;
      PpcAcc o;
      o.cnt = __shfl(mine.cnt, src, 64); o.mean = __shfl(mine.mean, src, 64); o.M2 = __shfl(mine.M2, src, 64);
      o.mn = __shfl(mine.mn, src, 64); o.mx = __shfl(mine.mx, src, 64);
      o.cr = __shfl(mine.cr, src, 64); o.co = __shfl(mine.co, src, 64);
      all = s == 0 ? o : ppc_merge(all, o);
    }
    if (col == 0 && 4 * r + kk < valid) {
      double* o = A.stats + c * PPC_NSTAT * A.N + rb + 4 * r + kk;
      o[0] = all.mean;
      o[A.N] = fmh_sqrt(all.M2 / (fn - 1.0));        // (n = 1: 0 / 0)
      o[2 * A.N] = all.mn;
      o[3 * A.N] = all.mx;
      o[4 * A.N] = all.cr;
      o[5 * A.N] = all.co;
    }
  }
}

// A thread a draw: per statistic one of {T_rep > T_obs, T_rep == T_obs, either side not finite, neither}; a wavefront's ballots
// go to the 15 integer counts behind the bad partials in `work`.
__global__ __launch_bounds__(PPC_T) void ppc_count_kernel(PpcArgs A, PpcTobs tobs) {
  const long long e = (long long)blockIdx.x * PPC_T + threadIdx.x;
  const bool in = e < A.cpg * A.N;
  const long long c = in ? e / A.N : 0, row = in ? e % A.N : 0;
  const double* __restrict__ s = A.stats + c * PPC_NSTAT * A.N + row;
  unsigned long long* __restrict__ counts = reinterpret_cast<unsigned long long*>(A.work + 2 * A.nblk);
  for (int j = 0; j < 5; j++) {
    const double rep = s[(long long)j * A.N], obs = j < 4 ? tobs.t[j] : s[5 * A.N];
    const bool nf = !fmh_isfinite(rep) || !fmh_isfinite(obs);
    const bool cls[3] = {in && !nf && rep > obs, in && !nf && rep == obs, in && nf};
    for (int w = 0; w < 3; w++) {
      const unsigned long long votes = __ballot(cls[w]);
      if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&counts[3 * j + w], (unsigned long long)__popcll(votes));
    }
  }
}

__global__ __launch_bounds__(PPC_T) void ppc_total_kernel(PpcArgs A, double* __restrict__ total) {
  __shared__ double red[PPC_T / 64];
  double bad = 0.0;
  for (long long i = threadIdx.x; i < A.nblk; i += PPC_T) bad += A.work[i];
  bad = block_sum<PPC_T / 64>(bad, red);
  const unsigned long long* __restrict__ counts = reinterpret_cast<const unsigned long long*>(A.work + 2 * A.nblk);
  if (threadIdx.x == 0) { total[0] = (double)(A.cpg * A.N); total[1] = bad; }
  if (threadIdx.x < PPC_NCOUNT) total[2 + threadIdx.x] = (double)counts[threadIdx.x];
}

// The checks of the keys: every id and chain id of the call must fit 32 bits (they are Philox counter words).
inline int ppc_check_ids(const char* who, int64_t nchains, int64_t chain_base, int64_t id0, int64_t id_step, int64_t last_row) {
  if (chain_base < 0 || id0 < 0 || id_step < 1)
    return fail(FMCMC_ERR_ARG, "%s: chain_base = %lld, id0 = %lld, id_step = %lld: needed are chain_base >= 0, id0 >= 0, id_step >= 1",
                who, (long long)chain_base, (long long)id0, (long long)id_step);
  if (chain_base > 0xffffffffLL - (nchains - 1))
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: the chain ids %lld .. %lld do not fit 32 bits", who, (long long)chain_base,
                (long long)(chain_base + nchains - 1));
  if (id0 > 0xffffffffLL || id_step > 0xffffffffLL || id_step * last_row > 0xffffffffLL - id0)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: the iteration labels %lld + %lld r, r <= %lld, do not fit 32 bits", who, (long long)id0,
                (long long)id_step, (long long)last_row);
  return FMCMC_OK;
}

inline PpcArgs ppc_args(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                        uint64_t seed, int64_t chain_base, int64_t id0, int64_t id_step) {
  PpcArgs A;
  A.samples = samples; A.X = m->X; A.y = m->y; A.work = nullptr; A.stats = nullptr; A.yrep = nullptr;
  A.S = S; A.row0 = row0; A.N = N; A.n = m->n; A.cpg = nchains;
  A.T = (N + 15) / 16; A.U = nchains * A.T; A.ntiles = (m->n + 15) / 16; A.nblk = (nchains * N + PRED_T - 1) / PRED_T;
  A.chain_base = chain_base; A.id0 = id0; A.id_step = id_step; A.seed = seed;
  A.k = k; A.gauss = m->family == FMCMC_FAM_GAUSSIAN_LINREG; A.ic = m->intercept ? 1 : 0; A.ncoef = A.ic + m->p;
  A.nq = (A.ncoef + 3) / 4; A.nsel = 0;
  return A;
}

template <int MODE>
int ppc_launch_tiles(const char* who, const PpcArgs& A, const PpcSel& sel, dim3 grid, hipStream_t st) {
  if (A.nq <= 2) {                                   // (k' <= 8: the headline regression)
    hipLaunchKernelGGL((ppc_tile_kernel<2, MODE>), grid, dim3(PPC_T), 0, st, A, sel);
  } else if (A.nq <= 4) {
    hipLaunchKernelGGL((ppc_tile_kernel<4, MODE>), grid, dim3(PPC_T), 0, st, A, sel);
  } else if (A.nq <= WAIC_REG_Q) {
    hipLaunchKernelGGL((ppc_tile_kernel<WAIC_REG_Q, MODE>), grid, dim3(PPC_T), 0, st, A, sel);
  } else {
    const size_t lds = (size_t)A.nq * PPC_T * sizeof(double);
    const int rc = allow_lds(who, ppc_tile_kernel<0, MODE>, lds);
    if (rc != FMCMC_OK) return rc;
    hipLaunchKernelGGL((ppc_tile_kernel<0, MODE>), grid, dim3(PPC_T), lds, st, A, sel);
  }
  return FMCMC_OK;
}

}  // namespace

extern "C" {

int64_t fmcmc_ppc_work_len(const fmcmc_model* m, int64_t nchains, int64_t N) {
  if (!m) return 0;
  if (pred_check("fmcmc_ppc_work_len", m, nchains, pred_family_k(m), N, 0, N, PRED_LINPRED, nullptr, 0) != FMCMC_OK) return 0;
  return 2 * ((nchains * N + PRED_T - 1) / PRED_T) + PPC_NCOUNT + 1;
}

int fmcmc_ppc_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, int64_t row0, int64_t N,
                  uint64_t seed, int64_t chain_base, int64_t id0, int64_t id_step, const double* tobs, double* work, double* stats,
                  double* total, void* hip_stream) {
  const char* who = "fmcmc_ppc_dev";
  if (!m || !samples || !tobs || !work || !stats || !total) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = pred_check(who, m, nchains, k, S, row0, N, PRED_LINPRED, nullptr, 0);
  if (rc != FMCMC_OK) return rc;
  if (!m->y) return fail(FMCMC_ERR_ARG, "%s: the model needs its observations y", who);
  if ((rc = ppc_check_ids(who, nchains, chain_base, id0, id_step, N - 1)) != FMCMC_OK) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  PpcArgs A = ppc_args(m, samples, nchains, k, S, row0, N, seed, chain_base, id0, id_step);
  A.work = work; A.stats = stats;
  PredArgs D = {};                                   // pred_draw_kernel reads these alone
  D.samples = samples; D.work = work; D.S = S; D.row0 = row0; D.N = N; D.cpg = nchains; D.k = k;
  D.P.gauss = A.gauss; D.P.off_s2 = A.nblk;
  PpcTobs T;
  for (int j = 0; j < 4; j++) T.t[j] = tobs[j];
  PpcSel none = {};
  hipLaunchKernelGGL(pred_draw_kernel, dim3((unsigned)A.nblk), dim3(PRED_T), 0, st, D);
  const dim3 grid((unsigned)((A.U + PPC_T / 64 - 1) / (PPC_T / 64)));
  if ((rc = ppc_launch_tiles<PPC_FOLD>(who, A, none, grid, st)) != FMCMC_OK) return rc;
  hipLaunchKernelGGL(ppc_count_kernel, dim3((unsigned)A.nblk), dim3(PPC_T), 0, st, A, T);
  hipLaunchKernelGGL(ppc_total_kernel, dim3(1), dim3(PPC_T), 0, st, A, total);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

int fmcmc_ppc_yrep_dev(const fmcmc_model* m, const double* samples, int64_t nchains, int32_t k, int64_t S, uint64_t seed,
                       int64_t chain_base, int64_t id0, int64_t id_step, const int64_t* sel_chain, const int64_t* sel_row,
                       int64_t nsel, double* yrep, void* hip_stream) {
  const char* who = "fmcmc_ppc_yrep_dev";
  if (!m || !samples || !sel_chain || !sel_row || !yrep) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = pred_check(who, m, nchains, k, S, 0, S, PRED_LINPRED, nullptr, 0);
  if (rc != FMCMC_OK) return rc;
  if (nsel < 1) return fail(FMCMC_ERR_ARG, "%s: nsel = %lld: at least one draw is needed", who, (long long)nsel);
  if (nsel > PPC_MAX_SEL)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: nsel = %lld selected draws; at most %d a call", who, (long long)nsel, PPC_MAX_SEL);
  int64_t last = 0;
  for (int64_t i = 0; i < nsel; i++) {
    if (sel_chain[i] < 0 || sel_chain[i] >= nchains || sel_row[i] < 0 || sel_row[i] >= S)
      return fail(FMCMC_ERR_ARG, "%s: selection %lld (chain %lld, row %lld) is outside the %lld chains x %lld rows", who,
                  (long long)i, (long long)sel_chain[i], (long long)sel_row[i], (long long)nchains, (long long)S);
    if (sel_row[i] > last) last = sel_row[i];
  }
  if ((rc = ppc_check_ids(who, nchains, chain_base, id0, id_step, last)) != FMCMC_OK) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  PpcArgs A = ppc_args(m, samples, nchains, k, S, 0, S, seed, chain_base, id0, id_step);
  for (int64_t s0 = 0; s0 < nsel; s0 += PPC_SEL_BATCH) {
    const int nb = (int)(nsel - s0 < PPC_SEL_BATCH ? nsel - s0 : PPC_SEL_BATCH);
    PpcSel sel = {};
    for (int i = 0; i < nb; i++) { sel.chain[i] = (int)sel_chain[s0 + i]; sel.row[i] = sel_row[s0 + i]; }
    A.nsel = nb;
    A.yrep = yrep + s0 * A.n;
    const dim3 grid((unsigned)((A.ntiles + PPC_T / 64 - 1) / (PPC_T / 64)), (unsigned)((nb + 15) / 16));
    if ((rc = ppc_launch_tiles<PPC_YREP>(who, A, sel, grid, st)) != FMCMC_OK) return rc;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

int fmcmc_ppc_elem_host(int32_t family, uint64_t seed, int64_t chain_id, int64_t id, int64_t n, const double* eta, double sigma,
                        double* yrep, double* variate) {
  const char* who = "fmcmc_ppc_elem_host";
  if (family != FMCMC_FAM_GAUSSIAN_LINREG && family != FMCMC_FAM_LOGISTIC)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: family %d; gaussian_linreg or logistic", who, (int)family);
  if (n < 0 || n > 0x7fffffffLL || (n > 0 && (!eta || !yrep || !variate))) return fail(FMCMC_ERR_ARG, "%s: bad argument", who);
  if (chain_id < 0 || chain_id > 0xffffffffLL || id < 0 || id > 0xffffffffLL)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: chain id %lld, id %lld: they must fit 32 bits", who, (long long)chain_id, (long long)id);
  const int gauss = family == FMCMC_FAM_GAUSSIAN_LINREG;
  for (int64_t i = 0; i < n; i++) {
    double u0, u1;
    fmh_uniform2(seed, (uint32_t)id, (uint32_t)chain_id, (uint32_t)(i >> 1), FMH_STREAM_PPC, &u0, &u1);
    const PpcElem e = ppc_elem(gauss, (i & 1) ? u1 : u0, eta[i], sigma, 1.0 / sigma, 0.0);
    yrep[i] = e.yrep;
    variate[i] = e.variate;
  }
  return FMCMC_OK;
}

}  // extern "C"
