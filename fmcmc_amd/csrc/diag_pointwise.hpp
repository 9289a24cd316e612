// diag_pointwise.hpp — WAIC and PSIS-LOO of a user-defined model: the pointwise log-likelihood l[s][i] = log p(y_i | theta_s)
// comes from the caller's batched callback (fmcmc_pointwise_fn, include/fmcmc_amd.h) in blocks of rows, and every block is
// consumed by one read before the next one overwrites it (the contract is INTEGRATION.md §2.2, the kernels, the fold order and
// the times DESIGN.md §5.10).  Included by summary.hip behind diag_loo.hpp: the plan of parts (waic_plan), the merges
// (waic_merge, loo_lse_merge), the layout of the partials, the threshold, flag, scan, finish and total kernels are the
// families'; their object code is not touched.
//
// A block is a run of consecutive units (a unit: the tile of 16 rows of one chain, u = c T + t, the last tile of a chain
// shorter); its rows lie one behind the other in [B][n], n contiguous.
//   pw_gather_kernel      a workgroup a unit: its rows of `samples` ([C][k][S]) through LDS into the row-major [B][k] block the
//                         callback reads, and the unit's count of draws with a parameter that is not finite into `work`.
//   pw_waic_fold_kernel   a workgroup = 64 observations (a lane an observation, so a wavefront reads 512 contiguous bytes of a
//                         row) x one part of the plan; wavefront w takes the rows r = w, w + 4, w + 8, w + 12 of every unit, four
//                         loads in flight, and folds them in unit order into {count, M, E, K, sum d, sum d^2} (waic_tile_kernel's
//                         arithmetic).  A part that ends in the block: the four wavefronts are merged ((0 + 1) + 2) + 3
//                         (waic_merge, through LDS) and {M, E, mean, M2} goes to the partial of (part, observation); one that
//                         goes on: the six numbers of every (wavefront, observation) are carried in `work` to the next launch
//                         (two slots, taken in turn: a launch reads the slot its predecessor wrote while its own last part
//                         writes the other).  (Sixteen wavefronts, one per row, were measured 20 % slower: DESIGN.md §5.10.)
//   pw_loo_kernel<MODE>   the same walk with loo_tile_kernel's three uses of l: SAMPLE writes the keys of the subsample (a
//                         workgroup a subsample unit), COLLECT counts and appends the keys above the threshold (integer
//                         atomics), counts the ties, folds the leftovers and the running (max, sum exp) per wavefront (carried
//                         like WAIC's), HIST adds to the integer histograms of the fallback.
//   pw_flagged_kernel     the number of flagged observations, an integer, for the driver's one read-back.
// The draws of a wavefront's accumulator and their order are a function of (nchains, N, n) alone: of the plan's parts, the unit
// order and r mod 4.  The block size, the number of launches and the order in which atomics land change no floating sum: the
// same bits for every block_rows.  Counts are integers; there are no float atomics.
#pragma once

namespace {

constexpr int PW_T = 256;                    // threads of the gather and the count kernels
constexpr int PW_W = 4;                      // wavefronts of a fold workgroup: wavefront w takes the rows w, w + 4, w + 8, w + 12 of a unit
constexpr int PW_FT = 64 * PW_W;             // threads of the kernels that read a block: 4 wavefronts x 64 observations
constexpr int PW_ACC = 6;                    // carried doubles per (wavefront, observation)
constexpr int PW_ROWS = 16 / PW_W;           // rows of a unit a wavefront takes: their loads are issued before the first is used
constexpr long long PW_BLOCK_DOUBLES = 1LL << 25;   // block_rows = 0: a [B][n] block of about 256 MiB

struct PwPlan {
  long long ub, brows;                       // units and rows of the largest block
  long long off_carry, off_nflag, off_theta, off_ll;
};

struct PwBlock {
  const double* ll;                          // [rows][n]
  long long i0, i1, stride;                  // the block: units idx * stride, idx in [i0, i1)
  long long index, off_carry;                // its number within the sweep; the two carry slots, read (index - 1) & 1, written index & 1
};

// The rows of the units idx' * stride, idx' in [i0, idx): 16 each but for the last tile of a chain.
__host__ __device__ inline long long pw_rows_before(long long i0, long long idx, long long stride, long long T, long long N) {
  if (idx <= i0) return 0;
  long long shorts = 0;
  if (stride == 1) {
    shorts = idx / T - i0 / T;
  } else {
    const long long c0 = i0 * stride / T, c1 = (idx - 1) * stride / T;
    for (long long c = c0; c <= c1; c++) {
      const long long last = c * T + T - 1;
      if (last % stride == 0 && last / stride >= i0 && last / stride < idx) shorts++;
    }
  }
  return 16 * (idx - i0) - shorts * (16 * T - N);
}

// The units of a block: block_rows rounded up to whole units, or the library's choice; never more than there are.
// The library's choice: about PW_BLOCK_DOUBLES, and whole parts where a part fits (every workgroup of a launch then has the
// same work, and nothing is carried).
inline long long pw_block_units(long long n, long long U, long long upp, long long block_rows) {
  long long ub = block_rows > 0 ? (block_rows + 15) / 16 : PW_BLOCK_DOUBLES / (16 * n);
  if (ub >= U) return U;
  if (block_rows == 0 && ub >= upp) ub -= ub % upp;
  return ub < 1 ? 1 : ub;
}

// `work` of the two entries: the bad-draw count of every unit, the partials [parts][n][4], the carried accumulators
// [2][PW_W][PW_ACC][n], the flagged count, the block of draws [brows][FMCMC_MAX_K] and the block [brows][n]; W.len is its end
// (where loo_plan puts its own).
inline void pw_plan(long long n, long long cpg, long long N, long long block_rows, WaicPlan& W, PwPlan& F) {
  const fmcmc_model m = loo_plan_model(n);
  W = waic_plan(&m, 1, cpg, N);
  F.ub = pw_block_units(n, W.U, W.upp, block_rows);
  const long long ub = F.ub;
  F.brows = 16 * ub < cpg * N ? 16 * ub : cpg * N;
  W.nblk = W.U;
  W.off_w = 0;
  W.off_bad = 0;
  W.off_part = W.U;
  F.off_carry = W.off_part + W.nparts * n * 4;
  F.off_nflag = F.off_carry + 2 * PW_W * PW_ACC * n;
  F.off_theta = F.off_nflag + 1;
  F.off_ll = F.off_theta + F.brows * FMCMC_MAX_K;
  W.len = F.off_ll + F.brows * n;
}

__global__ __launch_bounds__(PW_T) void pw_gather_kernel(const double* __restrict__ samples, int k, long long S, long long row0,
                                                         long long N, long long T, PwBlock B, double* __restrict__ theta,
                                                         double* __restrict__ bad) {
  extern __shared__ double s_t[];              // [16][k + 1]
  __shared__ unsigned int s_bad;
  __shared__ long long s_row;
  const int tid = threadIdx.x;
  const long long idx = B.i0 + blockIdx.x, u = idx * B.stride, c = u / T, t = u - c * T;
  const int valid = N - 16 * t < 16 ? (int)(N - 16 * t) : 16;
  if (tid == 0) { s_bad = 0u; s_row = pw_rows_before(B.i0, idx, B.stride, T, N); }   // (one thread walks the chains of the block)
  __syncthreads();
  const long long row = s_row;
  const double* __restrict__ src = samples + c * k * S + row0 + 16 * t;
  unsigned int nf = 0u;
  for (int e = tid; e < 16 * k; e += PW_T) {   // 16 consecutive rows of a column: 128 contiguous bytes
    const int r = e & 15, j = e >> 4;
    if (r < valid) {
      const double v = src[(long long)j * S + r];
      s_t[r * (k + 1) + j] = v;
      if (!fmh_isfinite(v)) nf |= 1u << r;
    }
  }
  if (nf) atomicOr(&s_bad, nf);
  __syncthreads();
  double* __restrict__ dst = theta + row * k;
  for (int e = tid; e < valid * k; e += PW_T) dst[e] = s_t[(e / k) * (k + 1) + e % k];
  if (tid == 0) bad[u] = (double)__popc(s_bad);
}

// The fold of waic_tile_kernel for one l, with a -Inf that leaves (M, E) as they are.
__device__ __forceinline__ void pw_lse(double l, double& M, double& E) {
  if (l > M) { E = fmh_fma(E, fmh_exp(M - l), 1.0); M = l; }
  else if (l != -fmh_inf()) E += fmh_exp(l - M);
}

// A wavefront's walk over the units [ua, ub) of a block: a unit a step, its PW_ROWS loads issued before the first is used.
struct PwWalk {
  long long u, ub, t, row, T, N;
  __device__ __forceinline__ PwWalk(long long i0, long long ua, long long ub_, long long T_, long long N_)
      : u(ua), ub(ub_), t(ua % T_), row(pw_rows_before(i0, ua, 1, T_, N_)), T(T_), N(N_) {}
  // loads the rows wave + PW_W q of the next unit; has[q]: the unit has that row
  __device__ __forceinline__ void load(const double* __restrict__ src, long long n, int wave, bool mine, double* v, bool* has) {
    const int valid = N - 16 * t < 16 ? (int)(N - 16 * t) : 16;
#pragma unroll
    for (int q = 0; q < PW_ROWS; q++) {
      has[q] = mine && wave + PW_W * q < valid;
      v[q] = has[q] ? src[(row + wave + PW_W * q) * n] : 0.0;
    }
    row += valid;
    u++;
    if (++t == T) t = 0;
  }
};

__global__ __launch_bounds__(PW_FT) void pw_waic_fold_kernel(WaicArgs A, PwBlock B) {
  __shared__ double s_acc[PW_W - 1][5][64];
  const WaicPlan& P = A.P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long tile = blockIdx.x % P.tiles, part = B.i0 / P.upp + blockIdx.x / P.tiles;
  const long long obs = tile * 64 + lane;
  const bool ok = obs < A.n;
  const long long pa = part * P.upp, pe = pa + P.upp < P.U ? pa + P.upp : P.U;
  const long long ua = pa > B.i0 ? pa : B.i0, ub = pe < B.i1 ? pe : B.i1;
  const long long cw = (long long)wave * PW_ACC * A.n + (ok ? obs : 0), slot = (long long)PW_W * PW_ACC * A.n;
  const double* __restrict__ cin = A.work + B.off_carry + ((B.index + 1) & 1) * slot + cw;
  double* __restrict__ cout = A.work + B.off_carry + (B.index & 1) * slot + cw;
  double cnt = 0.0, M = -fmh_inf(), E = 0.0, K = 0.0, sd = 0.0, sdd = 0.0;
  if (ok && ua > pa) { cnt = cin[0]; M = cin[A.n]; E = cin[2 * A.n]; K = cin[3 * A.n]; sd = cin[4 * A.n]; sdd = cin[5 * A.n]; }
  const double* __restrict__ src = B.ll + (ok ? obs : 0);
  PwWalk walk(B.i0, ua, ub, P.T, A.N);
  while (walk.u < ub) {
    double v[PW_ROWS];
    bool has[PW_ROWS];
    walk.load(src, A.n, wave, ok, v, has);
#pragma unroll
    for (int q = 0; q < PW_ROWS; q++) {
      if (has[q]) {
        const double l = v[q];
        if (cnt == 0.0) K = l;
        cnt += 1.0;
        const double d = l - K;
        sd += d;
        sdd = fmh_fma(d, d, sdd);
        pw_lse(l, M, E);
      }
    }
  }
  if (ub < pe) {                                     // (the same for the whole workgroup)
    if (ok) { cout[0] = cnt; cout[A.n] = M; cout[2 * A.n] = E; cout[3 * A.n] = K; cout[4 * A.n] = sd; cout[5 * A.n] = sdd; }
    return;
  }
  WaicAcc mine;
  mine.cnt = cnt; mine.M = M; mine.E = E;
  mine.mean = cnt != 0.0 ? K + sd / cnt : 0.0;
  mine.M2 = cnt != 0.0 ? sdd - sd * sd / cnt : 0.0;
  if (mine.M2 < 0.0) mine.M2 = 0.0;                  // (a rounding of the difference; a NaN stays)
  if (wave) {
    double (*o)[64] = s_acc[wave - 1];
    o[0][lane] = mine.cnt; o[1][lane] = mine.M; o[2][lane] = mine.E; o[3][lane] = mine.mean; o[4][lane] = mine.M2;
  }
  __syncthreads();
  if (wave == 0 && ok) {
    WaicAcc acc = mine;
    for (int w = 0; w < PW_W - 1; w++) {             // the four wavefronts of an observation, ((0 + 1) + 2) + 3
      WaicAcc b;
      b.cnt = s_acc[w][0][lane]; b.M = s_acc[w][1][lane]; b.E = s_acc[w][2][lane]; b.mean = s_acc[w][3][lane];
      b.M2 = s_acc[w][4][lane];
      acc = waic_merge(acc, b);
    }
    double* o = A.work + P.off_part + (part * A.n + obs) * 4;
    o[0] = acc.M; o[1] = acc.E; o[2] = acc.mean; o[3] = acc.M2;
  }
}

template <int MODE>
__global__ __launch_bounds__(PW_FT) void pw_loo_kernel(LooArgs Q, PwBlock B) {
  __shared__ double s_acc[PW_W - 1][4][64];
  const WaicArgs& A = Q.W;
  const WaicPlan& P = A.P;
  const LooPlan& L = Q.L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long tile = blockIdx.x % P.tiles, which = blockIdx.x / P.tiles;
  const long long obs = tile * 64 + lane;
  const bool ok = obs < A.n;
  const long long go = ok ? obs : 0;
  unsigned long long* __restrict__ st = reinterpret_cast<unsigned long long*>(A.work + L.off_state) + go * LOO_STATE;
  bool mine = ok;
  unsigned long long tkey = 0ull, prefix = 0ull;
  if (MODE != LOO_SAMPLE) {
    if (MODE == LOO_HIST || Q.only) {
      mine = ok && st[LOO_ST_FLAG] != 0ull;
      if (!__syncthreads_or(mine ? 1 : 0)) return;
    }
    if (mine) { tkey = st[LOO_ST_T]; prefix = st[LOO_ST_PREFIX]; }
  }
  const double* __restrict__ src = B.ll + go;
  if (MODE == LOO_SAMPLE) {                          // a workgroup a subsample unit
    const long long idx = B.i0 + which, u = idx * B.stride, t = u % P.T;
    const int valid = A.N - 16 * t < 16 ? (int)(A.N - 16 * t) : 16;
    __shared__ long long s_row;
    if (threadIdx.x == 0) s_row = pw_rows_before(B.i0, idx, B.stride, P.T, A.N);   // (one thread walks the chains of the block)
    __syncthreads();
    const long long row = s_row;
    unsigned long long* __restrict__ sub = reinterpret_cast<unsigned long long*>(A.work + L.off_sub) + go * L.ns16 + idx * 16;
#pragma unroll
    for (int q = 0; q < PW_ROWS; q++) {
      const int r = wave + PW_W * q;
      if (mine) sub[r] = r < valid ? key_of(-src[(row + r) * A.n]) : 0ull;   // (0: below every key, a row that does not exist)
    }
    return;
  }
  const double tval = value_of(tkey);
  const long long part = B.i0 / P.upp + which;
  const long long pa = part * P.upp, pe = pa + P.upp < P.U ? pa + P.upp : P.U;
  const long long ua = pa > B.i0 ? pa : B.i0, ub = pe < B.i1 ? pe : B.i1;
  unsigned long long* __restrict__ buf = reinterpret_cast<unsigned long long*>(A.work + L.off_buf) + go * L.cap;
  unsigned int* __restrict__ hist = reinterpret_cast<unsigned int*>(A.work + L.off_hist) + go * 256;
  const long long cw = (long long)wave * PW_ACC * A.n + go, slot = (long long)PW_W * PW_ACC * A.n;
  const double* __restrict__ cin = A.work + B.off_carry + ((B.index + 1) & 1) * slot + cw;
  double* __restrict__ cout = A.work + B.off_carry + (B.index & 1) * slot + cw;
  double Mx = -fmh_inf(), E = 0.0, a1 = 0.0, a2 = 0.0;
  if (MODE == LOO_COLLECT && mine && ua > pa) { Mx = cin[0]; E = cin[A.n]; a1 = cin[2 * A.n]; a2 = cin[3 * A.n]; }
  unsigned long long neq = 0ull;
  PwWalk walk(B.i0, ua, ub, P.T, A.N);
  while (walk.u < ub) {
    double v[PW_ROWS];
    bool has[PW_ROWS];
    walk.load(src, A.n, wave, mine, v, has);
#pragma unroll
    for (int q = 0; q < PW_ROWS; q++) {
      if (!has[q]) continue;
      const double l = v[q], rv = -l;
      const unsigned long long key = key_of(rv);
      if (MODE == LOO_HIST) {
        if (radix_high(key, Q.pass) == prefix) atomicAdd(&hist[radix_digit(key, Q.pass)], 1u);
      } else {
        pw_lse(l, Mx, E);
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
  if (MODE != LOO_COLLECT) return;
  if (mine && neq) atomicAdd(&st[LOO_ST_EQ], neq);
  if (ub < pe) {                                     // (the same for the whole workgroup)
    if (mine) { cout[0] = Mx; cout[A.n] = E; cout[2 * A.n] = a1; cout[3 * A.n] = a2; }
    return;
  }
  if (wave) {
    double (*o)[64] = s_acc[wave - 1];
    o[0][lane] = Mx; o[1][lane] = E; o[2][lane] = a1; o[3][lane] = a2;
  }
  __syncthreads();
  if (wave == 0 && mine) {
    for (int w = 0; w < PW_W - 1; w++) {             // the four wavefronts of an observation, ((0 + 1) + 2) + 3
      loo_lse_merge(Mx, E, s_acc[w][0][lane], s_acc[w][1][lane]);
      a1 += s_acc[w][2][lane];
      a2 += s_acc[w][3][lane];
    }
    double* o = A.work + P.off_part + (part * A.n + obs) * 4;
    o[0] = Mx; o[1] = E; o[2] = a1; o[3] = a2;
  }
}

__global__ __launch_bounds__(PW_T) void pw_flagged_kernel(LooArgs Q, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_n;
  const WaicArgs& A = Q.W;
  const unsigned long long* __restrict__ st = reinterpret_cast<const unsigned long long*>(A.work + Q.L.off_state);
  if (threadIdx.x == 0) s_n = 0ull;
  __syncthreads();
  unsigned long long c = 0ull;
  for (long long i = threadIdx.x; i < A.n; i += PW_T) c += st[i * LOO_STATE + LOO_ST_FLAG] != 0ull ? 1ull : 0ull;
  if (c) atomicAdd(&s_n, c);
  __syncthreads();
  if (threadIdx.x == 0) *out = s_n;
}

// Every check of the four entries, before any device call.
inline int pw_check(const char* who, bool loo, int64_t n, int64_t cpg, int32_t k, int64_t S, int64_t row0, int64_t N,
                    int64_t block_rows) {
  if (n < 1 || n > 0x7fffffffLL) return fail(FMCMC_ERR_ARG, "%s: n = %lld observations; supported are 1 .. 2^31 - 1", who, (long long)n);
  if (k < 1 || k > FMCMC_MAX_K) return fail(FMCMC_ERR_ARG, "%s: k = %d parameters; supported are 1 .. %d", who, (int)k, FMCMC_MAX_K);
  if (cpg < 1 || cpg > 0x7fffffffLL) return fail(FMCMC_ERR_ARG, "%s: nchains = %lld: must be 1 .. 2^31 - 1", who, (long long)cpg);
  if (N < 1 || row0 < 0 || S < N || row0 > S - N)
    return fail(FMCMC_ERR_ARG, "%s: the window [%lld, %lld) is outside the %lld rows of a chain", who, (long long)row0,
                (long long)(row0 + N), (long long)S);
  if (N > (1LL << 40) / cpg) return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld chains x %lld rows exceed one call", who, (long long)cpg,
                                         (long long)N);
  if (cpg * N < 2) return fail(FMCMC_ERR_ARG, "%s: S = %lld draw: %s needs at least 2", who, (long long)(cpg * N), loo ? "LOO" : "WAIC");
  if (block_rows < 0 || block_rows > (1LL << 40))
    return fail(FMCMC_ERR_ARG, "%s: block_rows = %lld: must be 0 (the library's choice) or a number of rows up to 2^40", who,
                (long long)block_rows);
  if (loo && loo_tail_len(cpg * N) > LOO_MAX_M)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: %lld draws ask for a tail of %lld; supported are tails up to %d (S <= 29826161)", who,
                (long long)(cpg * N), loo_tail_len(cpg * N), LOO_MAX_M);
  const fmcmc_model pm = loo_plan_model(n);
  const WaicPlan PW = waic_plan(&pm, 1, cpg, N);
  const long long ub = pw_block_units(n, PW.U, PW.upp, block_rows);
  if (ub > 0x3fffffffLL || (n + 63) / 64 * ub > 0x7fffffffLL || 16 * ub > (1LL << 50) / n)
    return fail(FMCMC_ERR_UNSUPPORTED, "%s: a block of %lld rows x %lld observations exceeds one launch; pass a smaller block_rows",
                who, 16 * ub, (long long)n);
  return FMCMC_OK;
}

struct PwRun {
  const char* who;
  fmcmc_pointwise_fn fun;
  void* user;
  const double* samples;
  int k;
  long long S, row0, N, n;
  double* work;
  WaicPlan W;
  PwPlan F;
  hipStream_t st;
};

// One sweep of the callback over the units idx * stride, idx in [0, count), block after block: gather, callback, use(block).
template <typename Use>
int pw_sweep(const PwRun& R, const char* pass, long long count, long long stride, Use use) {
  const WaicPlan& W = R.W;
  double* theta = R.work + R.F.off_theta;
  double* ll = R.work + R.F.off_ll;
  const size_t lds = (size_t)16 * (R.k + 1) * sizeof(double);
  long long block = 0;
  for (long long i0 = 0; i0 < count; i0 += R.F.ub, block++) {
    PwBlock B;
    B.ll = ll; B.i0 = i0; B.i1 = i0 + R.F.ub < count ? i0 + R.F.ub : count; B.stride = stride; B.index = block;
    B.off_carry = R.F.off_carry;
    const long long rows = pw_rows_before(B.i0, B.i1, stride, W.T, R.N);
    hipLaunchKernelGGL(pw_gather_kernel, dim3((unsigned)(B.i1 - B.i0)), dim3(PW_T), lds, R.st, R.samples, R.k, R.S, R.row0, R.N, W.T,
                       B, theta, R.work + W.off_bad);
    const int code = R.fun(theta, rows, R.k, R.n, ll, (void*)R.st, R.user);
    if (code != 0)
      return fail(FMCMC_ERR_FUN, "%s: the pointwise callback returned %d in block %lld of the %s pass (%lld rows); the call was "
                  "abandoned", R.who, code, block, pass, rows);
    use(B);
  }
  return FMCMC_OK;
}

inline unsigned pw_part_grid(const WaicPlan& W, const PwBlock& B) {
  return (unsigned)(W.tiles * ((B.i1 - 1) / W.upp - B.i0 / W.upp + 1));
}

inline int pw_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(FMCMC_ERR_DEVICE, "%s: launch failed (%s)", who, hipGetErrorString(e));
  return FMCMC_OK;
}

int pw_waic_run(const char* who, fmcmc_pointwise_fn fun, void* user, int64_t n, const double* samples, int64_t nchains, int32_t k,
                int64_t S, int64_t row0, int64_t N, int64_t block_rows, double* work, double* point, double* total,
                void* hip_stream) {
  if (!fun || !samples || !work || !point || !total) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = pw_check(who, false, n, nchains, k, S, row0, N, block_rows);
  if (rc != FMCMC_OK) return rc;
  PwRun R;
  R.who = who; R.fun = fun; R.user = user; R.samples = samples; R.k = k; R.S = S; R.row0 = row0; R.N = N; R.n = n; R.work = work;
  R.st = (hipStream_t)hip_stream;
  pw_plan(n, nchains, N, block_rows, R.W, R.F);
  WaicArgs A;
  A.samples = samples; A.X = nullptr; A.y = nullptr; A.active = nullptr; A.work = work;
  A.x_stride = 0; A.y_stride = 0; A.S = S; A.row0 = row0; A.N = N; A.n = n; A.cpg = nchains; A.k = k;
  A.P = R.W;
  rc = pw_sweep(R, "fold", R.W.U, 1, [&](const PwBlock& B) {
    hipLaunchKernelGGL(pw_waic_fold_kernel, dim3(pw_part_grid(R.W, B)), dim3(PW_FT), 0, R.st, A, B);
  });
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(waic_merge_kernel, dim3((unsigned)((n + WAIC_T - 1) / WAIC_T), 1), dim3(WAIC_T), 0, R.st, A, point);
  hipLaunchKernelGGL(waic_total_kernel, dim3(1), dim3(WAIC_T), 0, R.st, A, point, total);
  return pw_launched(who);
}

int pw_loo_run(const char* who, fmcmc_pointwise_fn fun, void* user, int64_t n, const double* samples, int64_t nchains, int32_t k,
               int64_t S, int64_t row0, int64_t N, int64_t block_rows, double* work, double* point, double* tail, double* total,
               void* hip_stream) {
  if (!fun || !samples || !work || !point || !total) return fail(FMCMC_ERR_ARG, "%s: null argument", who);
  int rc = pw_check(who, true, n, nchains, k, S, row0, N, block_rows);
  if (rc != FMCMC_OK) return rc;
  PwRun R;
  R.who = who; R.fun = fun; R.user = user; R.samples = samples; R.k = k; R.S = S; R.row0 = row0; R.N = N; R.n = n; R.work = work;
  R.st = (hipStream_t)hip_stream;
  pw_plan(n, nchains, N, block_rows, R.W, R.F);
  LooArgs Q;
  WaicArgs& A = Q.W;
  A.samples = samples; A.X = nullptr; A.y = nullptr; A.active = nullptr; A.work = work;
  A.x_stride = 0; A.y_stride = 0; A.S = S; A.row0 = row0; A.N = N; A.n = n; A.cpg = nchains; A.k = k;
  A.P = R.W;
  Q.L = loo_plan(R.W, 1, nchains, N, n);
  Q.point = point; Q.tail = tail; Q.total = total;
  const double dS = (double)(nchains * N), tau = 1.0 - 1.0 / log10(dS);
  Q.tau = tau < 0.7 ? tau : 0.7;
  Q.pass = 0; Q.only = 0;
  const WaicPlan& P = R.W;
  const LooPlan& L = Q.L;
  const dim3 per_obs((unsigned)((n + LOO_T - 1) / LOO_T), 1), wg_obs((unsigned)n, 1);
  const size_t lds = (size_t)L.M * sizeof(double);
  if (lds > 65536 && (rc = allow_lds(who, loo_finish_kernel, lds)) != FMCMC_OK) return rc;
  rc = pw_sweep(R, "sample", L.nsu, L.ustride, [&](const PwBlock& B) {
    hipLaunchKernelGGL(pw_loo_kernel<LOO_SAMPLE>, dim3((unsigned)(P.tiles * (B.i1 - B.i0))), dim3(PW_FT), 0, R.st, Q, B);
  });
  if (rc != FMCMC_OK) return rc;
  hipLaunchKernelGGL(loo_thresh_kernel, wg_obs, dim3(LOO_T), 0, R.st, Q);
  auto collect = [&](const PwBlock& B) {
    hipLaunchKernelGGL(pw_loo_kernel<LOO_COLLECT>, dim3(pw_part_grid(P, B)), dim3(PW_FT), 0, R.st, Q, B);
  };
  if ((rc = pw_sweep(R, "collect", P.U, 1, collect)) != FMCMC_OK) return rc;
  hipLaunchKernelGGL(loo_flag_kernel, per_obs, dim3(LOO_T), 0, R.st, Q);
  unsigned long long* nflag_d = reinterpret_cast<unsigned long long*>(work + R.F.off_nflag);
  hipLaunchKernelGGL(pw_flagged_kernel, dim3(1), dim3(PW_T), 0, R.st, Q, nflag_d);
  if ((rc = pw_launched(who)) != FMCMC_OK) return rc;
  unsigned long long nflag = 0ull;                   // the one synchronisation: how many observations take the fallback
  if (hipMemcpyAsync(&nflag, nflag_d, sizeof(nflag), hipMemcpyDeviceToHost, R.st) != hipSuccess ||
      hipStreamSynchronize(R.st) != hipSuccess)
    return fail(FMCMC_ERR_DEVICE, "%s: reading the number of flagged observations failed (%s)", who,
                hipGetErrorString(hipGetLastError()));
  if (nflag) {
    static const char* const names[8] = {"histogram 0", "histogram 1", "histogram 2", "histogram 3",
                                         "histogram 4", "histogram 5", "histogram 6", "histogram 7"};
    for (int pass = 0; pass < 8; pass++) {
      Q.pass = pass;
      rc = pw_sweep(R, names[pass], P.U, 1, [&](const PwBlock& B) {
        hipLaunchKernelGGL(pw_loo_kernel<LOO_HIST>, dim3(pw_part_grid(P, B)), dim3(PW_FT), 0, R.st, Q, B);
      });
      if (rc != FMCMC_OK) return rc;
      hipLaunchKernelGGL(loo_scan_kernel, per_obs, dim3(LOO_T), 0, R.st, Q);
    }
    Q.only = 1;
    if ((rc = pw_sweep(R, "second collect", P.U, 1, collect)) != FMCMC_OK) return rc;
  }
  hipLaunchKernelGGL(loo_finish_kernel, wg_obs, dim3(LOO_T), lds, R.st, Q);
  hipLaunchKernelGGL(loo_total_kernel, dim3(1), dim3(LOO_T), 0, R.st, Q);
  return pw_launched(who);
}

inline int64_t pw_work_len(const char* who, bool loo, int64_t n, int64_t nchains, int64_t N, int64_t block_rows, int64_t* state) {
  if (pw_check(who, loo, n, nchains, 1, N, 0, N, block_rows) != FMCMC_OK) return 0;
  WaicPlan W;
  PwPlan F;
  pw_plan(n, nchains, N, block_rows, W, F);
  if (!loo) return W.len;
  const LooPlan L = loo_plan(W, 1, nchains, N, n);
  if (state) *state = L.off_state;
  return L.len;
}

}  // namespace

extern "C" {

int64_t fmcmc_pointwise_block_rows(int64_t n, int64_t nchains, int64_t N, int64_t block_rows) {
  if (pw_check("fmcmc_pointwise_block_rows", false, n, nchains, 1, N, 0, N, block_rows) != FMCMC_OK) return 0;
  WaicPlan W;
  PwPlan F;
  pw_plan(n, nchains, N, block_rows, W, F);
  return 16 * F.ub;
}

int64_t fmcmc_waic_fun_work_len(int64_t n, int64_t nchains, int64_t N, int64_t block_rows) {
  return pw_work_len("fmcmc_waic_fun_work_len", false, n, nchains, N, block_rows, nullptr);
}

int fmcmc_waic_fun_dev(fmcmc_pointwise_fn fun, void* user, int64_t n, const double* samples, int64_t nchains, int32_t k, int64_t S,
                       int64_t row0, int64_t N, int64_t block_rows, double* work, double* point, double* total, void* hip_stream) {
  return pw_waic_run("fmcmc_waic_fun_dev", fun, user, n, samples, nchains, k, S, row0, N, block_rows, work, point, total, hip_stream);
}

int64_t fmcmc_loo_fun_work_len(int64_t n, int64_t nchains, int64_t N, int64_t block_rows) {
  return pw_work_len("fmcmc_loo_fun_work_len", true, n, nchains, N, block_rows, nullptr);
}

int64_t fmcmc_loo_fun_state_offset(int64_t n, int64_t nchains, int64_t N, int64_t block_rows) {
  int64_t off = -1;
  return pw_work_len("fmcmc_loo_fun_state_offset", true, n, nchains, N, block_rows, &off) ? off : -1;
}

int fmcmc_loo_fun_dev(fmcmc_pointwise_fn fun, void* user, int64_t n, const double* samples, int64_t nchains, int32_t k, int64_t S,
                      int64_t row0, int64_t N, int64_t block_rows, double* work, double* point, double* tail, double* total,
                      void* hip_stream) {
  return pw_loo_run("fmcmc_loo_fun_dev", fun, user, n, samples, nchains, k, S, row0, N, block_rows, work, point, tail, total,
                    hip_stream);
}

}  // extern "C"
