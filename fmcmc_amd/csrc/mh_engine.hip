// mh_engine.hip — gfx950 (MI355X) many-chain Metropolis-Hastings engine: the C-ABI (include/fmcmc_amd.h), validation
// and launches (the kernel selection, plan_route, is in mh_route.hpp).  The sweep kernels are instantiated in the k_*.hip translation units (compiled in parallel,
// fmcmc_amd/build.py) and reached through the look-ups of mh_kernels.hpp; their source is in the headers:
//   mh_common.hpp  shared device helpers      mh_streamed.hpp  general kernel (all families / kernels / schemes)
//   mh_rng.hpp     RNG stream kernel          mh_mfma.hpp      fp64-MFMA kernel, owner waves (headline)
//   mh_spec.hpp    wave-specialised kernel (kernel_adapt / kernel_ram; the latency form for few chains)
//   mh_wide2.hpp   wide models: observation-sharded dataflow kernel (owner / evaluator waves, two chain groups)
//   mh_mfma_ad.hpp adaptive owners on the MFMA evaluation   mh_bigk.hpp  more than 64 parameters
//
// Replaces, for ALL chains of a call at once, the per-chain loop of the reference
//   R/mcmc.R:720-838 (loop, accept, burn-in/thin)  x  R/kernel_normal.R / R/kernel_adapt.R /
//   R/kernel_ram.R / R/recursive.R / R/kernel.R:450-493 (proposal kernels).
//
// Execution model (DESIGN.md has the full picture):
//   * one 512-thread workgroup (8 wavefronts) owns CW chains; its 512 threads ARE the 512
//     "canonical lanes" of the log-posterior reduction: observation i belongs to lane i mod 512,
//     each lane accumulates its observations in index order with fma, lanes are combined by an
//     xor-butterfly tree (levels 1..32 inside a wavefront, 64..256 across the 8 wavefronts).
//     The CPU oracle mirrors exactly this tree, so accept decisions are bit-identical.
//   * every data value loaded by a thread is applied to all CW chains of the workgroup
//     (register/L2 traffic amortised over chains);
//   * per-chain "scalar" work (proposal, adaptation, accept) is done by the chain's owner
//     wavefront, lanes = parameters (one lane per row of Sigma / S);
//   * RNG = Philox4x32-10 counter stream (include/fmh_philox.h) or host-fed variates.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (explicit fma only).
#define FMH_WITH_RNG_FILL
#include "mh_tu.hpp"
#include <vector>
// (host-side shape helpers of the kernel families -- LDS sizes, slot counts; their kernels are instantiated in the k_*.hip files)
#include "mh_streamed.hpp"
#include "mh_mfma.hpp"
#include "mh_spec.hpp"
#include "mh_lat.hpp"
#include "mh_wide2.hpp"
#include "mh_mfma_ad.hpp"
#include "mh_bigk.hpp"
#include "mh_route.hpp"   // (kernel selection: plan_route)
#include "mh_fun.hpp"     // (the callback path: FunArgs, its LDS size; mh_fun_step is instantiated in k_fun.hip)

namespace {

// diagnostic: evaluates include/fmh_detmath.h / fmh_philox.h on the device (tests compare bitwise
// with the host build of the same headers)
__global__ void detmath_kernel(int which, const double* x, double* out, long long n,
                               unsigned long long seed) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = x[i], r;
  switch (which) {
    case 0: r = fmh_log(v); break;
    case 1: r = fmh_exp(v); break;
    case 2: r = fmh_log1p(v); break;
    case 3: r = fmh_qnorm(v); break;
    case 4: r = fmh_log_accept_u(seed, (unsigned)(i & 0xffff), (unsigned)(i >> 16)); break;
    case 5: r = fmh_normal(seed, (unsigned)(i & 0xffff), (unsigned)(i >> 16), (unsigned)(i % 7)); break;
    case 6: r = fmh_student_t(seed, (unsigned)(i & 0xffff), (unsigned)(i >> 16), (unsigned)(i % 7), v); break;
    case 7: r = fmh_sqrt(v); break;
    case 8: r = 1.0 / v; break;
    case 9: r = fmh_logit_g(v); break;   // g(|v|), the per-observation term of the logistic family
    case 10: r = fmh_unif(seed, (unsigned)(i & 0xffff), (unsigned)(i >> 16), (unsigned)(i % 7)); break;
    case 12: r = fmh_tan_0_halfpi(v); break;
    default: r = fmh_nan();
  }
  out[i] = r;
}

// the observation slots beyond the operand registers of mh_sweep_mfma<.., EXT>, in operand order: for wave w, streamed slot e
// (observation slot ns_res + e), group q, lane l, lane-group value g: column 4 q + l / 16 of [x_1 .. x_p, y, 0 ..] for
// observation i = 64 w + cl_a(l % 16) + g + 512 (ns_res + e); 0 beyond n.  out[((((w next + e) ng + q) 64 + l) 4 + g]
__global__ void mfma_build_stream(const double* X, const double* y, long long n, int p, int ng, int ns_res, int next, double* out) {
  const long long total = (long long)NW * next * ng * 64 * 4;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(idx & 3), l = (int)((idx >> 2) & 63);
    long long r = idx >> 8;
    const int q = (int)(r % ng); r /= ng;
    const int e = (int)(r % next), w = (int)(r / next);
    const int f = 4 * q + (l >> 4), o16 = l & 15;
    const long long i = (long long)(64 * w + 16 * (o16 & 3) + 4 * (o16 >> 2) + g) + (long long)NT * (ns_res + e);
    double a = 0.0;
    if (i < n) {
      if (f < p) a = X[(long long)f * n + i];
      else if (f == p) a = y[i];
    }
    out[idx] = a;
  }
}

// Data-only sums of the canonical logistic form (include/fmh_detmath.h, fmh_logit_g; oracle: logit_hs): hs[0] = sum_i w_i when
// the model has an intercept, hs[ic + j] = sum_i w_i x_ij, w_i = +1/2 (y_i != 0) or -1/2 -- every product exact, the sums over
// the 512 canonical lanes in index order and their tree -- and behind them, for the range check of the fast loops, the largest
// |x| of every column (a NaN stays).  One workgroup, once per launch: n (p + 1) additions.
__global__ __launch_bounds__(NT) void logit_hs_kernel(const double* X, const double* y, long long n, int p, int ic, double* hs) {
  __shared__ double s_w[NW], s_m[NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int col = -ic; col < p; col++) {
    double acc = 0.0, mx = 0.0;
    for (long long i = tid; i < n; i += NT) {
      const double w = (y[i] != 0.0) ? 0.5 : -0.5;
      if (col < 0) { acc = acc + w; }
      else {
        const double x = X[(long long)col * n + i], ax = __builtin_fabs(x);
        acc = acc + w * x;
        mx = (ax > mx || ax != ax) ? ax : mx;
      }
    }
    const double v = wave_xor_sum(acc);
    for (int o = 32; o >= 1; o >>= 1) { const double t = __shfl_xor(mx, o, 64); mx = (t > mx || t != t) ? t : mx; }
    if (lane == 0) { s_w[wave] = v; s_m[wave] = mx; }
    __syncthreads();
    if (tid == 0) {
      hs[ic + col] = ((s_w[0] + s_w[1]) + (s_w[2] + s_w[3])) + ((s_w[4] + s_w[5]) + (s_w[6] + s_w[7]));
      if (col >= 0) {
        double m = s_m[0];
        for (int q = 1; q < NW; q++) m = (s_m[q] > m || s_m[q] != s_m[q]) ? s_m[q] : m;
        hs[ic + p + col] = m;
      }
    }
    __syncthreads();
  }
}
// per-workgroup slices for the observation-sharded logistic evaluation (mh_common.hpp, logit_shard): workgroup b owns the
// canonical lanes 2 b, 2 b + 1; xs[((b nslots + slot) 2 + q) p + j] = x_ij of observation i = 512 slot + 2 b + q (0 beyond n)
__global__ void logit_build_slices(const double* X, long long n, int p, int nslots, double* xs) {
  const int b = blockIdx.x;
  for (int idx = threadIdx.x; idx < nslots * 2 * p; idx += blockDim.x) {
    const int o = idx / p, j = idx - o * p;
    const long long i = (long long)NT * (o >> 1) + 2 * b + (o & 1);
    xs[(long long)b * nslots * 2 * p + idx] = (i < n) ? X[(long long)j * n + i] : 0.0;
  }
}

// the slices of the long-data form (mh_common.hpp, shard_long): per workgroup [p + 1][2 nslots], columns then y, observation
// o = 2 slot + q <-> i = 512 slot + 2 b + q (0 beyond n): thread t of the workgroup reads element o = t, t + 512, .. of every column
__global__ void long_build_slices(const double* X, const double* y, long long n, int p, int nslots, double* xs) {
  const int b = blockIdx.x, nobs = 2 * nslots;
  for (long long idx = threadIdx.x; idx < (long long)(p + 1) * nobs; idx += blockDim.x) {
    const int j = (int)(idx / nobs), o = (int)(idx - (long long)j * nobs);
    const long long i = (long long)NT * (o >> 1) + 2 * b + (o & 1);
    xs[(long long)b * (p + 1) * nobs + idx] = (i < n) ? (j < p ? X[(long long)j * n + i] : y[i]) : 0.0;
  }
}

// compact per-workgroup slices of X and y for the observation-sharded evaluation (mh_common.hpp, eval_sharded):
// xs[(b p + j) SH_MAXO + o], ys[b SH_MAXO + o] with o = slot * LPW + q <-> observation b LPW + q + 512 slot (0 beyond n)
__global__ void shard_build_slices(const double* X, const double* y, long long n, int p, int lpw, int nslots,
                                   double* xs, double* ys) {
  const int b = blockIdx.x;
  for (int idx = threadIdx.x; idx < (p + 1) * SH_MAXO; idx += blockDim.x) {
    const int j = idx / SH_MAXO, o = idx - j * SH_MAXO;
    const int sl = o / lpw, q = o - sl * lpw;
    const long long i = (long long)b * lpw + q + (long long)NT * sl;
    const bool valid = sl < nslots && i < n;
    if (j < p) xs[((long long)b * p + j) * SH_MAXO + o] = valid ? X[(long long)j * n + i] : 0.0;
    else ys[(long long)b * SH_MAXO + o] = valid ? y[i] : 0.0;
  }
}

// the same slices in fp64-MFMA operand layout (mh_common.hpp, shard_columns_mfma): per workgroup a block of
// shm_hdr(nmt) + nmt KB 64 doubles = validity bits | y in D layout | A tiles [mt][kb][lane]
// t10: the third M-tile in the layout of the two 4x4x4 MFMAs that compute its 8 live rows, per K-block 32 doubles [kk][i][r]
// = row 4 r + i of the tile (value t = 8 + r of lane group i), column 4 kb + kk; the other 32 doubles of the K-block stay 0
__global__ void shard_build_mfma(const double* X, const double* y, long long n, int p, int lpw, int nslots, int nmt, int t10,
                                 double* out, int blk_doubles) {
  const int b = blockIdx.x, KB = (p + 3) >> 2, H = 4 / lpw, spg = (nslots + H - 1) / H, HDR = shm_hdr(nmt);
  double* o = out + (long long)b * blk_doubles;
  auto obs_of = [&](int g, int t) -> long long {   // observation at D position (lane group g, value t), -1: none
    const int q = g / H, h = g % H;
    if (t >= spg) return -1;
    const int slot = spg * h + t;
    if (slot >= nslots) return -1;
    const long long i = (long long)b * lpw + q + (long long)NT * slot;
    return i < n ? i : -1;
  };
  for (int idx = threadIdx.x; idx < blk_doubles; idx += blockDim.x) {
    if (idx < 32) {
      unsigned w[2];
      for (int e = 0; e < 2; e++) {
        const int g = (2 * idx + e) >> 4;
        unsigned m = 0;
        for (int t = 0; t < SHM_T; t++) if (obs_of(g, t) >= 0) m |= 1u << t;
        w[e] = m;
      }
      ((unsigned*)o)[2 * idx] = w[0];
      ((unsigned*)o)[2 * idx + 1] = w[1];
    } else if (idx < HDR) {
      const int t = (idx - 32) >> 6, lane = (idx - 32) & 63;
      const long long i = obs_of(lane >> 4, t);
      o[idx] = i >= 0 ? y[i] : 0.0;
    } else {
      const int e = idx - HDR, lane = e & 63, kb = (e >> 6) % KB, mt = (e >> 6) / KB;
      if (t10 && mt == 2) {
        const int kk4 = lane >> 3, i4 = (lane >> 1) & 3, r4 = lane & 1, col4 = 4 * kb + kk4;
        const long long i = lane < 32 ? obs_of(i4, 8 + r4) : -1;
        o[idx] = (i >= 0 && col4 < p) ? X[(long long)col4 * n + i] : 0.0;
        continue;
      }
      const int row = lane & 15, kk = lane >> 4, col = 4 * kb + kk;
      const long long i = obs_of(row & 3, 4 * mt + (row >> 2));   // D register r of lane group g is row 4 r + g of the tile
      o[idx] = (i >= 0 && col < p && mt < nmt) ? X[(long long)col * n + i] : 0.0;
    }
  }
}

// the canonical stream of chains [chain_base, + nchains) x steps [step_base, + nsteps) into logu [C][rows], z [C][rows][kz]
static void fill_rng(const fmcmc_run* run, long long step_base, long long nchains, long long nsteps, int kz, double df, double* ws, hipStream_t s) {
  const size_t items = (size_t)nchains * (size_t)nsteps;
  hipLaunchKernelGGL(rng_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (unsigned long long)run->seed, step_base,
                     (long long)run->chain_base, nchains, nsteps, kz, df, ws, ws + items);
}

// the free parameters which(!fixed) of a kernel, 0-based, into which[0 .. kf) (the callback path, once per call)
__global__ void fun_which_kernel(const uint8_t* fixed, int k, int* which) {
  if (threadIdx.x != 0) return;
  int kf = 0;
  for (int j = 0; j < k; j++)
    if (!fixed[j]) which[kf++] = j;
}

// accept counts of a continuation window (step windows, launch_sweep) added to the call's
__global__ void add_counts_kernel(long long* total, const long long* part, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) total[i] += part[i];
}

}  // namespace

// ==============================================================================================
// C-ABI
// ==============================================================================================
extern "C" {

int fmcmc_abi_version(void) { return FMCMC_ABI_VERSION; }
const char* fmcmc_last_error(void) { return g_err; }
// (not part of the C-ABI: the other translation units of the library leave their texts in the same thread-local buffer)
__attribute__((visibility("hidden"))) void fmcmc_set_error_text_(const char* text) { set_err("%s", text); }
static thread_local const char* g_kernel = "";
const char* fmcmc_last_kernel(void) { return g_kernel; }

int fmcmc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int64_t fmcmc_kept_rows(int64_t nsteps, int64_t burnin, int64_t thin) {
  if (thin < 1 || burnin >= nsteps) return 0;
  return (nsteps - burnin) / thin;
}

static int count_free(const fmcmc_kernel* kn, const uint8_t* fixed_host) {
  int kf = 0;
  for (int j = 0; j < kn->k; j++)
    if (!fixed_host[j]) kf++;
  return kf;
}

// Argument checks with the reference's own messages (R/mcmc.R:501-520, R/kernel.R:9,129-132,
// R/kernel_normal.R:134-135). Pointers inside `kernel` must be HOST pointers here.
static bool is_simple_kind(int kind) {
  return kind == FMCMC_KERNEL_NORMAL || kind == FMCMC_KERNEL_NORMAL_REFLECTIVE || kind == FMCMC_KERNEL_UNIF ||
         kind == FMCMC_KERNEL_UNIF_REFLECTIVE || kind == FMCMC_KERNEL_NMIRROR || kind == FMCMC_KERNEL_UMIRROR;
}
static int variates_per_step(const fmcmc_kernel* kn, int kf) {  // single-parameter schemes draw one variate per step
  return (is_simple_kind(kn->kind) && kn->scheme != FMCMC_SCHEME_JOINT) ? 1 : kf;
}

// the run arguments and the parameter count (R/mcmc.R:501-520), the checks fmcmc_validate and fmcmc_validate_fun share first
static int validate_run(const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (run->nchains < 1) { set_err("`nchains` must be an integer greater than 1."); return FMCMC_ERR_ARG; }
  if (run->burnin >= run->nsteps) {
    set_err("-burnin- (%lld) cannot be >= than -nsteps- (%lld).", (long long)run->burnin, (long long)run->nsteps);
    return FMCMC_ERR_ARG;
  }
  if (run->thin >= run->nsteps) {
    set_err("-thin- (%lld) cannot be > than -nsteps- (%lld).", (long long)run->thin, (long long)run->nsteps);
    return FMCMC_ERR_ARG;
  }
  if (run->thin < 1) { set_err("-thin- should be >= 1."); return FMCMC_ERR_ARG; }
  if (kn->k < 1 || kn->k > FMCMC_MAX_K) {
    set_err("number of parameters k=%d outside [1, %d]", kn->k, FMCMC_MAX_K);
    return FMCMC_ERR_UNSUPPORTED;
  }
  return FMCMC_OK;
}

// the kernel's own arguments (R/kernel.R:9,129-132, R/kernel_normal.R:134-135, ...) and the fed stream, shared as well
static int validate_kernel(const fmcmc_kernel* kn, const fmcmc_run* run);

int fmcmc_validate(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (!m || !kn || !run) { set_err("null argument"); return FMCMC_ERR_ARG; }
  const int rr = validate_run(kn, run);
  if (rr != FMCMC_OK) return rr;
  if (kn->k > FMCMC_MAX_K_WAVE) {   // one workgroup per chain (mh_sweep_bigk): what it implements
    const bool simple_joint = (kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE || kn->kind == FMCMC_KERNEL_UNIF || kn->kind == FMCMC_KERNEL_UNIF_REFLECTIVE) &&
                              kn->scheme == FMCMC_SCHEME_JOINT;
    const bool adapt_plain = kn->kind == FMCMC_KERNEL_ADAPT && kn->bw == 0 && kn->freq <= 1;
    if (!(simple_joint || adapt_plain || kn->kind == FMCMC_KERNEL_RAM)) {
      set_err("k = %d > %d parameters: supported are kernel_normal(_reflective) / kernel_unif(_reflective) with scheme = 'joint', "
              "kernel_adapt(bw = 0, freq = 1) and kernel_ram", kn->k, FMCMC_MAX_K_WAVE);
      return FMCMC_ERR_UNSUPPORTED;
    }
  }
  int kexp = -1;
  switch (m->family) {
    case FMCMC_FAM_GAUSSIAN_LINREG: kexp = (m->intercept ? 1 : 0) + m->p + 1; break;
    case FMCMC_FAM_LOGISTIC: kexp = (m->intercept ? 1 : 0) + m->p; break;
    case FMCMC_FAM_IID_NORMAL: kexp = 2; break;
    default: set_err("unknown log-posterior family %d", m->family); return FMCMC_ERR_ARG;
  }
  if (kexp != kn->k) {
    set_err("Incorrect length of -initial-: the model has %d parameters, the kernel %d.", kexp, kn->k);
    return FMCMC_ERR_ARG;
  }
  if (m->n < 1) { set_err("the model needs at least one observation"); return FMCMC_ERR_ARG; }
  return validate_kernel(kn, run);
}

static int validate_kernel(const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (kn->kind < FMCMC_KERNEL_NORMAL || kn->kind > FMCMC_KERNEL_UMIRROR) {
    set_err("unknown kernel kind %d", kn->kind);
    return FMCMC_ERR_ARG;
  }
  const bool simple = is_simple_kind(kn->kind);
  if (kn->kind == FMCMC_KERNEL_RAM) {
    if (kn->ram_qfun < FMCMC_RAM_QFUN_T_K || kn->ram_qfun > FMCMC_RAM_QFUN_T_DF) {
      set_err("kernel_ram: unknown -qfun- family %d (0 = rt(k, k), 1 = rnorm(k), 2 = rt(k, df)).", kn->ram_qfun);
      return FMCMC_ERR_ARG;
    }
    if (kn->ram_qfun == FMCMC_RAM_QFUN_T_DF && !(kn->ram_df > 0.0 && kn->ram_df <= DBL_MAX)) {
      set_err("kernel_ram: -qfun- = rt(k, df) needs a finite df > 0.");
      return FMCMC_ERR_ARG;
    }
    if (!(kn->ram_eta_exp >= 0.0 && kn->ram_eta_exp <= DBL_MAX)) {
      set_err("kernel_ram: the exponent of -eta- must be finite and positive (0 selects the default 2/3).");
      return FMCMC_ERR_ARG;
    }
  }
  if (simple && (kn->scheme < FMCMC_SCHEME_JOINT || kn->scheme > FMCMC_SCHEME_EXPLICIT)) {
    set_err("-scheme- update must be either an integer sequence, 'joint', 'ordered', or 'random'.");
    return FMCMC_ERR_ARG;
  }
  if (kn->fixed && kn->lb && kn->ub) {
    int kf = count_free(kn, kn->fixed);
    if (kf == 0) {
      set_err("The number of parameters to update, i.e. not fixed, cannot be zero. "
              "Check the value -fixed- in the kernel initialization.");
      return FMCMC_ERR_ARG;
    }
    if (kn->kind != FMCMC_KERNEL_NORMAL && kn->kind != FMCMC_KERNEL_UNIF)
      for (int j = 0; j < kn->k; j++)
        if (!(kn->ub[j] > kn->lb[j])) { set_err("-ub- cannot be <= than -lb-."); return FMCMC_ERR_ARG; }
    if ((kn->kind == FMCMC_KERNEL_UNIF || kn->kind == FMCMC_KERNEL_UNIF_REFLECTIVE) && kn->scale)
      for (int j = 0; j < kn->k; j++)   // scale = max. - min. (R/kernel_unif.R:55-56, :123-124)
        if (!(kn->scale[j] > 0.0)) { set_err("-max.- cannot be <= than -min.-."); return FMCMC_ERR_ARG; }
    if (simple && kn->scheme == FMCMC_SCHEME_EXPLICIT) {  // R/kernel.R:72-90
      if (!kn->scheme_seq || kn->scheme_len != kf) {
        set_err("When setting the update scheme, it should have the same length as the number of variables that will "
                "not be fixed. Right now length(scheme) = %d while sum(!fixed) = %d.", kn->scheme_seq ? kn->scheme_len : 0, kf);
        return FMCMC_ERR_ARG;
      }
      for (int j = 0; j < kn->k; j++) {
        if (kn->fixed[j]) continue;
        bool found = false;
        for (int a = 0; a < kn->scheme_len; a++) found = found || (kn->scheme_seq[a] == j);
        if (!found) {
          set_err("One or more variables was not included in the ordering sequence. Only variables that are not fixed "
                  "can be included in this list.");
          return FMCMC_ERR_ARG;
        }
      }
    }
  }
  if (kn->kind == FMCMC_KERNEL_ADAPT && (kn->freq < 1 || kn->bw < 0)) {
    set_err("-freq- must be >= 1 and -bw- >= 0 (got freq=%d, bw=%d)", kn->freq, kn->bw);
    return FMCMC_ERR_ARG;
  }
  if (kn->kind == FMCMC_KERNEL_RAM && kn->freq < 1) { set_err("-freq- must be >= 1."); return FMCMC_ERR_ARG; }
  if (kn->kind == FMCMC_KERNEL_ADAPT && kn->bw > 0 && kn->bw > kn->warmup) {
    set_err("The `warmup` parameter must be greater than `bw`.");
    return FMCMC_ERR_ARG;
  }
  if (run->rng_mode == FMCMC_RNG_FED && (!run->fed_logu || !run->fed_z)) {
    set_err("rng_mode = FED needs fed_logu and fed_z");
    return FMCMC_ERR_ARG;
  }
  return FMCMC_OK;
}

// The same sweep for the chains [off, off + cnt) of a call: every per-chain array advanced, RNG ids continued.
static SweepArgs chain_window(const SweepArgs& A, long long off, long long cnt, int kf) {
  SweepArgs W = A;
  const long long k = A.k, S = A.ldS, ns = A.nsteps, words = (A.nsteps + 31) >> 5;
  W.nchains = cnt; W.chain_base = A.chain_base + off;
#define ADV(f, stride) if (W.f) W.f += off * (stride)
  ADV(scheme_cols, ns); ADV(mirror_mu, k); ADV(mirror_scale, k); ADV(obs_arate, k);
  ADV(hist, (long long)A.hist_rows * kf);
  ADV(fed_logu, ns); ADV(fed_z, ns * A.kz);
  ADV(win_sum, kf); ADV(theta0, k); ADV(f0, 1); ADV(abs_iter, 1); ADV(Sigma, (long long)kf * kf); ADV(mean_prev, kf); ADV(have_mean, 1); ADV(nerrors, 1);
  ADV(samples, k * S); ADV(logpost, S); ADV(draws, k * S); ADV(accept_count, 1); ADV(accept_bits, words);
  ADV(status, 1); ADV(status_step, 1); ADV(status_theta, k);
#undef ADV
  return W;
}

// stream-ordered scratch that is released on EVERY way out of launch_sweep
struct AsyncScratch {
  void* p = nullptr;
  hipStream_t s = nullptr;
  ~AsyncScratch() { if (p) (void)hipFreeAsync(p, s); }
};

// launch of a kernel handle (mh_kernels.hpp): every sweep kernel takes the launch's SweepArgs by value
static hipError_t launch_k(const void* kfn, long long grid, int block, size_t lds, hipStream_t stream, const SweepArgs& A) {
  if (!kfn) return hipErrorInvalidDeviceFunction;
  if (lds > 48 * 1024) {
    const hipError_t ea = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return ea;
  }
  void* kargs[] = {(void*)&A};
  return hipLaunchKernel(kfn, dim3((unsigned)grid), dim3((unsigned)block), kargs, lds, stream);
}

// Can `nb` workgroups of kernel `kfn` with `lds` bytes of LDS be co-resident, i.e. may it run as ONE cooperative launch?
// `what`: the A.debug & 256 diagnostic of a refusal (nullptr: none).  A refusal leaves no error behind.
static bool coop_fits(const void* kfn, size_t lds, long long nb, int ncu, int dev, int debug, const char* what) {
  int coop = 0, perCU = 0;
  (void)hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, dev);
  const hipError_t e = kfn ? hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipErrorInvalidDeviceFunction;
  if (e != hipSuccess || !coop || hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kfn, NT, lds) != hipSuccess || (long long)perCU * ncu < nb) {
    if (what && (debug & 256)) fprintf(stderr, "fmcmc_amd: %s not launched: err=%d coop=%d perCU=%d lds=%zu\n", what, (int)e, coop, perCU, lds);
    (void)hipGetLastError();
    return false;
  }
  return true;
}

// The chains of a call as consecutive cooperative launches of `nb` workgroups, `per` chains each (the observation-sharded forms:
// the slices and tables serve every launch; the grid barrier words `bar` are cleared in front of each).
enum CoopRun { COOP_OK, COOP_NOTHING_RAN, COOP_LATER_FAILED };
static CoopRun coop_chain_windows(const void* kfn, long long nb, size_t lds, const SweepArgs& A, long long nchains, long long per, int kf,
                                  unsigned* bar, size_t nbar, hipStream_t stream) {
  hipError_t e = hipSuccess;
  long long done = 0;
  for (; done < nchains && e == hipSuccess; done += per) {
    SweepArgs W = chain_window(A, done, (nchains - done < per) ? nchains - done : per, kf);
    (void)hipMemsetAsync(bar, 0, sizeof(double) * nbar, stream);
    void* kargs[] = {(void*)&W};
    e = hipLaunchCooperativeKernel(kfn, dim3((unsigned)nb), dim3(NT), kargs, (unsigned int)lds, stream);
  }
  if (e == hipSuccess) return COOP_OK;
  (void)hipGetLastError();
  if (done <= per) return COOP_NOTHING_RAN;     // the runtime refused the first cooperative launch
  // a LATER window failed: the chains of the earlier windows have run
  set_err("HIP launch of chain window %lld failed (%s): the state of the first %lld chains is already advanced, the results of this call are invalid",
          (long long)(done / per), hipGetErrorString(e), (long long)(done - per));
  return COOP_LATER_FAILED;
}

// kernel->fixed etc. are DEVICE pointers here; kf and bounds info come via `kf`/`ram_bounded`.
static int launch_sweep(const fmcmc_model* m_in, const fmcmc_kernel* kn_in, const fmcmc_run* run,
                        fmcmc_state* st, fmcmc_out* out, int kf, int ram_bounded, hipStream_t stream) {
  SweepArgs A;
  memset(&A, 0, sizeof(A));
  // iid Normal(mu, sigma) IS the Gaussian linear model with an intercept and no covariate -- the same canonical arithmetic in
  // every kernel and in the oracle (fmcmc_oracle.c: pp = 0, icc = 1) -- so it takes that model's fast paths instead of the
  // all-family kernel (tools/option_audit.py)
  fmcmc_model m_norm = *m_in;
  if (m_norm.family == FMCMC_FAM_IID_NORMAL) { m_norm.family = FMCMC_FAM_GAUSSIAN_LINREG; m_norm.p = 0; m_norm.intercept = 1; }
  const fmcmc_model* m = &m_norm;
  AsyncScratch hist_guard, ws_guard, shw_guard, wc_guard;
  // the uniform kernels ARE the normal kernels with mu = min., scale = max. - min. and U(0,1) variates
  fmcmc_kernel ke = *kn_in;
  if (ke.kind == FMCMC_KERNEL_UNIF) { ke.kind = FMCMC_KERNEL_NORMAL; A.variate = 1; }
  if (ke.kind == FMCMC_KERNEL_UNIF_REFLECTIVE) { ke.kind = FMCMC_KERNEL_NORMAL_REFLECTIVE; A.variate = 1; }
  if (ke.kind == FMCMC_KERNEL_UMIRROR) A.variate = 1;
  const bool mirror = (ke.kind == FMCMC_KERNEL_NMIRROR || ke.kind == FMCMC_KERNEL_UMIRROR);
  if (mirror && (!st->mirror_mu || !st->mirror_scale || !st->obs_arate || !st->abs_iter)) {
    set_err("mirror kernels need state->mirror_mu, mirror_scale, obs_arate and abs_iter");
    return FMCMC_ERR_ARG;
  }
  A.nadapt = kn_in->nadapt; A.mirror_mu = st->mirror_mu; A.mirror_scale = st->mirror_scale; A.obs_arate = st->obs_arate;
  const fmcmc_kernel* kn = &ke;
  if ((kn->kind <= FMCMC_KERNEL_NORMAL_REFLECTIVE || mirror) && kn->scheme == FMCMC_SCHEME_RANDOM && run->rng_mode == FMCMC_RNG_FED &&
      !st->scheme_cols) {
    set_err("rng_mode = FED with scheme = 'random' needs state->scheme_cols");
    return FMCMC_ERR_ARG;
  }
  A.bw = (kn->kind == FMCMC_KERNEL_ADAPT) ? kn->bw : 0; A.Sd = kn->Sd;
  const bool adapt_hist = (kn->kind == FMCMC_KERNEL_ADAPT && (kn->bw > 0 || kn->freq > 1));
  if (adapt_hist) {   // ring of the last rows of every chain (the reference reads them from env$ans)
    A.hist_rows = (kn->bw - 1 > kn->freq) ? kn->bw - 1 : kn->freq;
    hipError_t eh = hipMallocAsync((void**)&A.hist, sizeof(double) * (size_t)run->nchains * (size_t)A.hist_rows * (size_t)kf, stream);
    if (eh != hipSuccess) { set_err("hipMallocAsync(adapt history) failed: %s", hipGetErrorString(eh)); return FMCMC_ERR_DEVICE; }
    hist_guard.p = A.hist; hist_guard.s = stream;
  }
  A.freq = kn->freq < 1 ? 1 : kn->freq; A.scheme_seq = kn->scheme_seq; A.scheme_len = kn->scheme_len;
  A.constr = (kn->kind == FMCMC_KERNEL_RAM) ? kn->constr : nullptr; A.scheme_cols = st->scheme_cols;
  A.family = m->family; A.p = m->p; A.intercept = m->intercept ? 1 : 0; A.guard = m->guard ? 1 : 0;
  A.n = m->n; A.X = m->X; A.y = m->y; A.prior_div = m->prior_div;
  A.kind = kn->kind; A.k = kn->k; A.scheme = kn->scheme; A.warmup = kn->warmup;
  A.until = kn->until; A.eps = kn->eps; A.arate = kn->arate;
  // kernel_ram's qfun / eta families (R/kernel_ram.R:67-68): df of the t variates (0 = normal) and the exponent of eta
  A.ram_df = (kn->ram_qfun == FMCMC_RAM_QFUN_NORMAL) ? 0.0 : (kn->ram_qfun == FMCMC_RAM_QFUN_T_DF ? kn->ram_df : (double)kf);
  A.ram_neg_exp = (kn->ram_eta_exp != 0.0) ? -kn->ram_eta_exp : (-2.0 / 3.0);
  A.mu = kn->mu; A.scale = kn->scale; A.lb = kn->lb; A.ub = kn->ub; A.fixed = kn->fixed;
  A.nchains = run->nchains; A.nsteps = run->nsteps; A.burnin = run->burnin; A.thin = run->thin;
  A.S = fmcmc_kept_rows(run->nsteps, run->burnin, run->thin);
  A.ldS = out->ld_rows > 0 ? out->ld_rows : A.S;
  if (A.ldS < A.S) { set_err("fmcmc_out.ld_rows (%lld) is smaller than the %lld kept rows of this call", (long long)out->ld_rows, (long long)A.S); return FMCMC_ERR_ARG; }
  A.chain_base = run->chain_base; A.step_base = run->step_base; A.seed = run->seed;
  A.rng_mode = run->rng_mode; A.fresh = st->fresh; A.ram_bounded = ram_bounded;
  A.kz = variates_per_step(kn, kf);
  A.fed_logu = run->fed_logu; A.fed_z = run->fed_z;
  const Knobs K = read_knobs();
  A.debug = K.mode;   // timing ablations only
  A.theta0 = st->theta0; A.f0 = st->f0; A.abs_iter = (long long*)st->abs_iter; A.Sigma = st->Sigma;
  A.mean_prev = st->mean_prev; A.have_mean = st->have_mean; A.nerrors = st->nerrors;
  A.samples = out->samples; A.logpost = out->logpost; A.draws = out->draws;
  A.accept_count = (long long*)out->accept_count; A.accept_bits = out->accept_bits;
  A.status = out->status; A.status_step = (long long*)out->status_step; A.status_theta = out->status_theta;

  // logistic family: the data-only sums of the linear part and the columns' largest |x| (logit_hs_kernel), once per launch
  AsyncScratch hs_guard;
  if (m->family == FMCMC_FAM_LOGISTIC) {
    double* hs = nullptr;
    hipError_t eh = hipMallocAsync((void**)&hs, sizeof(double) * (size_t)(2 * MAXK + 2), stream);
    if (eh != hipSuccess) { set_err("hipMallocAsync(logistic sums) failed: %s", hipGetErrorString(eh)); return FMCMC_ERR_DEVICE; }
    hs_guard.p = hs; hs_guard.s = stream;
    hipLaunchKernelGGL(logit_hs_kernel, dim3(1), dim3(NT), 0, stream, m->X, m->y, (long long)m->n, m->p, m->intercept ? 1 : 0, hs);
    A.lg_hs = hs;
  }
  // ---- launch geometry
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  if (ncu <= 0) ncu = 256;
  {   // the code object is gfx950 only, and the hand-overs of the wide kernels rest on ITS cache behaviour (mh_common.hpp)
    static int arch_ok = -1;
    if (arch_ok < 0) {
      hipDeviceProp_t prop;
      arch_ok = (hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ? 1 : 0;
    }
    if (!arch_ok) { set_err("this library is built for gfx950 (MI355X); the current device is another architecture"); return FMCMC_ERR_DEVICE; }
  }
  Route R = plan_route(m, kn, run, kf, ram_bounded, A.kz, A.ldS, ncu, K);
  if (R.lds_exceeded) { set_err("LDS budget exceeded (k=%d)", kn->k); return FMCMC_ERR_UNSUPPORTED; }
  if (R.no_kernel) { set_err("no device kernel for the %s form (k=%d)", kernel_name(R), kn->k); return FMCMC_ERR_DEVICE; }
  hipError_t e = hipSuccess;
  if (R.form == Form::BIGK || R.form == Form::BIGK_HBM) {
    g_kernel = kernel_name(R);
    e = launch_k(R.kfn, run->nchains, NT, R.lds, stream, A);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { set_err("HIP launch failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
    return FMCMC_OK;
  }
  A.tb = R.tb;
  const double fill_df = (kn->kind == FMCMC_KERNEL_RAM) ? A.ram_df : (A.variate == 1 ? -1.0 : 0.0);   // (rng_fill_kernel: t / U(0,1) / normal)
  A.spec_opt = R.pipe_opt;
  A.spec_cw = R.spec_cw;
  A.nsteps_call = run->nsteps;
  // the long-data form first, where the plan has it: a refused cooperative launch leaves the planned form
  bool launched_long = false;
  if (R.kfn_long && coop_fits(R.kfn_long, R.lds_long, 256, ncu, dev, K.mode, nullptr)) {
    double* shw = nullptr;
    const int nobs = 2 * R.nslots;
    const size_t nxs = (size_t)256 * (m->p + 1) * nobs, nth = ((size_t)kn->k * (run->nchains + SH_PAD) + 7) & ~(size_t)7,
                 npt = (size_t)(NT + SH_PAD) * run->nchains, nbar = 32 * 20 / 2;
    hipError_t ea = hipMallocAsync((void**)&shw, sizeof(double) * (nxs + nth + npt + nbar), stream);
    if (ea != hipSuccess) { set_err("hipMallocAsync(sharded evaluation) failed: %s", hipGetErrorString(ea)); return FMCMC_ERR_DEVICE; }
    shw_guard.p = shw; shw_guard.s = stream;
    double* thw = shw; double* ptw = thw + nth; unsigned* bar = (unsigned*)(ptw + npt); double* xs = ptw + npt + nbar;
    hipLaunchKernelGGL(long_build_slices, dim3(256), dim3(256), 0, stream, m->X, m->y, (long long)m->n, m->p, R.nslots, xs);
    SweepArgs W = A;
    W.shard = 2; W.sh_nslots = R.nslots; W.sh_xs = xs; W.sh_ys = nullptr; W.sh_th = thw; W.sh_part = ptw; W.sh_bar = bar;
    W.sh_long = 1; W.sh_lcg = (int)R.lcg; W.sh_mblk = (int)(R.lcg * R.lrow);
    // (all chains in one launch: at most 64)
    if (coop_chain_windows(R.kfn_long, 256, R.lds_long, W, run->nchains, run->nchains, kf, bar, nbar, stream) == COOP_OK) {
      launched_long = true;
      R.form = Form::LONG;
    } else {                            // the runtime refused the cooperative launch: nothing ran, take the planned form
      (void)hipFreeAsync(shw, stream);   // (the forms below put their own block into shw_guard)
      shw_guard.p = nullptr;
    }
  }
  // the operand-order copy of the observation slots beyond the registers (EXT / adaptive MFMA forms): 4 ng doubles per streamed
  // observation -- for p = 1 several times the size of X.  When the device cannot give that memory the call still runs: on
  // the chain-sharded form beneath (for these shapes the resident or the general kernel), which needs none
  AsyncScratch mfs_guard;
  if (!launched_long && R.mfma_ng && R.mfma_ext) {
    const int next = R.nslots - R.mfma_ext;
    double* mfs = nullptr;
    const size_t nd = (size_t)NW * (next > 0 ? next : 1) * R.mfma_ng * 64 * 4;   // (everything resident: one slot of stand-in, read and never used)
    if (hipMallocAsync((void**)&mfs, sizeof(double) * nd, stream) != hipSuccess) {
      (void)hipGetLastError();
      R.form = R.base; R.kfn = R.kfn_base;
      R.mfma_ng = 0; R.mfma_ext = 0; R.mfma_ad = 0; R.pipe_opt = 0;
    } else {
      mfs_guard.p = mfs; mfs_guard.s = stream;
      if (next > 0) hipLaunchKernelGGL(mfma_build_stream, dim3(512), dim3(256), 0, stream, m->X, m->y, (long long)m->n, m->p, R.mfma_ng, R.mfma_ext, next, mfs);
      else (void)hipMemsetAsync(mfs, 0, sizeof(double) * nd, stream);
      A.mf_stream = mfs; A.mf_next = next > 0 ? next : 0;
    }
  }
  if (launched_long) {
  } else
  if (stream_fed(R.form)) {
    double* ws = nullptr;
    // Step windows: the normal / uniform kernels with the library's own stream.  Window 0 is an ordinary launch of the call's
    // first n0 steps; every later window is a launch of w + 1 steps whose step 1 re-evaluates the state the window starts
    // from (bit for bit the f0 it replaces) and whose steps 2 .. w + 1 are the call's next w steps (SweepArgs.win_cont).
    // The stream of a window (rows of w + 1 steps) is filled right in front of it into ONE reused buffer of <= ~256 MiB
    // (it was nchains x nsteps x (kz + 1) doubles, and the reason for the 4 GiB limit; measured at C2's shape, 1.2e5 steps:
    // windows of 320 / 1344 / 8192 steps 2.17 / 2.08 / 2.05 us per step -- a window costs ~40 us of launches, refill of the
    // 80 operand registers and one extra evaluation, so the buffer is as large as is reasonable, not cache-sized).  The Philox counter
    // is the ABSOLUTE step, so the variates, and with them every bit of the output, do not depend on the cut
    // (windows begin behind a step = 1 mod 32: the accept bitmap's words then line up).
    // Round 5: kernel_adapt / kernel_ram too (R/kernel_adapt.R:118-133, R/kernel_ram.R:129-152 are ONE loop of any length).  What
    // depends on the step -- `i > 2`, the mean of this call's rows before the first adaptation, eta(i, k), `i %% freq` -- reads
    // the call's step (SweepArgs.step_off + the window's), the running sum of the rows travels from window to window
    // (SweepArgs.win_sum), everything else (Sigma / S, the running mean, abs_iter) is the state the windows hand on anyway.
    const long long win = R.win ? R.win : run->nsteps;
    const long long n0 = (R.win && run->nsteps > win + 1) ? win + 1 : run->nsteps;   // steps of window 0
    if (A.rng_mode == FMCMC_RNG_PHILOX) {
      // materialise the canonical stream: [C][rows] log u, then [C][rows][kz] z; rows = a window's steps (or the whole call)
      const long long rows = (n0 < run->nsteps) ? win + 1 : run->nsteps;
      const size_t items = (size_t)run->nchains * (size_t)rows;
      e = hipMallocAsync((void**)&ws, sizeof(double) * items * (size_t)(A.kz + 1), stream);
      if (e != hipSuccess) { set_err("hipMallocAsync(rng stream) failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
      ws_guard.p = ws; ws_guard.s = stream;
    }
    auto fill_stream = [&](SweepArgs& W, long long step_base_eff) {   // the stream of launch W, rows = W.nsteps
      fill_rng(run, step_base_eff, W.nchains, W.nsteps, A.kz, fill_df, ws, stream);
      W.fed_logu = ws; W.fed_z = ws + (size_t)W.nchains * (size_t)W.nsteps; W.rng_mode = FMCMC_RNG_FED;
    };
    auto launch_fast = [&](const SweepArgs& W) {   // one launch of the call, or one step window of it
      const long long pblk = (W.nchains + 3) / 4, sblk = (W.nchains + R.spec_cw - 1) / R.spec_cw;
      // (MFMA forms: offsets from the buffer bases stay 32 bits -- the cheaper form, see mh_sweep_mfma's BIG -- while the samples of
      //  all chains and the stream of this launch stay below 4 GiB)
      const bool big = (unsigned long long)W.nchains * kn->k * (unsigned long long)W.ldS * 8ull >= (1ull << 32) ||
                       (unsigned long long)W.nchains * (unsigned long long)W.nsteps * (unsigned long long)W.kz * 8ull >= (1ull << 32);
      const int kv = (kn->kind == FMCMC_KERNEL_NORMAL) ? 1 : 2;
      switch (R.form) {
        case Form::MFMA_ADAPTIVE: e = launch_k(R.kfn, pblk, NT, mfma_ad_lds_bytes(R.mfma_ad == 2), stream, W); break;
        case Form::MFMA_STREAMED: e = launch_k(fmh::k_mfma_ext(kv, R.mfma_ng, R.mfma_ext, big ? 1 : 0), pblk, NT, mfma_lds_bytes(), stream, W); break;
        case Form::MFMA: e = launch_k(fmh::k_mfma(kv, R.mfma_ng, R.nslots, big ? 1 : 0), pblk, NT, mfma_lds_bytes(), stream, W); break;
        // the latency form (mh_lat.hpp): 1 .. 3 chains per workgroup
        case Form::LAT_LOGIT: e = launch_k(R.kfn, sblk, NT, fmh::k_lat_logit_lds(), stream, W); break;
        case Form::LAT: e = launch_k(R.kfn, sblk, NT, lat_lds_bytes(), stream, W); break;
        // the wave-specialised kernel (mh_spec.hpp): spec_cw chains per workgroup
        case Form::SPEC_LOGIT: e = launch_k(R.kfn, sblk, SPEC_NT, fmh::k_spec_logit_lds(kn->kind >= FMCMC_KERNEL_ADAPT ? 1 : 0), stream, W); break;
        default: e = launch_k(R.kfn, sblk, SPEC_NT, spec_lds_bytes(R.pipe_opt, kn->kind == FMCMC_KERNEL_ADAPT || kn->kind == FMCMC_KERNEL_RAM), stream, W); break;
      }
    };
    SweepArgs W = A;
    W.nsteps = n0;
    W.bits_stride = (run->nsteps + 31) >> 5;
    const long long kept_all = A.S;
    long long* wcount = nullptr;                                          // accept counts of one continuation window
    double* wsum = nullptr;
    if (n0 < run->nsteps) {   // (window counts, and behind them kernel_adapt's running sums of the call's rows)
      const size_t nsum = (kn->kind == FMCMC_KERNEL_ADAPT) ? (size_t)run->nchains * (size_t)kf : 0;
      e = hipMallocAsync((void**)&wcount, sizeof(long long) * (size_t)run->nchains + sizeof(double) * nsum, stream);
      if (e != hipSuccess) { set_err("hipMallocAsync(window counts) failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
      wc_guard.p = wcount; wc_guard.s = stream;
      if (nsum) wsum = reinterpret_cast<double*>(wcount + run->nchains);
    }
    W.win_sum = wsum;
    if (A.rng_mode == FMCMC_RNG_PHILOX) fill_stream(W, (long long)run->step_base);
    launch_fast(W);
    for (long long s0 = n0; s0 < run->nsteps && e == hipSuccess; ) {     // continuation windows
      const long long w = (run->nsteps - s0 < win) ? run->nsteps - s0 : win;
      const long long rows_done = fmcmc_kept_rows(s0, run->burnin, run->thin);
      W = A;
      W.nsteps = w + 1;
      W.win_cont = 1;
      W.fresh = 0;                 // (kernel state: what the window before wrote back)
      W.win_sum = wsum;
      W.step_off = s0 - 1;
      W.burnin = (run->burnin - s0 + 1 > 1) ? run->burnin - s0 + 1 : 1;
      W.thin_ctr0 = (s0 > run->burnin) ? (int)((s0 - run->burnin) % run->thin) : 0;
      W.bits_stride = (run->nsteps + 31) >> 5;
      W.samples = A.samples + rows_done;
      if (A.logpost) W.logpost = A.logpost + rows_done;
      if (A.draws) W.draws = A.draws + rows_done;
      if (A.accept_bits) W.accept_bits = A.accept_bits + ((s0 - 1) >> 5);
      W.S = kept_all - rows_done;
      W.accept_count = wcount;
      fill_stream(W, (long long)run->step_base + s0 - 1);
      launch_fast(W);
      hipLaunchKernelGGL(add_counts_kernel, dim3((unsigned)((run->nchains + 255) / 256)), dim3(256), 0, stream, A.accept_count, wcount,
                         (long long)run->nchains);
      s0 += w;
    }
  } else
  if (R.base == Form::LOGISTIC) {
    // the logistic-only instantiations: observation-sharded (logistic-sharded / -shadow) where the plan has it and the launch is
    // resident, else chain-sharded
    if (R.form == Form::LOGISTIC_SHARDED && !coop_fits(R.kfn, R.lds_run, R.nb_launch, ncu, dev, K.mode, "sharded logistic evaluation")) R.form = Form::LOGISTIC;
    if (R.form == Form::LOGISTIC_SHARDED) {
      double* shw = nullptr;
      const long long nb_launch = R.nb_launch;
      const int nslots = R.nslots;
      // (+ 8 observations behind the last slice: the pipelined loop's scalar loads run up to three passes ahead without a clamp)
      // (mh_sweep_logit2 holds four chains per workgroup whatever cw says: tables for the larger of the two launch widths)
      const long long ch_tab = (R.ch_shadow > R.ch_launch) ? R.ch_shadow : R.ch_launch;
      const size_t nxs = (size_t)nb_launch * nslots * 2 * m->p + 8 * (size_t)m->p, nth = ((size_t)kn->k * (ch_tab + SH_PAD) + 7) & ~(size_t)7,
                   npt = (size_t)(NT + SH_PAD) * ch_tab, nbar = 32 * 20 / 2;
      e = hipMallocAsync((void**)&shw, sizeof(double) * (nxs + nth + npt + nbar), stream);
      if (e != hipSuccess) { set_err("hipMallocAsync(sharded evaluation) failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
      shw_guard.p = shw; shw_guard.s = stream;
      double* thw = shw; double* ptw = thw + nth; unsigned* bar = (unsigned*)(ptw + npt); double* xs = ptw + npt + nbar;
      (void)hipMemsetAsync(xs + (size_t)nb_launch * nslots * 2 * m->p, 0, sizeof(double) * 8 * (size_t)m->p, stream);
      hipLaunchKernelGGL(logit_build_slices, dim3((unsigned)nb_launch), dim3(256), 0, stream, m->X, (long long)m->n, m->p, nslots, xs);
      A.shard = 2; A.sh_nslots = nslots; A.sh_xs = xs; A.sh_ys = nullptr; A.sh_th = thw; A.sh_part = ptw; A.sh_bar = bar;
      A.sh_t10 = (K.turn >= 0) ? K.turn : 1600700;   // (logit_shard's issue-priority turn: starts at 0.700 of the younger wave's passes, regulated towards a lead of 16 x 256 cycles; knob turn)
      // Round 5: the canonical stream of the call materialised in front of the sweep (rng_fill_kernel), where it fits 1 GiB, instead
      // of being drawn inside the cooperative kernel: there the draws of a tile of steps -- Philox, AS241 with its ~50 constants
      // reloaded from scratch -- sit between two grid-wide hand-overs with 255 workgroups waiting (C5: 1.4 us of a 66 us step,
      // tools/bench_c5_fed.py).  The same variates, the same bits.
      SweepArgs A_own = A;
      const unsigned long long stream_bytes = (unsigned long long)run->nchains * (unsigned long long)run->nsteps * (unsigned long long)(A.kz + 1) * 8ull;
      if (A.rng_mode == FMCMC_RNG_PHILOX && stream_bytes <= (1ull << 30) &&
          (kn->kind >= FMCMC_KERNEL_ADAPT || kn->scheme == FMCMC_SCHEME_JOINT)) {
        double* wsl = nullptr;
        if (hipMallocAsync((void**)&wsl, (size_t)stream_bytes, stream) == hipSuccess) {
          ws_guard.p = wsl; ws_guard.s = stream;
          fill_rng(run, run->step_base, run->nchains, run->nsteps, A.kz, fill_df, wsl, stream);
          A.fed_logu = wsl; A.fed_z = wsl + (size_t)run->nchains * (size_t)run->nsteps; A.rng_mode = FMCMC_RNG_FED;
        } else {
          (void)hipGetLastError();
        }
      }
      // (variates from a stream, the library's or the caller's: the instantiation without the generators in its body, and where the
      //  plan has one the shadow form)
      const void* kfr = R.kfn;
      size_t lds_run = R.lds_run;
      long long ch_run = R.ch_launch;
      if (A.rng_mode == FMCMC_RNG_FED) {
        if (R.kfn_fed && hipFuncSetAttribute(R.kfn_fed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.lds_run) == hipSuccess) kfr = R.kfn_fed;
        else (void)hipGetLastError();
        if (R.kfn_shadow && coop_fits(R.kfn_shadow, R.lds_shadow, nb_launch, ncu, dev, K.mode, nullptr)) {
          kfr = R.kfn_shadow; lds_run = R.lds_shadow; ch_run = R.ch_shadow;
          R.form = Form::LOGISTIC_SHADOW;
        }
      }
      SweepArgs Ab = A;
      Ab.bits_stride = (run->nsteps + 31) >> 5;       // (the owners of mh_spec.hpp address the accept bitmap through it)
      const CoopRun cr = coop_chain_windows(kfr, nb_launch, lds_run, Ab, run->nchains, ch_run, kf, bar, nbar, stream);
      if (cr == COOP_LATER_FAILED) return FMCMC_ERR_DEVICE;
      if (cr == COOP_NOTHING_RAN) {                  // the runtime refused the first cooperative launch: the chain-sharded kernel
        R.form = Form::LOGISTIC;
        A = A_own;
        A.shard = 0; A.sh_xs = nullptr; A.sh_th = nullptr; A.sh_part = nullptr; A.sh_bar = nullptr;
      }
    }
    if (R.form == Form::LOGISTIC) e = launch_k(R.kfn_base, R.nblk, NT, R.lds, stream, A);
  } else
  if (R.base == Form::WIDE) {
    // wide linear models: observation-sharded (sequential, matrix-core or dataflow form) where the plan has it and the launch is
    // resident, else chain-sharded
    if (R.wide2) { A.sh_ngrp = R.ngrp; A.sh_tiles = R.tiles; }
    if (R.form != Form::WIDE && !coop_fits(R.kfn, R.lds_run, R.nb_launch, ncu, dev, K.mode, "sharded evaluation")) R.form = Form::WIDE;
    if (R.form != Form::WIDE) {
      double* shw = nullptr;
      const long long nb_launch = R.nb_launch, ch_launch = R.ch_launch;
      const bool mfma_form = R.mfma_form;
      const size_t nxs = mfma_form ? 0 : (size_t)nb_launch * m->p * SH_MAXO, nys = mfma_form ? 0 : (size_t)nb_launch * SH_MAXO, nth = ((size_t)kn->k * (ch_launch + SH_PAD) + 7) & ~(size_t)7,   // (the partials behind it stay 64-byte aligned)
                   npt = (size_t)(NT + SH_PAD) * ch_launch, nbar = R.wide2 ? 8 * W2_BARW / 2 : 32 * 20 / 2;   // (barrier words counted in doubles)
      const size_t nmf = mfma_form ? (size_t)nb_launch * R.mblk : 0;
      e = hipMallocAsync((void**)&shw, sizeof(double) * (nxs + nys + nth + npt + nbar + nmf), stream);
      if (e != hipSuccess) { set_err("hipMallocAsync(sharded evaluation) failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
      shw_guard.p = shw; shw_guard.s = stream;
      double* xs = shw; double* ys = xs + nxs; double* thw = ys + nys; double* ptw = thw + nth;
      unsigned* bar = (unsigned*)(ptw + npt);
      if (!mfma_form)
        hipLaunchKernelGGL(shard_build_slices, dim3((unsigned)nb_launch), dim3(256), 0, stream, m->X, m->y, (long long)m->n, m->p, R.lpw, R.nslots, xs, ys);
      A.shard = R.lpw; A.sh_nslots = R.nslots; A.sh_xs = xs; A.sh_ys = ys; A.sh_th = thw; A.sh_part = ptw; A.sh_bar = bar;
      if (mfma_form) {
        double* mf = ptw + npt + nbar;
        hipLaunchKernelGGL(shard_build_mfma, dim3((unsigned)nb_launch), dim3(256), 0, stream, m->X, m->y, (long long)m->n, m->p, R.lpw, R.nslots,
                           R.nmt, R.t10, mf, R.mblk);
        A.sh_mfma = mf; A.sh_mblk = R.mblk; A.sh_nmt = R.nmt; A.sh_t10 = R.t10;
      }
      const CoopRun cr = coop_chain_windows(R.kfn, nb_launch, R.lds_run, A, run->nchains, ch_launch, kf, bar, nbar, stream);
      if (cr == COOP_LATER_FAILED) return FMCMC_ERR_DEVICE;
      if (cr == COOP_NOTHING_RAN) {                  // the runtime refused the first cooperative launch: the chain-sharded kernel
        R.form = Form::WIDE;
        A.shard = 0; A.sh_xs = nullptr; A.sh_ys = nullptr; A.sh_th = nullptr; A.sh_part = nullptr; A.sh_bar = nullptr;
        A.sh_mfma = nullptr; A.sh_mblk = 0; A.sh_nmt = 0; A.sh_t10 = 0;
      }
    }
    if (R.form == Form::WIDE) e = launch_k(R.kfn_base, R.nblk, NT, R.lds, stream, A);
  }
  else e = launch_k(R.kfn, R.nblk, NT, R.lds, stream, A);   // resident / general kernel
  g_kernel = kernel_name(R);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) { set_err("HIP launch failed: %s", hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
  // timing ablations and stamps (knob mode=<bits>: 8 stamps in the draws buffer, 32 / 64 / 128 / 1024 parts of a step left out)
  // produce INVALID samples: a call made with one of them says so in fmcmc_last_kernel(), so that its results cannot pass for
  // a product run's
  if (K.mode & (8 | 32 | 64 | 128 | 1024)) {
    static thread_local char kbuf[96];
    snprintf(kbuf, sizeof(kbuf), "invalid-results(mode=%d):%s", K.mode, g_kernel);
    g_kernel = kbuf;
  }
  return FMCMC_OK;
}

int fmcmc_rng_stream_dev(uint64_t seed, int64_t step_base, int64_t chain_base, int64_t nchains, int64_t nsteps,
                         int32_t kz, double student_df, double* logu, double* z, void* hip_stream) {
  if (!logu || !z || nchains < 1 || nsteps < 1 || kz < 1) { set_err("fmcmc_rng_stream_dev: bad argument"); return FMCMC_ERR_ARG; }
  const size_t items = (size_t)nchains * (size_t)nsteps;
  hipLaunchKernelGGL(rng_fill_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                     (unsigned long long)seed, (long long)step_base, (long long)chain_base, (long long)nchains,
                     (long long)nsteps, (int)kz, student_df, logu, z);
  return hipGetLastError() == hipSuccess ? FMCMC_OK : FMCMC_ERR_DEVICE;
}

int fmcmc_detmath_dev(int which, const double* x, double* out, int64_t n, uint64_t seed, void* hip_stream) {
  if (n <= 0) return FMCMC_OK;
  hipLaunchKernelGGL(detmath_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                     which, x, out, (long long)n, (unsigned long long)seed);
  return hipGetLastError() == hipSuccess ? FMCMC_OK : FMCMC_ERR_DEVICE;
}

// Reads the kernel arrays the host side needs (fixed, lb, ub; scale of the uniform kernels; scheme_seq) from their host mirrors,
// or from the device, which synchronises `stream` (fmcmc_mcmc_run_dev's rule), and returns a copy of *kn pointing at them.
static int kernel_host_view(const fmcmc_kernel* kn, hipStream_t stream, uint8_t* fx, double* lb, double* ub, double* sc, int32_t* seq,
                            fmcmc_kernel* kh) {
  if (kn->k < 1 || kn->k > MAXK) { set_err("k=%d outside [1,%d]", kn->k, MAXK); return FMCMC_ERR_UNSUPPORTED; }
  const bool unif = (kn->kind == FMCMC_KERNEL_UNIF || kn->kind == FMCMC_KERNEL_UNIF_REFLECTIVE);
  const bool expl = (is_simple_kind(kn->kind) && kn->scheme == FMCMC_SCHEME_EXPLICIT && kn->scheme_seq &&
                     kn->scheme_len >= 1 && kn->scheme_len <= MAXK);
  const bool mirrored = kn->h_fixed && kn->h_lb && kn->h_ub && (!unif || kn->h_scale) && (!expl || kn->h_scheme_seq);
  if (mirrored) {
    memcpy(fx, kn->h_fixed, (size_t)kn->k);
    memcpy(lb, kn->h_lb, sizeof(double) * (size_t)kn->k);
    memcpy(ub, kn->h_ub, sizeof(double) * (size_t)kn->k);
    if (unif) memcpy(sc, kn->h_scale, sizeof(double) * (size_t)kn->k);
    if (expl) memcpy(seq, kn->h_scheme_seq, sizeof(int32_t) * (size_t)kn->scheme_len);
  } else if (hipMemcpyAsync(fx, kn->fixed, kn->k, hipMemcpyDeviceToHost, stream) != hipSuccess ||
             hipMemcpyAsync(lb, kn->lb, kn->k * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
             hipMemcpyAsync(ub, kn->ub, kn->k * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
             (unif && hipMemcpyAsync(sc, kn->scale, kn->k * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
             (expl && hipMemcpyAsync(seq, kn->scheme_seq, kn->scheme_len * sizeof(int32_t), hipMemcpyDeviceToHost, stream) != hipSuccess) ||
             hipStreamSynchronize(stream) != hipSuccess) {
    set_err("cannot read kernel parameters from device memory");
    return FMCMC_ERR_DEVICE;
  }
  *kh = *kn;
  kh->fixed = fx; kh->lb = lb; kh->ub = ub;
  kh->scale = unif ? sc : nullptr;
  kh->scheme_seq = expl ? seq : nullptr;
  return FMCMC_OK;
}

int fmcmc_mcmc_run_dev(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run,
                       fmcmc_state* st, fmcmc_out* out, void* hip_stream) {
  if (!m || !kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  // `fixed`, `lb`, `ub` (and scale / scheme_seq where they are checked) live on the device.  A caller that passes their
  // host copies (fmcmc_kernel.h_*) gets a call that only enqueues work; otherwise the few bytes are read back here, which
  // synchronises the stream.
  uint8_t fx[MAXK];
  double lb[MAXK], ub[MAXK], sc[MAXK];
  int32_t seq[MAXK];
  hipStream_t stream = (hipStream_t)hip_stream;
  fmcmc_kernel kh;
  const int rv = kernel_host_view(kn, stream, fx, lb, ub, sc, seq, &kh);
  if (rv != FMCMC_OK) return rv;
  int rc = fmcmc_validate(m, &kh, run);
  if (rc != FMCMC_OK) return rc;
  int kf = count_free(kn, fx);
  int bounded = 0;
  for (int j = 0; j < kn->k; j++)
    if (!fx[j] && (lb[j] > -DBL_MAX || ub[j] < DBL_MAX)) bounded = 1;
  return launch_sweep(m, kn, run, st, out, kf, bounded, stream);
}

#define HCHK(x)                                                                    \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      set_err("%s failed: %s", #x, hipGetErrorString(e_));                         \
      rc = FMCMC_ERR_DEVICE;                                                       \
      goto done;                                                                   \
    }                                                                              \
  } while (0)

int fmcmc_mcmc_run_host(const fmcmc_model* m, const fmcmc_kernel* kn, const fmcmc_run* run,
                        fmcmc_state* st, fmcmc_out* out, int device) {
  if (!m || !kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  int rc = fmcmc_validate(m, kn, run);
  if (rc != FMCMC_OK) return rc;
  if (fmcmc_device_count() < 1) { set_err("no HIP device: the engine has no CPU fallback"); return FMCMC_ERR_DEVICE; }
  const int k = kn->k;
  const int kf = count_free(kn, kn->fixed);
  const int64_t C = run->nchains, S = fmcmc_kept_rows(run->nsteps, run->burnin, run->thin);
  const int64_t nwords = (run->nsteps + 31) / 32;
  const bool adaptive = (kn->kind == FMCMC_KERNEL_ADAPT || kn->kind == FMCMC_KERNEL_RAM);
  const bool mirror_h = (kn->kind == FMCMC_KERNEL_NMIRROR || kn->kind == FMCMC_KERNEL_UMIRROR);
  std::vector<void*> allocs;
  auto dalloc = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (bytes == 0) bytes = 8;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    allocs.push_back(p);
    return p;
  };
  fmcmc_model dm = *m;
  fmcmc_kernel dk = *kn;
  fmcmc_run dr = *run;
  fmcmc_state ds = *st;
  fmcmc_out dout = *out;
  hipStream_t stream = nullptr;
  if (out->ld_rows != 0 && out->ld_rows != S) { set_err("fmcmc_out.ld_rows is honoured by fmcmc_mcmc_run_dev only (host buffers are dense)"); return FMCMC_ERR_ARG; }
  dout.ld_rows = 0;
  int bounded = 0;
  for (int j = 0; j < k; j++)
    if (!kn->fixed[j] && (kn->lb[j] > -DBL_MAX || kn->ub[j] < DBL_MAX)) bounded = 1;

  HCHK(hipSetDevice(device));
  HCHK(hipStreamCreate(&stream));
#define UP(dst, src, bytes)                                                                  \
  do {                                                                                       \
    void* p_ = dalloc(bytes);                                                                \
    if (!p_) { set_err("hipMalloc(%zu) failed", (size_t)(bytes)); rc = FMCMC_ERR_DEVICE; goto done; } \
    if ((src) != nullptr) HCHK(hipMemcpyAsync(p_, (src), (bytes), hipMemcpyHostToDevice, stream)); \
    dst = (decltype(dst))p_;                                                                 \
  } while (0)
  if (m->p > 0) UP(dm.X, m->X, sizeof(double) * (size_t)m->p * m->n);
  UP(dm.y, m->y, sizeof(double) * (size_t)m->n);
  UP(dk.mu, kn->mu, sizeof(double) * k);
  UP(dk.scale, kn->scale, sizeof(double) * k);
  UP(dk.lb, kn->lb, sizeof(double) * k);
  UP(dk.ub, kn->ub, sizeof(double) * k);
  UP(dk.fixed, kn->fixed, (size_t)k);
  if (kn->scheme_seq && kn->scheme_len > 0) UP(dk.scheme_seq, kn->scheme_seq, sizeof(int32_t) * (size_t)kn->scheme_len);
  if (kn->constr && kn->kind == FMCMC_KERNEL_RAM) UP(dk.constr, kn->constr, sizeof(double) * (size_t)kf * kf);
  if (st->scheme_cols) UP(ds.scheme_cols, st->scheme_cols, sizeof(int32_t) * (size_t)C * run->nsteps);
  if (run->rng_mode == FMCMC_RNG_FED) {
    const int kz = variates_per_step(kn, kf);
    UP(dr.fed_logu, run->fed_logu, sizeof(double) * (size_t)C * run->nsteps);
    UP(dr.fed_z, run->fed_z, sizeof(double) * (size_t)C * run->nsteps * kz);
  }
  UP(ds.theta0, st->theta0, sizeof(double) * (size_t)C * k);
  UP(ds.f0, (double*)nullptr, sizeof(double) * (size_t)C);
  if (mirror_h) {
    if (!st->mirror_mu || !st->mirror_scale || !st->obs_arate || !st->abs_iter) {
      set_err("mirror kernels need state->mirror_mu, mirror_scale, obs_arate and abs_iter");
      rc = FMCMC_ERR_ARG;
      goto done;
    }
    UP(ds.abs_iter, st->fresh ? nullptr : st->abs_iter, sizeof(int64_t) * (size_t)C);
    UP(ds.mirror_mu, st->fresh ? nullptr : st->mirror_mu, sizeof(double) * (size_t)C * k);
    UP(ds.mirror_scale, st->fresh ? nullptr : st->mirror_scale, sizeof(double) * (size_t)C * k);
    UP(ds.obs_arate, st->fresh ? nullptr : st->obs_arate, sizeof(double) * (size_t)C * k);
  }
  if (adaptive) {
    UP(ds.abs_iter, st->fresh ? nullptr : st->abs_iter, sizeof(int64_t) * (size_t)C);
    UP(ds.Sigma, st->fresh ? nullptr : st->Sigma, sizeof(double) * (size_t)C * kf * kf);
    UP(ds.mean_prev, st->fresh ? nullptr : st->mean_prev, sizeof(double) * (size_t)C * kf);
    UP(ds.have_mean, st->fresh ? nullptr : st->have_mean, sizeof(int32_t) * (size_t)C);
    UP(ds.nerrors, (st->fresh || !st->nerrors) ? nullptr : st->nerrors, sizeof(int32_t) * (size_t)C);
    if (st->fresh || !st->nerrors) HCHK(hipMemsetAsync(ds.nerrors, 0, sizeof(int32_t) * (size_t)C, stream));
  }
  UP(dout.samples, (double*)nullptr, sizeof(double) * (size_t)C * k * S);
  HCHK(hipMemsetAsync(dout.samples, 0xff, sizeof(double) * (size_t)C * k * S, stream));  // NaN fill
  if (out->logpost) UP(dout.logpost, (double*)nullptr, sizeof(double) * (size_t)C * S);
  if (out->draws) UP(dout.draws, (double*)nullptr, sizeof(double) * (size_t)C * k * S);
  UP(dout.accept_count, (int64_t*)nullptr, sizeof(int64_t) * (size_t)C);
  if (out->accept_bits) UP(dout.accept_bits, (uint32_t*)nullptr, sizeof(uint32_t) * (size_t)C * nwords);
  UP(dout.status, (int32_t*)nullptr, sizeof(int32_t) * (size_t)C);
  UP(dout.status_step, (int64_t*)nullptr, sizeof(int64_t) * (size_t)C);
  UP(dout.status_theta, (double*)nullptr, sizeof(double) * (size_t)C * k);
  HCHK(hipMemsetAsync(dout.status_theta, 0, sizeof(double) * (size_t)C * k, stream));
#undef UP
  rc = launch_sweep(&dm, &dk, &dr, &ds, &dout, kf, bounded, stream);
  if (rc != FMCMC_OK) goto done;
#define DOWN(dst, src, bytes) HCHK(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, stream))
  DOWN(st->theta0, ds.theta0, sizeof(double) * (size_t)C * k);
  DOWN(st->f0, ds.f0, sizeof(double) * (size_t)C);
  if (mirror_h) {
    DOWN(st->abs_iter, ds.abs_iter, sizeof(int64_t) * (size_t)C);
    DOWN(st->mirror_mu, ds.mirror_mu, sizeof(double) * (size_t)C * k);
    DOWN(st->mirror_scale, ds.mirror_scale, sizeof(double) * (size_t)C * k);
    DOWN(st->obs_arate, ds.obs_arate, sizeof(double) * (size_t)C * k);
  }
  if (adaptive) {
    DOWN(st->abs_iter, ds.abs_iter, sizeof(int64_t) * (size_t)C);
    DOWN(st->Sigma, ds.Sigma, sizeof(double) * (size_t)C * kf * kf);
    DOWN(st->mean_prev, ds.mean_prev, sizeof(double) * (size_t)C * kf);
    DOWN(st->have_mean, ds.have_mean, sizeof(int32_t) * (size_t)C);
    if (st->nerrors) DOWN(st->nerrors, ds.nerrors, sizeof(int32_t) * (size_t)C);
  }
  if (st->scheme_cols && run->rng_mode != FMCMC_RNG_FED && is_simple_kind(kn->kind) && kn->scheme == FMCMC_SCHEME_RANDOM)
    DOWN(st->scheme_cols, ds.scheme_cols, sizeof(int32_t) * (size_t)C * run->nsteps);
  DOWN(out->samples, dout.samples, sizeof(double) * (size_t)C * k * S);
  if (out->logpost) DOWN(out->logpost, dout.logpost, sizeof(double) * (size_t)C * S);
  if (out->draws) DOWN(out->draws, dout.draws, sizeof(double) * (size_t)C * k * S);
  DOWN(out->accept_count, dout.accept_count, sizeof(int64_t) * (size_t)C);
  if (out->accept_bits) DOWN(out->accept_bits, dout.accept_bits, sizeof(uint32_t) * (size_t)C * nwords);
  DOWN(out->status, dout.status, sizeof(int32_t) * (size_t)C);
  DOWN(out->status_step, dout.status_step, sizeof(int64_t) * (size_t)C);
  DOWN(out->status_theta, dout.status_theta, sizeof(double) * (size_t)C * k);
#undef DOWN
  HCHK(hipStreamSynchronize(stream));
  st->fresh = 0;
  for (int64_t c = 0; c < C; c++)
    if (out->status[c] != FMCMC_CHAIN_OK) {
      // NaN log-posterior: the message of R/mcmc.R:759-765; the engine's own conditions by name
      const char* what = "fun(par) is undefined.";
      switch (out->status[c]) {
        case FMCMC_CHAIN_NAN_LOGPOST: what = "fun(par) is undefined (NaN)."; break;
        case FMCMC_CHAIN_NAN_RATIO: what = "fun(par) is undefined (f1 - f0 is NaN)."; break;
        case FMCMC_CHAIN_NOT_PD: what = "'Sigma' is not positive definite."; break;
        case FMCMC_CHAIN_BAD_WINDOW: what = "subscript out of bounds: the rows kernel_adapt(bw / freq) adapts on reach before the first row of this call."; break;
        case FMCMC_CHAIN_SYNC_TIMEOUT: what = "a grid-wide hand-over of the observation-sharded evaluation timed out; the results of this call are invalid (FMCMC_AMD_DEBUG=shard=0 selects the chain-sharded kernel)."; break;
        default: break;
      }
      // (R/mcmc.R:759-765 attaches the fun / lb / ub hint to a NaN log-posterior only)
      const bool nan_status = out->status[c] == FMCMC_CHAIN_NAN_LOGPOST || out->status[c] == FMCMC_CHAIN_NAN_RATIO;
      set_err("%s (chain %lld, status %d).%s This error ocurred during step i = %lld",
              what, (long long)(run->chain_base + c), out->status[c],
              nan_status ? " Check either -fun- or the -lb- and -ub- parameters." : "", (long long)out->status_step[c]);
      rc = FMCMC_ERR_CHAIN;
      break;
    }
done:
  for (void* p : allocs) hipFree(p);
  if (stream) hipStreamDestroy(stream);
  return rc;
}

// ==============================================================================================
// user-defined log-posteriors: the sweep around a batched callback (fmcmc_logpost_fn; mh_fun.hpp)
// ==============================================================================================
int fmcmc_validate_fun(const fmcmc_kernel* kn, const fmcmc_run* run) {
  if (!kn || !run) { set_err("null argument"); return FMCMC_ERR_ARG; }
  const int rr = validate_run(kn, run);
  if (rr != FMCMC_OK) return rr;
  if (kn->kind == FMCMC_KERNEL_NMIRROR || kn->kind == FMCMC_KERNEL_UMIRROR) {
    set_err("a user-defined -fun- runs with kernel_normal(_reflective), kernel_unif(_reflective), kernel_adapt(bw = 0, freq = 1) "
            "and kernel_ram; the mirror kernels are not supported on this path");
    return FMCMC_ERR_UNSUPPORTED;
  }
  if (kn->kind == FMCMC_KERNEL_ADAPT && (kn->bw > 0 || kn->freq > 1)) {
    set_err("a user-defined -fun- runs kernel_adapt with bw = 0 and freq = 1 only (got bw=%d, freq=%d): the windowed and the "
            "strided adaptation are not supported on this path", kn->bw, kn->freq);
    return FMCMC_ERR_UNSUPPORTED;
  }
  return validate_kernel(kn, run);
}

// The call: every pointer of kn / run / st / out is a DEVICE pointer (fx, lb, ub: host copies of the kernel's).  host_fun: `fun`
// takes host buffers (the theta1 of every chain is copied out and f(theta1) back in around each evaluation).
static int run_fun(const fmcmc_kernel* kn, const uint8_t* fx, const double* lb, const double* ub, const fmcmc_run* run,
                   fmcmc_state* st, fmcmc_out* out, fmcmc_logpost_fn fun, void* user, hipStream_t stream, bool host_fun) {
  if (!fun) { set_err("null log-posterior callback"); return FMCMC_ERR_ARG; }
  const int k = kn->k, kf = count_free(kn, fx);
  const long long C = run->nchains;
  const bool adapt = kn->kind == FMCMC_KERNEL_ADAPT, ram = kn->kind == FMCMC_KERNEL_RAM;
  if ((adapt || ram) && (!st->Sigma || !st->abs_iter || (adapt && (!st->mean_prev || !st->have_mean)))) {
    set_err("kernel_adapt / kernel_ram need state->Sigma and abs_iter (kernel_adapt: mean_prev and have_mean as well)");
    return FMCMC_ERR_ARG;
  }
  if (is_simple_kind(kn->kind) && kn->scheme == FMCMC_SCHEME_RANDOM && run->rng_mode == FMCMC_RNG_FED && !st->scheme_cols) {
    set_err("rng_mode = FED with scheme = 'random' needs state->scheme_cols");
    return FMCMC_ERR_ARG;
  }
  int bounded = 0;
  for (int j = 0; j < k; j++)
    if (!fx[j] && (lb[j] > -DBL_MAX || ub[j] < DBL_MAX)) bounded = 1;
  FunArgs A;
  memset(&A, 0, sizeof(A));
  A.kind = kn->kind; A.k = k; A.kf = kf; A.scheme = kn->scheme; A.warmup = kn->warmup; A.freq = kn->freq < 1 ? 1 : kn->freq;
  A.scheme_len = kn->scheme_len; A.ram_bounded = ram ? bounded : 0;
  A.until = kn->until; A.eps = kn->eps; A.arate = kn->arate;
  A.ram_df = (kn->ram_qfun == FMCMC_RAM_QFUN_NORMAL) ? 0.0 : (kn->ram_qfun == FMCMC_RAM_QFUN_T_DF ? kn->ram_df : (double)kf);
  A.ram_neg_exp = (kn->ram_eta_exp != 0.0) ? -kn->ram_eta_exp : (-2.0 / 3.0);
  A.mu = kn->mu; A.scale = kn->scale; A.lb = kn->lb; A.ub = kn->ub; A.scheme_seq = kn->scheme_seq;
  A.constr = ram ? kn->constr : nullptr;
  A.nchains = C; A.nsteps = run->nsteps; A.burnin = run->burnin; A.thin = run->thin;
  const long long S = fmcmc_kept_rows(run->nsteps, run->burnin, run->thin);
  A.ldS = out->ld_rows > 0 ? out->ld_rows : S;
  if (A.ldS < S) { set_err("fmcmc_out.ld_rows (%lld) is smaller than the %lld kept rows of this call", (long long)out->ld_rows, S); return FMCMC_ERR_ARG; }
  A.chain_base = run->chain_base; A.step_base = run->step_base; A.seed = run->seed;
  A.rng_mode = run->rng_mode; A.kz = variates_per_step(kn, kf); A.fresh = st->fresh;
  A.fed_logu = run->fed_logu; A.fed_z = run->fed_z;
  A.theta0 = st->theta0; A.f0 = st->f0; A.abs_iter = (long long*)st->abs_iter; A.Sigma = st->Sigma; A.mean_prev = st->mean_prev;
  A.have_mean = st->have_mean; A.nerrors = st->nerrors; A.scheme_cols = st->scheme_cols;
  A.samples = out->samples; A.logpost = out->logpost; A.draws = out->draws; A.accept_count = (long long*)out->accept_count;
  A.accept_bits = out->accept_bits; A.status = out->status; A.status_step = (long long*)out->status_step; A.status_theta = out->status_theta;
  {   // the code object is gfx950 only
    int dev = 0;
    hipDeviceProp_t prop;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      set_err("this library is built for gfx950 (MI355X); the current device is another architecture");
      return FMCMC_ERR_DEVICE;
    }
  }
  // scratch of the call: theta1 [C][k] and f(theta1) [C] (what `fun` reads and writes), kernel_adapt's running row sum [C][kf],
  // nerrors [C] when the caller keeps none, the free-parameter list [kf]
  const size_t n_th = (size_t)C * k, n_rs = adapt ? (size_t)C * kf : 0, n_ne = ((adapt || ram) && !st->nerrors) ? (size_t)C : 0;
  const size_t bytes = sizeof(double) * (n_th + (size_t)C + n_rs) + sizeof(int) * (n_ne + (size_t)kf);
  AsyncScratch scr;
  if (hipMallocAsync(&scr.p, bytes, stream) != hipSuccess) {
    (void)hipGetLastError();
    set_err("hipMallocAsync(%zu) for the callback sweep failed", bytes);
    return FMCMC_ERR_DEVICE;
  }
  scr.s = stream;
  double* th1 = (double*)scr.p;
  double* f1 = th1 + n_th;
  A.rsum = adapt ? f1 + C : nullptr;
  int* ne = (int*)(f1 + C + n_rs);
  int* which = ne + n_ne;
  if (n_ne) { A.nerrors = ne; (void)hipMemsetAsync(ne, 0, sizeof(int) * n_ne, stream); }
  A.which = which; A.th1 = th1; A.f1 = f1;
  hipLaunchKernelGGL(fun_which_kernel, dim3(1), dim3(64), 0, stream, kn->fixed, k, which);
  (void)hipMemcpyAsync(th1, st->theta0, sizeof(double) * n_th, hipMemcpyDeviceToDevice, stream);   // row 1: f(initial)

  const int nth = (k <= FMCMC_MAX_K_WAVE) ? 64 : 256;
  const void* kfn = fmh::k_fun(nth);
  const size_t lds = sizeof(double) * fun_lds_doubles(k, kf, kn->kind, nth);
  if (!kfn) { set_err("no device kernel for the callback sweep (k=%d)", k); return FMCMC_ERR_DEVICE; }
  if (lds > 48 * 1024 && hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    set_err("LDS budget exceeded (k=%d)", k);
    return FMCMC_ERR_UNSUPPORTED;
  }
  g_kernel = (nth == 64) ? "fun" : "fun-wg";
  std::vector<double> h_th, h_f;
  if (host_fun) { h_th.resize(n_th); h_f.resize((size_t)C); }
  auto evaluate = [&](long long step) -> int {
    int rc;
    if (host_fun) {
      if (hipMemcpyAsync(h_th.data(), th1, sizeof(double) * n_th, hipMemcpyDeviceToHost, stream) != hipSuccess ||
          hipStreamSynchronize(stream) != hipSuccess) {
        set_err("cannot read the proposals of loop step i = %lld back from the device", step);
        return FMCMC_ERR_DEVICE;
      }
      rc = fun(h_th.data(), (int64_t)C, (int32_t)k, h_f.data(), (void*)stream, user);
      if (rc == 0 && hipMemcpyAsync(f1, h_f.data(), sizeof(double) * (size_t)C, hipMemcpyHostToDevice, stream) != hipSuccess) {
        set_err("cannot copy the log-posterior of loop step i = %lld to the device", step);
        return FMCMC_ERR_DEVICE;
      }
    } else {
      rc = fun(th1, (int64_t)C, (int32_t)k, f1, (void*)stream, user);
    }
    if (rc != 0) {
      set_err("the log-posterior callback returned %d at loop step i = %lld%s", rc, step, step == 1 ? " (row 1: the initial values)" : "");
      return FMCMC_ERR_FUN;
    }
    return FMCMC_OK;
  };
  auto launch = [&](long long step, int phase) -> int {
    A.step = step; A.phase = phase;
    void* kargs[] = {(void*)&A};
    hipError_t e = hipLaunchKernel(kfn, dim3((unsigned)C), dim3((unsigned)nth), kargs, lds, stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { set_err("HIP launch failed at loop step i = %lld: %s", step, hipGetErrorString(e)); return FMCMC_ERR_DEVICE; }
    return FMCMC_OK;
  };
  const long long nsteps = run->nsteps;
  int rc = evaluate(1);
  if (rc == FMCMC_OK) rc = launch(1, FPH_START | (nsteps >= 2 ? FPH_PROPOSE : FPH_FINISH));
  for (long long i = 2; i <= nsteps && rc == FMCMC_OK; i++) {
    const int tail = (i < nsteps ? FPH_PROPOSE : FPH_FINISH);
    rc = evaluate(i);
    if (rc != FMCMC_OK) break;
    if (ram && bounded) {   // f(un-reflected theta1) for the adaptation, then f(theta1) (R/kernel_ram.R:129-152)
      rc = launch(i, FPH_RAM);
      if (rc == FMCMC_OK) rc = evaluate(i);
      if (rc == FMCMC_OK) rc = launch(i, FPH_ACCEPT | tail);
    } else {
      rc = launch(i, (ram ? FPH_RAM : 0) | FPH_ACCEPT | tail);
    }
  }
  return rc;
}

int fmcmc_mcmc_run_fun_dev(const fmcmc_kernel* kn, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out,
                           fmcmc_logpost_fn fun, void* user, void* hip_stream) {
  if (!kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  hipStream_t stream = (hipStream_t)hip_stream;
  uint8_t fx[MAXK];
  double lb[MAXK], ub[MAXK], sc[MAXK];
  int32_t seq[MAXK];
  fmcmc_kernel kh;
  int rc = kernel_host_view(kn, stream, fx, lb, ub, sc, seq, &kh);
  if (rc != FMCMC_OK) return rc;
  rc = fmcmc_validate_fun(&kh, run);
  if (rc != FMCMC_OK) return rc;
  return run_fun(kn, fx, lb, ub, run, st, out, fun, user, stream, false);
}

int fmcmc_mcmc_run_fun_host(const fmcmc_kernel* kn, const fmcmc_run* run, fmcmc_state* st, fmcmc_out* out,
                            fmcmc_logpost_fn fun, void* user, int device) {
  if (!kn || !run || !st || !out) { set_err("null argument"); return FMCMC_ERR_ARG; }
  int rc = fmcmc_validate_fun(kn, run);
  if (rc != FMCMC_OK) return rc;
  if (!kn->fixed || !kn->lb || !kn->ub || !kn->mu || !kn->scale) { set_err("kernel arrays mu, scale, lb, ub and fixed are required"); return FMCMC_ERR_ARG; }
  if (fmcmc_device_count() < 1) { set_err("no HIP device: the engine has no CPU fallback"); return FMCMC_ERR_DEVICE; }
  const int k = kn->k;
  const int kf = count_free(kn, kn->fixed);
  const int64_t C = run->nchains, S = fmcmc_kept_rows(run->nsteps, run->burnin, run->thin);
  const int64_t nwords = (run->nsteps + 31) / 32;
  const bool adaptive = (kn->kind == FMCMC_KERNEL_ADAPT || kn->kind == FMCMC_KERNEL_RAM);
  if (adaptive && (!st->Sigma || !st->abs_iter || !st->mean_prev || !st->have_mean)) {
    set_err("kernel_adapt / kernel_ram need state->Sigma, abs_iter, mean_prev and have_mean");
    return FMCMC_ERR_ARG;
  }
  if (out->ld_rows != 0 && out->ld_rows != S) { set_err("fmcmc_out.ld_rows is honoured by fmcmc_mcmc_run_fun_dev only (host buffers are dense)"); return FMCMC_ERR_ARG; }
  std::vector<void*> allocs;
  auto dalloc = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (bytes == 0) bytes = 8;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    allocs.push_back(p);
    return p;
  };
  fmcmc_kernel dk = *kn;
  fmcmc_run dr = *run;
  fmcmc_state ds = *st;
  fmcmc_out dout = *out;
  dout.ld_rows = 0;
  hipStream_t stream = nullptr;
  HCHK(hipSetDevice(device));
  HCHK(hipStreamCreate(&stream));
#define UP(dst, src, bytes)                                                                  \
  do {                                                                                       \
    void* p_ = dalloc(bytes);                                                                \
    if (!p_) { set_err("hipMalloc(%zu) failed", (size_t)(bytes)); rc = FMCMC_ERR_DEVICE; goto done; } \
    if ((src) != nullptr) HCHK(hipMemcpyAsync(p_, (src), (bytes), hipMemcpyHostToDevice, stream)); \
    dst = (decltype(dst))p_;                                                                 \
  } while (0)
  UP(dk.mu, kn->mu, sizeof(double) * k);
  UP(dk.scale, kn->scale, sizeof(double) * k);
  UP(dk.lb, kn->lb, sizeof(double) * k);
  UP(dk.ub, kn->ub, sizeof(double) * k);
  UP(dk.fixed, kn->fixed, (size_t)k);
  if (kn->scheme_seq && kn->scheme_len > 0) UP(dk.scheme_seq, kn->scheme_seq, sizeof(int32_t) * (size_t)kn->scheme_len);
  if (kn->constr && kn->kind == FMCMC_KERNEL_RAM) UP(dk.constr, kn->constr, sizeof(double) * (size_t)kf * kf);
  if (st->scheme_cols) UP(ds.scheme_cols, st->scheme_cols, sizeof(int32_t) * (size_t)C * run->nsteps);
  if (run->rng_mode == FMCMC_RNG_FED) {
    const int kz = variates_per_step(kn, kf);
    UP(dr.fed_logu, run->fed_logu, sizeof(double) * (size_t)C * run->nsteps);
    UP(dr.fed_z, run->fed_z, sizeof(double) * (size_t)C * run->nsteps * kz);
  }
  UP(ds.theta0, st->theta0, sizeof(double) * (size_t)C * k);
  UP(ds.f0, (double*)nullptr, sizeof(double) * (size_t)C);
  if (adaptive) {
    UP(ds.abs_iter, st->fresh ? nullptr : st->abs_iter, sizeof(int64_t) * (size_t)C);
    UP(ds.Sigma, st->fresh ? nullptr : st->Sigma, sizeof(double) * (size_t)C * kf * kf);
    UP(ds.mean_prev, st->fresh ? nullptr : st->mean_prev, sizeof(double) * (size_t)C * kf);
    UP(ds.have_mean, st->fresh ? nullptr : st->have_mean, sizeof(int32_t) * (size_t)C);
    UP(ds.nerrors, (st->fresh || !st->nerrors) ? nullptr : st->nerrors, sizeof(int32_t) * (size_t)C);
    if (st->fresh || !st->nerrors) HCHK(hipMemsetAsync(ds.nerrors, 0, sizeof(int32_t) * (size_t)C, stream));
  }
  UP(dout.samples, (double*)nullptr, sizeof(double) * (size_t)C * k * S);
  HCHK(hipMemsetAsync(dout.samples, 0xff, sizeof(double) * (size_t)C * k * S, stream));  // NaN fill
  if (out->logpost) UP(dout.logpost, (double*)nullptr, sizeof(double) * (size_t)C * S);
  if (out->draws) UP(dout.draws, (double*)nullptr, sizeof(double) * (size_t)C * k * S);
  UP(dout.accept_count, (int64_t*)nullptr, sizeof(int64_t) * (size_t)C);
  if (out->accept_bits) UP(dout.accept_bits, (uint32_t*)nullptr, sizeof(uint32_t) * (size_t)C * nwords);
  UP(dout.status, (int32_t*)nullptr, sizeof(int32_t) * (size_t)C);
  UP(dout.status_step, (int64_t*)nullptr, sizeof(int64_t) * (size_t)C);
  UP(dout.status_theta, (double*)nullptr, sizeof(double) * (size_t)C * k);
  HCHK(hipMemsetAsync(dout.status_theta, 0, sizeof(double) * (size_t)C * k, stream));
#undef UP
  rc = run_fun(&dk, kn->fixed, kn->lb, kn->ub, &dr, &ds, &dout, fun, user, stream, true);
  if (rc != FMCMC_OK) goto done;
#define DOWN(dst, src, bytes) HCHK(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, stream))
  DOWN(st->theta0, ds.theta0, sizeof(double) * (size_t)C * k);
  DOWN(st->f0, ds.f0, sizeof(double) * (size_t)C);
  if (adaptive) {
    DOWN(st->abs_iter, ds.abs_iter, sizeof(int64_t) * (size_t)C);
    DOWN(st->Sigma, ds.Sigma, sizeof(double) * (size_t)C * kf * kf);
    DOWN(st->mean_prev, ds.mean_prev, sizeof(double) * (size_t)C * kf);
    DOWN(st->have_mean, ds.have_mean, sizeof(int32_t) * (size_t)C);
    if (st->nerrors) DOWN(st->nerrors, ds.nerrors, sizeof(int32_t) * (size_t)C);
  }
  if (st->scheme_cols && run->rng_mode != FMCMC_RNG_FED && is_simple_kind(kn->kind) && kn->scheme == FMCMC_SCHEME_RANDOM)
    DOWN(st->scheme_cols, ds.scheme_cols, sizeof(int32_t) * (size_t)C * run->nsteps);
  DOWN(out->samples, dout.samples, sizeof(double) * (size_t)C * k * S);
  if (out->logpost) DOWN(out->logpost, dout.logpost, sizeof(double) * (size_t)C * S);
  if (out->draws) DOWN(out->draws, dout.draws, sizeof(double) * (size_t)C * k * S);
  DOWN(out->accept_count, dout.accept_count, sizeof(int64_t) * (size_t)C);
  if (out->accept_bits) DOWN(out->accept_bits, dout.accept_bits, sizeof(uint32_t) * (size_t)C * nwords);
  DOWN(out->status, dout.status, sizeof(int32_t) * (size_t)C);
  DOWN(out->status_step, dout.status_step, sizeof(int64_t) * (size_t)C);
  DOWN(out->status_theta, dout.status_theta, sizeof(double) * (size_t)C * k);
#undef DOWN
  HCHK(hipStreamSynchronize(stream));
  st->fresh = 0;
  for (int64_t c = 0; c < C; c++)
    if (out->status[c] != FMCMC_CHAIN_OK) {
      const char* what = out->status[c] == FMCMC_CHAIN_NAN_LOGPOST ? "fun(par) is undefined (NaN)."
                       : out->status[c] == FMCMC_CHAIN_NAN_RATIO ? "fun(par) is undefined (f1 - f0 is NaN)."
                       : out->status[c] == FMCMC_CHAIN_NOT_PD ? "'Sigma' is not positive definite." : "fun(par) is undefined.";
      const bool nan_status = out->status[c] == FMCMC_CHAIN_NAN_LOGPOST || out->status[c] == FMCMC_CHAIN_NAN_RATIO;
      set_err("%s (chain %lld, status %d).%s This error ocurred during step i = %lld",
              what, (long long)(run->chain_base + c), out->status[c],
              nan_status ? " Check either -fun- or the -lb- and -ub- parameters." : "", (long long)out->status_step[c]);
      rc = FMCMC_ERR_CHAIN;
      break;
    }
done:
  if (stream) (void)hipStreamSynchronize(stream);   // (the call's stream-ordered scratch is released before its buffers)
  for (void* p : allocs) hipFree(p);
  if (stream) hipStreamDestroy(stream);
  return rc;
}

}  // extern "C"
