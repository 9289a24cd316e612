// mh_prep.hpp -- the data-preparation kernels of the launcher (mh_engine.hip, launch_sweep / run_fun): the operand stream of the
// MFMA forms, the logistic sums, the per-workgroup slices of the observation-sharded forms, the free-parameter list of the
// callback path, the window accept counts; and the diagnostic that evaluates the deterministic math headers on the device.
// Included by mh_engine.hip only, behind the headers whose constants they use (NT, NW, SH_MAXO, SHM_T, shm_hdr).
#pragma once

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
    case 11: { double up; fmh_pnorm_both(v, &r, &up); break; }   // Phi(v)
    case 12: { double lo; fmh_pnorm_both(v, &lo, &r); break; }   // 1 - Phi(v)
    case 13: r = fmh_tan_0_halfpi(v); break;
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
// |x| of every column (a NaN stays).  One workgroup per dataset, once per launch: n (p + 1) additions.
__device__ __forceinline__ void logit_hs_wg(const double* X, const double* y, long long n, int p, int ic, double* hs) {
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
__global__ __launch_bounds__(NT) void logit_hs_kernel(const double* X, const double* y, long long n, int p, int ic, double* hs) {
  logit_hs_wg(X, y, n, p, ic, hs);
}
// the same sums of every dataset of a batch (mh_batch.hpp): workgroup d serves X + d x_stride, y + d y_stride -> hs + d hs_stride
__global__ __launch_bounds__(NT) void logit_hs_batch_kernel(const double* X, const double* y, long long n, int p, int ic, double* hs,
                                                            long long x_stride, long long y_stride, long long hs_stride) {
  const long long d = blockIdx.x;
  logit_hs_wg(X + d * x_stride, y + d * y_stride, n, p, ic, hs + d * hs_stride);
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
