// mh_owner.hpp -- what the owner waves of the stream-fed kernels share besides their arithmetic.  One owner wave per chain
// (mh_spec.hpp: spec_owner_adaptive, spec_owner_adaptive_reg, mfma_owner_mirror, the normal / uniform owner inside mh_sweep_spec; the
// first three also serve mh_sweep_mfma_ad and mh_sweep_logit2a) reads as "wait, decide, adapt, propose, store"; the pieces, by phase:
//   start    WindowCarry      status, thinning counter and step offset as a launch starts (a continuation window takes them over)
//   wait     fold_partials    the 8 compute waves' lane partials of a chain -> the canonical total (SpecSync, SpecSyncB)
//   decide   linreg_logpost   the Gaussian closed form from the total and sigma (the slow case of the owners' prepare() fast paths;
//                             also mh_sweep_mfma's and mh_sweep_lat's)
//            ChainStream      the chain's block of the variate stream: z(row), logu(row), rows clamped to the launch's last
//   end      owner_writeback  f0, accept count and status of the chain; every role writes its own state behind it
// Every piece is forced inline, holds plain values (no reference to the SweepArgs) and is in a role only where the kernels built on
// it are, function for function, the device code of the locals and lambdas it replaced (tools/isa_diff.py against the commit
// before; profiles/owner_io_isa.txt).  That is why the row stores and the accept bitmap are still each role's own lines, and why
// the adaptive owners address the stream themselves: as helpers of any shape tried (aggregate, factory, constructor, free function)
// they moved the register allocation of kernels that already spill scalar registers (profiles/owner_io_resources.md).
#pragma once

namespace {

// Gaussian linear model: log-posterior from the total of squared residuals and sigma (dn: the number of observations as a double)
__device__ __forceinline__ double linreg_logpost(double tot, double sigma, double dn, int guard) {
  double f;
  if (sigma < 0.0 || fmh_isnan(sigma)) f = fmh_nan();
  else if (sigma == 0.0) f = -fmh_inf();
  else {
    double t1 = fmh_log(sigma) + FMH_K(FMH_LN_SQRT_2PI);
    double q = (0.5 * tot) / (sigma * sigma);
    f = -(dn * t1) - q;
  }
  if (guard && !fmh_isfinite(f)) f = -fmh_inf();
  return f;
}

// the canonical total of chain myc's 512 lane partials: this lane folds canonical lanes 8 lane .. 8 lane + 7, then the wave's tree
__device__ __forceinline__ double fold_partials(const double* s_tr, int myc) {
  const int lane = threadIdx.x & 63;
  const double* src = s_tr + myc * (8 * PIPE_TRS) + lane;
  const double v0 = src[0 * PIPE_TRS], v1 = src[1 * PIPE_TRS], v2 = src[2 * PIPE_TRS], v3 = src[3 * PIPE_TRS];
  const double v4 = src[4 * PIPE_TRS], v5 = src[5 * PIPE_TRS], v6 = src[6 * PIPE_TRS], v7 = src[7 * PIPE_TRS];
  return wave_xor_sum(((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)));
}

// The chain's block of the variate stream: a wave-uniform 64-bit base plus 32-bit byte offsets per lane and row -- one scalar-base
// load each (32-bit offsets from the BUFFER base capped a call at 4 GiB).  Rows are clamped to the launch's last.
struct ChainStream {
  const char* const z_base; const unsigned int z_lane; const double* const lu_row; const int kz, nsteps;
  __device__ __forceinline__ int clamped(int row) const { return row < nsteps ? row : nsteps - 1; }
  __device__ __forceinline__ double z(int row) const {      // the lane's variate of stream row `row`
    return *reinterpret_cast<const double*>(z_base + (z_lane + (unsigned int)clamped(row) * (unsigned int)(kz * 8)));
  }
  __device__ __forceinline__ double logu(int row) const { return lu_row[clamped(row)]; }
};
__device__ __forceinline__ ChainStream chain_stream(const SweepArgs& A, int cl, int kz, int zl) {   // zl: the lane's variate column
  const int nsteps = (int)A.nsteps;
  return {reinterpret_cast<const char*>(A.fed_z) + ((long long)cl * nsteps) * kz * 8, (unsigned int)zl * 8u,
          A.fed_logu + (long long)cl * nsteps, kz, nsteps};
}

// What a launch starts from.  A continuation window of a long call (launch_stream_fed, SweepArgs.win_cont) takes over the chain
// status and the thinning counter the windows before it left; the step-dependent rules read the CALL's step ioff + i.  (The accept
// COUNT is per launch: the host adds the windows up.)
struct WindowCarry {
  const int status, thin_ctr, ioff;
};
__device__ __forceinline__ WindowCarry window_carry(const SweepArgs& A, int cl) {
  return {A.win_cont ? A.status[cl] : FMCMC_CHAIN_OK, A.thin_ctr0, (int)A.step_off};
}

// the scalar tail every owner ends with (a failed chain's status and step were written where it failed)
__device__ __forceinline__ void owner_writeback(const SweepArgs& A, int cl, int lane, double f0, int nacc, int status) {
  if (lane == 0) {
    A.f0[cl] = f0;
    A.accept_count[cl] = nacc;
    if (status == FMCMC_CHAIN_OK) { A.status[cl] = FMCMC_CHAIN_OK; A.status_step[cl] = 0; }
  }
}

}  // namespace
