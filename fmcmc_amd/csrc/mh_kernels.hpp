// mh_kernels.hpp -- kernel look-ups: shape -> the host handle of the instantiation that runs it (nullptr: none compiled).
// plan_route (mh_route.hpp) picks the handle, launch_sweep (mh_engine.hip) launches it with hipLaunchKernel /
// hipLaunchCooperativeKernel; every kernel takes ONE argument, the SweepArgs of the launch, by value.
#pragma once

#define FMH_HIDDEN __attribute__((visibility("hidden")))

namespace fmh {
// Which instantiations exist is written once per kernel template, in the table of its source (FMH_TABLE of k_lat.hip, k_spec.hip,
// k_mfma.hip, k_streamed.hip: mh_parts.hpp; the look-ups of k_mfma_ad.hip, k_wide2.hip, k_logit2.hip, k_fun.hip themselves).
// Observation slots (of 512) the register kernels hold per compute lane at p covariates: the OPTMAX of every mh_sweep_lat /
// mh_sweep_spec instantiation -- P doubles per slot; 0: no instantiation
constexpr int reg_slots(int p) { return p < 0 ? 0 : p <= 3 ? 20 : p <= 5 ? 10 : p <= 7 ? 8 : p <= 15 ? 4 : 0; }
// Observation slots mh_sweep_mfma holds in its 80 operand registers per lane (one / two operand groups); 0: none, streamed forms only
constexpr int mfma_reg_slots(int p) { return p < 0 ? 0 : p <= 3 ? 20 : p <= 7 ? 10 : 0; }
// k_streamed.hip, mh_sweep_kernel: every family / proposal kernel / scheme at cw chains per workgroup; the register-resident shapes
FMH_HIDDEN const void* k_general(int cw);
FMH_HIDDEN const void* k_resident(int p, int kind);
// wide linear models: lpw = 0 (chain-sharded), 2, 4 (observation-sharded, cooperative); (cw, lpw) = (1, 2) is also the long-data form
FMH_HIDDEN const void* k_wide(int cw, int lpw, int kind);
// logistic only: sharded = 0 | 1 | 2 (chain-sharded | observation-sharded | the same, variates from a materialised stream only)
FMH_HIDDEN const void* k_logit(int cw, int sharded, int kind);
// k_logit2.hip: mh_sweep_logit2<KIND> (kind 1, 2): the observation-sharded sweep with the owners in the shadow of the hand-overs
FMH_HIDDEN const void* k_logit2(int kind);
FMH_HIDDEN size_t k_logit2_lds(int k);
FMH_HIDDEN const void* k_logit2a(int kind);     // mh_sweep_logit2a<KIND> (kind 3, 4; k <= 8, no fixed parameter, unbounded kernel_ram)
FMH_HIDDEN size_t k_logit2a_lds();
// k_mfma.hip: mh_sweep_mfma on ng operand groups with ns slots in registers (big: more than 4 GiB of samples), and its
// streamed-operand form with nsres of the slots resident
FMH_HIDDEN const void* k_mfma(int kv, int ng, int ns, int big);
FMH_HIDDEN const void* k_mfma_ext(int kv, int ng, int nsres, int big);
// k_mfma_ad.hip: mh_sweep_mfma_ad<KIND, NG, KX, BND, NSV>: kx = compile-time row count (5, 9), 0 (k <= 8), -1 (matrices in
//                LDS), -2 (mirror kernels); shrt = 1: one resident slot
FMH_HIDDEN const void* k_mfma_ad(int kind, int ng, int kx, int bnd, int shrt);
// k_spec.hip: mh_sweep_spec of the linear model at p covariates
FMH_HIDDEN const void* k_spec(int p, int kind);
FMH_HIDDEN const void* k_spec_ring(int p, int logistic);   // kernel_adapt(freq = 2 .. 8)
// (the slot count of mh_sweep_spec at p covariates under a proposal kernel: 8 .. 15 covariates, the adaptive and mirror kernels only)
inline int k_spec_optmax(int p, int kind) {
  return (p <= 7 || kind == FMCMC_KERNEL_ADAPT || kind == FMCMC_KERNEL_RAM || kind == FMCMC_KERNEL_NMIRROR || kind == FMCMC_KERNEL_UMIRROR) ? reg_slots(p) : 0;
}
FMH_HIDDEN const void* k_spec_logit(int p, int kind);      // the logistic model
FMH_HIDDEN size_t k_spec_logit_lds(int adaptive);
// k_lat.hip: mh_sweep_lat, the linear and the logistic model
FMH_HIDDEN const void* k_lat(int p, int kind);
FMH_HIDDEN const void* k_lat_logit(int p, int kind);
FMH_HIDDEN size_t k_lat_logit_lds();
// k_wide2.hip: mh_sweep_wide2<KIND, NMT> (kind 1, 2, 4; nmt 1..3) and mh_sweep_bigk<HBM> (hbm 0: matrices in LDS, 1: in HBM)
FMH_HIDDEN const void* k_wide2(int kind, int nmt);
FMH_HIDDEN const void* k_bigk(int hbm);
// k_fun.hip: mh_fun_step<NTH> (mh_fun.hpp), the steps around a caller-evaluated log-posterior: nth = 64 (k <= 64), 256 (k > 64)
FMH_HIDDEN const void* k_fun(int nth);
// k_fun.hip: mh_user_step<NTH> (mh_user.hpp), the accept / store step of a caller-defined transition kernel, at the same widths;
// logpost_eval_kernel, the families' log-posterior at caller-given points (one workgroup of 512 threads per chain)
FMH_HIDDEN const void* k_user(int nth);
FMH_HIDDEN const void* k_logpost_eval();
// k_fun.hip: mh_sweep_batch<LDS_DATA, MASKED> (mh_batch.hpp), one model on many datasets: the dataset in LDS, or streamed every
// step; with or without the dataset mask of fmcmc_mcmc_run_batch_sel_dev
FMH_HIDDEN const void* k_batch(bool lds_data, bool masked);
}  // namespace fmh
