// k_fun.hip -- mh_fun_step<NTH> (mh_fun.hpp: the sweep around a caller-evaluated log-posterior, fmcmc_mcmc_run_fun_*):
// NTH = 64 (k <= 64, one wavefront per chain) and 256 (k > 64, one workgroup per chain); and, for a caller-defined transition
// kernel (mh_user.hpp, fmcmc_mcmc_run_user_dev), mh_user_step<NTH> at the same two widths and the families' batched evaluator;
// and mh_sweep_batch<LDS_DATA, MASKED> (mh_batch.hpp, fmcmc_mcmc_run_batch_*): the two of them fused into one step loop per chain
#define FMH_WITH_FUN_KERNEL
#include "mh_tu.hpp"
#include "mh_fun.hpp"
#include "mh_user.hpp"
#include "mh_batch.hpp"

namespace fmh {
const void* k_fun(int nth) { return nth == 64 ? (const void*)mh_fun_step<64> : nth == 256 ? (const void*)mh_fun_step<256> : nullptr; }
const void* k_user(int nth) { return nth == 64 ? (const void*)mh_user_step<64> : nth == 256 ? (const void*)mh_user_step<256> : nullptr; }
const void* k_logpost_eval() { return (const void*)logpost_eval_kernel; }
const void* k_batch(bool lds_data, bool masked) {
  if (masked) return lds_data ? (const void*)mh_sweep_batch<true, true> : (const void*)mh_sweep_batch<false, true>;
  return lds_data ? (const void*)mh_sweep_batch<true, false> : (const void*)mh_sweep_batch<false, false>;
}
}  // namespace fmh
