// k_spec.hip -- mh_sweep_spec<P, reg_slots(P), KIND, FAM, RING> (mh_spec.hpp): the wave-specialised sweep, 8 compute + 4 owner
// wavefronts meeting on LDS sequence words, one to four chains per workgroup; linear and logistic model.  Compiled once per part
// (mh_parts.hpp).
#define FMH_PARTS(X) X(spec_a) X(spec_n) X(spec_m) X(spec_r) X(spec_w1) X(spec_w2) X(spec_w3) X(spec_w4) X(spec_l1) X(spec_l2) X(spec_lw1) X(spec_lw2)
#define FMH_LOOKUPS_spec_a 1
#include "mh_tu.hpp"
#include "mh_spec.hpp"

#define LINREG FMCMC_FAM_GAUSSIAN_LINREG
#define LOGISTIC FMCMC_FAM_LOGISTIC
#define FMH_KERNEL(KIND, FAM, RING, P) mh_sweep_spec<P, reg_slots(P), KIND, FAM, RING>
// rows: part, KIND, FAM, RING, p (0: no covariate, the iid Normal family; 8 and more: up to 2048 observations, four slots of P doubles
// per compute lane, the register owner at the compile-time width k <= 16)
#define FMH_TABLE(R)                                                                                                              \
  /* linear model.  kernel_adapt / kernel_ram (config C3); */                                                                     \
  FMH_P0_7(R, spec_a, FMCMC_KERNEL_ADAPT, LINREG, false) FMH_P0_7(R, spec_a, FMCMC_KERNEL_RAM, LINREG, false)                     \
  FMH_P8_11(R, spec_w1, FMCMC_KERNEL_ADAPT, LINREG, false) FMH_P12_14(R, spec_w2, FMCMC_KERNEL_ADAPT, LINREG, false)              \
  FMH_P8_11(R, spec_w3, FMCMC_KERNEL_RAM, LINREG, false) FMH_P12_14(R, spec_w4, FMCMC_KERNEL_RAM, LINREG, false)                  \
  /* the normal / uniform kernels at p = 1, 3: the VALU partner of mh_sweep_mfma (knob mfma=0), a second implementation of the   \
     same sweep for the parity tests; */                                                                                          \
  R(spec_n, FMCMC_KERNEL_NORMAL, LINREG, false, 1) R(spec_n, FMCMC_KERNEL_NORMAL_REFLECTIVE, LINREG, false, 1)                    \
  R(spec_n, FMCMC_KERNEL_NORMAL, LINREG, false, 3) R(spec_n, FMCMC_KERNEL_NORMAL_REFLECTIVE, LINREG, false, 3)                    \
  /* the mirror kernels (R/kernel_mirror.R), their owner mfma_owner_mirror on the same sequence words */                          \
  FMH_P0_7(R, spec_m, FMCMC_KERNEL_NMIRROR, LINREG, false) FMH_P8_14(R, spec_m, FMCMC_KERNEL_NMIRROR, LINREG, false)              \
  FMH_P0_7(R, spec_m, FMCMC_KERNEL_UMIRROR, LINREG, false) FMH_P8_14(R, spec_m, FMCMC_KERNEL_UMIRROR, LINREG, false)              \
  /* RING: kernel_adapt(freq = 2 .. 8, bw = 0) on the register owner with the LDS ring of the chain's last rows, both models */   \
  FMH_P0_7(R, spec_r, FMCMC_KERNEL_ADAPT, LINREG, true) FMH_P1_7(R, spec_r, FMCMC_KERNEL_ADAPT, LOGISTIC, true)                   \
  /* logistic model: the normal / uniform kernels; kernel_adapt / kernel_ram */                                                   \
  FMH_P1_7(R, spec_l1, FMCMC_KERNEL_NORMAL, LOGISTIC, false) FMH_P1_7(R, spec_l1, FMCMC_KERNEL_NORMAL_REFLECTIVE, LOGISTIC, false) \
  FMH_P1_7(R, spec_l2, FMCMC_KERNEL_ADAPT, LOGISTIC, false) FMH_P1_7(R, spec_l2, FMCMC_KERNEL_RAM, LOGISTIC, false)               \
  FMH_P8_15(R, spec_lw1, FMCMC_KERNEL_ADAPT, LOGISTIC, false) FMH_P8_15(R, spec_lw2, FMCMC_KERNEL_RAM, LOGISTIC, false)
#include "mh_parts.hpp"

#if FMH_HAS_LOOKUPS
namespace fmh {
const void* k_spec(int p, int kind) { return find_kernel(kind, LINREG, false, p); }
const void* k_spec_ring(int p, int logistic) { return find_kernel(FMCMC_KERNEL_ADAPT, logistic ? LOGISTIC : LINREG, true, p); }
const void* k_spec_logit(int p, int kind) { return find_kernel(kind, LOGISTIC, false, p); }
size_t k_spec_logit_lds(int adaptive) { return spec_logit_lds_bytes(adaptive != 0); }
}  // namespace fmh
#endif
