// k_lat_l3b.hip -- mh_sweep_lat<2, P, reg_slots(P), LOGISTIC> (mh_lat.hpp): the latency form for the logistic family with 8 .. 15 covariates (up to
// 2048 observations: four slots of P doubles per lane), the reflective kernels
#include "mh_tu.hpp"
#include "mh_lat.hpp"

namespace fmh {
FMH_HIDDEN const void* k_lat_lg2w(int p) {
  switch (p) {
    case 8: return (const void*)mh_sweep_lat<2, 8, reg_slots(8), FMCMC_FAM_LOGISTIC>;
    case 9: return (const void*)mh_sweep_lat<2, 9, reg_slots(9), FMCMC_FAM_LOGISTIC>;
    case 10: return (const void*)mh_sweep_lat<2, 10, reg_slots(10), FMCMC_FAM_LOGISTIC>;
    case 11: return (const void*)mh_sweep_lat<2, 11, reg_slots(11), FMCMC_FAM_LOGISTIC>;
    case 12: return (const void*)mh_sweep_lat<2, 12, reg_slots(12), FMCMC_FAM_LOGISTIC>;
    case 13: return (const void*)mh_sweep_lat<2, 13, reg_slots(13), FMCMC_FAM_LOGISTIC>;
    case 14: return (const void*)mh_sweep_lat<2, 14, reg_slots(14), FMCMC_FAM_LOGISTIC>;
    case 15: return (const void*)mh_sweep_lat<2, 15, reg_slots(15), FMCMC_FAM_LOGISTIC>;
    default: return nullptr;
  }
}
}  // namespace fmh
