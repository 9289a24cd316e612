// k_lat_l2b.hip -- mh_sweep_lat<2, P, OPTMAX, LOGISTIC> (mh_lat.hpp): the latency form for the logistic family (round 5), the reflective kernels, p = 4 .. 7
#include "mh_tu.hpp"
#include "mh_lat.hpp"

namespace fmh {
FMH_HIDDEN const void* k_lat_lg2b(int p) {
  switch (p) {
    case 4: return (const void*)mh_sweep_lat<2, 4, reg_slots(4), FMCMC_FAM_LOGISTIC>;
    case 5: return (const void*)mh_sweep_lat<2, 5, reg_slots(5), FMCMC_FAM_LOGISTIC>;
    case 6: return (const void*)mh_sweep_lat<2, 6, reg_slots(6), FMCMC_FAM_LOGISTIC>;
    case 7: return (const void*)mh_sweep_lat<2, 7, reg_slots(7), FMCMC_FAM_LOGISTIC>;
    default: return nullptr;
  }
}
}  // namespace fmh
