// k_lat_l2a.hip -- mh_sweep_lat<2, P, OPTMAX, LOGISTIC> (mh_lat.hpp): the latency form for the logistic family (round 5), the reflective kernels, p = 1 .. 3
#include "mh_tu.hpp"
#include "mh_lat.hpp"

namespace fmh {
FMH_HIDDEN const void* k_lat_lg2c();   // k_lat_l2c.hip: p = 3
FMH_HIDDEN const void* k_lat_lg2a(int p) {
  switch (p) {
    case 1: return (const void*)mh_sweep_lat<2, 1, reg_slots(1), FMCMC_FAM_LOGISTIC>;
    case 2: return (const void*)mh_sweep_lat<2, 2, reg_slots(2), FMCMC_FAM_LOGISTIC>;
    case 3: return k_lat_lg2c();
    default: return nullptr;
  }
}
}  // namespace fmh
