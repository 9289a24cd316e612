// k_lat.hip -- mh_sweep_lat<KIND, P, reg_slots(P), FAM> (mh_lat.hpp): the latency form (one to three chains per workgroup) of the
// linear and the logistic model, kernel_normal / kernel_unif (KIND 1) and the reflective kernels (KIND 2).  Compiled once per part
// (mh_parts.hpp); the 20-slot instantiations, the longest compiles of the library, are parts of their own.
#define FMH_PARTS(X) X(lat1a) X(lat1b) X(lat1c) X(lat1d) X(lat2a) X(lat2b) X(lat2c) X(lat2d) X(lat3a) X(lat3b) X(lat_l1a) X(lat_l1b) X(lat_l1c) X(lat_l2a) X(lat_l2b) X(lat_l2c) X(lat_l3a) X(lat_l3b)
#define FMH_LOOKUPS_lat1a 1
#include "mh_tu.hpp"
#include "mh_lat.hpp"

#define LINREG FMCMC_FAM_GAUSSIAN_LINREG
#define LOGISTIC FMCMC_FAM_LOGISTIC
#define FMH_KERNEL(KIND, FAM, P) mh_sweep_lat<KIND, P, reg_slots(P), FAM>
// rows: part, KIND, FAM, p.  Linear model p = 0 .. 15 (0: iid Normal, an intercept and no covariate; 3: C2's shape; 8 .. 15 on up to
// 2048 observations, four slots of P + 1 doubles per lane), logistic p = 1 .. 15
#define FMH_TABLE(R)                                                                                                       \
  R(lat1a, 1, LINREG, 0) R(lat1a, 1, LINREG, 1) R(lat1d, 1, LINREG, 2) R(lat1b, 1, LINREG, 3) FMH_P4_7(R, lat1c, 1, LINREG) \
  R(lat2a, 2, LINREG, 0) R(lat2a, 2, LINREG, 1) R(lat2d, 2, LINREG, 2) R(lat2b, 2, LINREG, 3) FMH_P4_7(R, lat2c, 2, LINREG) \
  FMH_P8_15(R, lat3a, 1, LINREG) FMH_P8_15(R, lat3b, 2, LINREG)                                                            \
  R(lat_l1a, 1, LOGISTIC, 1) R(lat_l1a, 1, LOGISTIC, 2) R(lat_l1c, 1, LOGISTIC, 3) FMH_P4_7(R, lat_l1b, 1, LOGISTIC)       \
  R(lat_l2a, 2, LOGISTIC, 1) R(lat_l2a, 2, LOGISTIC, 2) R(lat_l2c, 2, LOGISTIC, 3) FMH_P4_7(R, lat_l2b, 2, LOGISTIC)       \
  FMH_P8_15(R, lat_l3a, 1, LOGISTIC) FMH_P8_15(R, lat_l3b, 2, LOGISTIC)
#include "mh_parts.hpp"

#if FMH_HAS_LOOKUPS
namespace fmh {
const void* k_lat(int p, int kind) { return find_kernel(kind, LINREG, p); }
const void* k_lat_logit(int p, int kind) { return find_kernel(kind, LOGISTIC, p); }
size_t k_lat_logit_lds() { return lat_logit_lds_bytes(); }
}  // namespace fmh
#endif
