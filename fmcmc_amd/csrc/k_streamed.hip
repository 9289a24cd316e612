// k_streamed.hip -- mh_sweep_kernel<CW, P, OPT, KIND, FAM, MINB, FEDONLY> (mh_streamed.hpp): the chain-sharded kernel every other form
// steps down to, and its one-family forms.  Compiled once per part (mh_parts.hpp).
#define FMH_PARTS(X) X(general) X(wide) X(logit0) X(logit1) X(logit2)
#define FMH_LOOKUPS_general 1
#include "mh_tu.hpp"
#include "mh_streamed.hpp"

#define LINREG FMCMC_FAM_GAUSSIAN_LINREG
#define LOGISTIC FMCMC_FAM_LOGISTIC
#define FMH_KERNEL(CW, P, OPT, FAM, MINB, FEDONLY, KIND) mh_sweep_kernel<CW, P, OPT, KIND, FAM, MINB, FEDONLY>
#define ST_KIND124(R, ...) R(__VA_ARGS__, 1) R(__VA_ARGS__, 2) R(__VA_ARGS__, 4)
#define ST_KIND1_4(R, ...) ST_KIND124(R, __VA_ARGS__) R(__VA_ARGS__, 3)
// wide Gaussian linear models, one family and one proposal kernel compiled in: OPT = 0 the chain-sharded loop, OPT = 2 | 4 the
// observation-sharded evaluation (canonical lanes per workgroup, cooperative)
#define ST_WIDE(R, CW) ST_KIND124(R, wide, CW, -1, 0, LINREG, 1, false) ST_KIND124(R, wide, CW, -1, 2, LINREG, 1, false) ST_KIND124(R, wide, CW, -1, 4, LINREG, 1, false)
// logistic only, g table in LDS, cw = 1, 2, 4
#define ST_LOGIT(R, PART, OPT, FEDONLY) ST_KIND1_4(R, PART, 1, -1, OPT, LOGISTIC, 1, FEDONLY) ST_KIND1_4(R, PART, 2, -1, OPT, LOGISTIC, 1, FEDONLY) ST_KIND1_4(R, PART, 4, -1, OPT, LOGISTIC, 1, FEDONLY)
// rows: part, CW, P, OPT, FAM, MINB, FEDONLY, KIND
#define FMH_TABLE(R)                                                                                                               \
  /* every family / proposal kernel / scheme (FAM 0, KIND 0); the two register-resident shapes (p, slots) = (1, 4), (3, 20); */    \
  R(general, 1, -1, 0, 0, 1, false, 0) R(general, 2, -1, 0, 0, 1, false, 0) R(general, 4, -1, 0, 0, 1, false, 0) R(general, 8, -1, 0, 0, 1, false, 0) \
  ST_KIND1_4(R, general, 4, 1, 4, 0, 1, false) ST_KIND1_4(R, general, 4, 3, 20, 0, 1, false)                                       \
  /* the long-data form of the linear model (one chain per workgroup, OPT = 2) has kernel_adapt as well; */                        \
  ST_WIDE(R, 1) ST_WIDE(R, 2) R(wide, 1, -1, 2, LINREG, 1, false, 3)                                                               \
  /* the chain-sharded loop (logit_partials); the observation-sharded form (logit_shard) and the long-data form with variates      \
     drawn in the kernel (streams beyond 1 GiB, single-parameter schemes); the same from a materialised stream only (config C5) */ \
  ST_LOGIT(R, logit0, 0, false) ST_LOGIT(R, logit1, 2, false) ST_LOGIT(R, logit2, 2, true)
#include "mh_parts.hpp"

#if FMH_HAS_LOOKUPS
namespace fmh {
const void* k_general(int cw) { return find_kernel(cw, -1, 0, 0, 1, false, 0); }
// (a kind other than 1 .. 3 takes kernel_ram's instantiation)
const void* k_resident(int p, int kind) { return find_kernel(4, p, p == 1 ? 4 : 20, 0, 1, false, kind >= 1 && kind <= 3 ? kind : 4); }
const void* k_wide(int cw, int lpw, int kind) { return find_kernel(cw, -1, lpw, LINREG, 1, false, kind); }
// sharded = 0 | 1 | 2: the chain-sharded loop | observation-sharded | the same, variates from a materialised stream only
const void* k_logit(int cw, int sharded, int kind) { return find_kernel(cw, -1, sharded ? 2 : 0, LOGISTIC, 1, sharded == 2, kind); }
}  // namespace fmh
#endif
