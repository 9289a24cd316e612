// k_mfma.hip -- mh_sweep_mfma<KIND, NG, NS, false, BIG, EXT> (mh_mfma.hpp): kernel_normal / kernel_unif (KIND 1) and the reflective
// kernels (KIND 2) on NG operand groups; BIG: more than 4 GiB of samples.  Compiled once per part (mh_parts.hpp).
#define FMH_PARTS(X) X(mfma1) X(mfma2) X(mfma_ext)
#define FMH_LOOKUPS_mfma1 1
#include "mh_tu.hpp"
#include "mh_mfma.hpp"

#define FMH_KERNEL(KIND, NG, BIG, EXT, NS) mh_sweep_mfma<KIND, NG, NS, false, BIG, EXT>
#define MF_NS10(R, ...) FMH_P1_7(R, __VA_ARGS__) R(__VA_ARGS__, 8) R(__VA_ARGS__, 9) R(__VA_ARGS__, 10)
#define MF_NS20(R, ...) MF_NS10(R, __VA_ARGS__) R(__VA_ARGS__, 11) FMH_P12_14(R, __VA_ARGS__) R(__VA_ARGS__, 15) R(__VA_ARGS__, 16) R(__VA_ARGS__, 17) R(__VA_ARGS__, 18) R(__VA_ARGS__, 19) R(__VA_ARGS__, 20)
// the whole data set in operand registers: every slot count one group (1 .. 20) or two (1 .. 10) can hold
#define MF_RESIDENT(R, PART, KIND) MF_NS20(R, PART, KIND, 1, false, false) MF_NS20(R, PART, KIND, 1, true, false) MF_NS10(R, PART, KIND, 2, false, false) MF_NS10(R, PART, KIND, 2, true, false)
// EXT: NS observation slots in operand registers, the rest streamed from an operand-order copy every step (any n; 8 .. 15 covariates as
// three / four operand groups)
#define MF_STREAMED(R, KIND, BIG) R(mfma_ext, KIND, 1, BIG, true, 16) R(mfma_ext, KIND, 2, BIG, true, 8) R(mfma_ext, KIND, 3, BIG, true, 4) R(mfma_ext, KIND, 3, BIG, true, 1) R(mfma_ext, KIND, 4, BIG, true, 2) R(mfma_ext, KIND, 4, BIG, true, 1)
// rows: part, KIND, NG, BIG, EXT, NS
#define FMH_TABLE(R) MF_RESIDENT(R, mfma1, 1) MF_RESIDENT(R, mfma2, 2) MF_STREAMED(R, 1, false) MF_STREAMED(R, 1, true) MF_STREAMED(R, 2, false) MF_STREAMED(R, 2, true)
#include "mh_parts.hpp"

#if FMH_HAS_LOOKUPS
namespace fmh {
const void* k_mfma(int kv, int ng, int ns, int big) { return find_kernel(kv, ng, big != 0, false, ns); }
const void* k_mfma_ext(int kv, int ng, int nsres, int big) { return find_kernel(kv, ng, big != 0, true, nsres); }
}  // namespace fmh
#endif
