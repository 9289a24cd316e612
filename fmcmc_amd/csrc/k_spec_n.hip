// k_spec_n.hip -- mh_sweep_spec<P, reg_slots(P), KIND> (mh_spec.hpp) for the normal / uniform kernels (KIND 1, 2) at p = 1, 3: the VALU
// partner of mh_sweep_mfma (knob mfma=0), a second implementation of the same sweep for the parity tests
#include "mh_tu.hpp"
#include "mh_spec.hpp"

namespace fmh {
FMH_HIDDEN const void* k_spec_normal(int p, int kind) {
#define SPEC_N(PV) ((kind == 1) ? (const void*)mh_sweep_spec<PV, reg_slots(PV), 1> : (const void*)mh_sweep_spec<PV, reg_slots(PV), 2>)
  switch (p) {
    case 1: return SPEC_N(1);
    case 3: return SPEC_N(3);
    default: return nullptr;
  }
#undef SPEC_N
}
}  // namespace fmh
