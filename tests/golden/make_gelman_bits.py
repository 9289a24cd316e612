"""Writes the fixtures that hold fmcmc_gelman_partial_dev to the bits of an earlier commit: checksums of what it leaves in `work`
and `partial` (inputs and checksums: tests/gelman_dev.py).  Each committed file was written on an MI355X by the library built
from the commit BEFORE the change it guards (FMCMC_AMD_LIB=<that build> python tests/golden/make_gelman_bits.py [narrow] [--to FILE]);
regenerating one with the current library only restates what the library does now.
  gelman_narrow_bits.json (`narrow`): p = 64 and p = 50 (narrow_case), by the commit before the reduction learned p > 64;
  gelman_bits.json: every shape of BITS_SHAPES (bits_case), by the commit before gelman_chain_mfma (p <= 64) and
                    gelman_pair_mfma (above) became the one kernel gelman_cov_mfma."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    from gelman_dev import BITS_SHAPES, bit_checksums, bits_case, narrow_case
    if sys.argv[1:2] == ["narrow"]:
        name, cases = "gelman_narrow_bits.json", {"p%d" % p: narrow_case(p) for p in (64, 50)}
    else:
        name, cases = "gelman_bits.json", {"p%d_N%d" % s: bits_case(*s) for s in BITS_SHAPES}
    out = {key: {"work": bit_checksums(w), "partial": bit_checksums(pt)} for key, (w, pt) in cases.items()}
    with open(sys.argv[-1] if "--to" in sys.argv[1:-1] else os.path.join(HERE, name), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, sort_keys=True))
