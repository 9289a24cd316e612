"""Writes tests/golden/gelman_narrow_bits.json: checksums of the bits fmcmc_gelman_partial_dev leaves in `work` and `partial`
at p = 64 and p = 50 (inputs and checksums: tests/test_gpu_gelman_wide.py, narrow_case / bit_checksums).

The committed file was written on an MI355X by the library built from the commit BEFORE the reduction learned p > 64
(FMCMC_AMD_LIB=<that build> python tests/golden/make_gelman_narrow_bits.py), so that the test holds the p <= 64 path to the
bits it gave then.  Regenerating it with the current library only restates what the library does now."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    from test_gpu_gelman_wide import bit_checksums, narrow_case
    out = {}
    for p in (64, 50):
        work, part = narrow_case(p)
        out["p%d" % p] = {"work": bit_checksums(work), "partial": bit_checksums(part)}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "gelman_narrow_bits.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, sort_keys=True))
