"""Writes tests/golden/diag_bits.json, the fixture that holds fmcmc_summary_dev, fmcmc_heidel_dev, fmcmc_chain_order_dev and
fmcmc_raftery_dev to the bits of an earlier commit: checksums of what every case of tests/diag_dev.py compares.  The committed
file was written on an MI355X by the library built from the commit BEFORE csrc/diag_common.hpp took over what summary.hip and
raftery.hip each had a copy of (FMCMC_AMD_LIB=<that build> python tests/golden/make_diag_bits.py [--to FILE]).  A mismatch
means that a change altered an operation or the order of a sum: mend the code.  Regenerating the file with the current library
only restates what the library does now."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    from diag_dev import CASES, run_case
    from gelman_dev import bit_checksums
    out = {key: {name: bit_checksums(v) for name, v in run_case(key).items()} for key in CASES}
    with open(sys.argv[-1] if "--to" in sys.argv[1:-1] else os.path.join(HERE, "diag_bits.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d cases written" % len(out))
