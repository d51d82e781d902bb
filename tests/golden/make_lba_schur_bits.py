"""Writes tests/golden/lba_schur_bits.json: SHA-256 digests of Hs, bs and the pose part of b as k_schur leaves them (tap
aos2_debug_lba_assemble_device, stage 0, every window alone) for the windows of tests/lba_schur_cases.py.  Needs the built library and
a device.  The file pins the BITS of the reduced system: regenerate it only with a build whose sums are meant to differ, and say so.
    python tests/golden/make_lba_schur_bits.py [output path]"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lba_schur_cases as SC  # noqa: E402


def digests(ba, case):
    g = ba.debug_assemble([case["win"]], layout="slots", stage=0)[0]
    return {k: hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest() for k, a in SC.digest_arrays(g).items()}


def main():
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ba = pkg.LocalBA()
    out = {c["name"]: digests(ba, c) for c in SC.cases()}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lba_schur_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(out), "windows")


if __name__ == "__main__":
    main()
