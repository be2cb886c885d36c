#!/usr/bin/env python3
"""Record tests/golden/gemv_bits.json: the SHA-256 of the output bytes of every case of tests/test_gemv_bits_pinned.py, computed by the library
as built, and in the header the SHA-256 of the two sources that library was built from.  Run on the MI355X box BEFORE a change of the decode
GEMV that must keep its bits; the test then holds the change to them.  The case list, the inputs and the digest are the test module's.

    python tools/record_gemv_bits.py [--out tests/golden/gemv_bits.json]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemv_bits_pinned as T  # noqa: E402
from ntransformer_amd import ops  # noqa: E402

SOURCES = ["ntransformer_amd/csrc/gemv.hip", "ntransformer_amd/csrc/gemv_core.hip.h"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN_FILE)
    a = ap.parse_args()
    src = {}
    for s in SOURCES:
        with open(os.path.join(ROOT, s), "rb") as f:
            src[s] = hashlib.sha256(f.read()).hexdigest()
    ops.init(0)
    cases = {}
    for c in T.CASES:
        outs = T.run_case(c)
        if not all(np.isfinite(y).all() for y in T.written(c, outs)):
            sys.exit("%s: an output that is not finite -- nothing recorded" % c["id"])
        cases[c["id"]] = T.digest(outs)
    with open(a.out, "w") as f:
        json.dump({"recorded_from": src, "cases": cases}, f, indent=0)
        f.write("\n")
    print("%d cases -> %s (%d bytes)" % (len(cases), a.out, os.path.getsize(a.out)))
    for s, h in src.items():
        print(h, s)


if __name__ == "__main__":
    main()
