#!/usr/bin/env python3
"""Record tests/golden/gemm_f16_bits.json: the SHA-256 of the output bytes of every case of tests/test_gemm_f16_bits_pinned.py, computed by the
library as built, and in the header the SHA-256 of the prompt GEMM's sources that library was built from.  Run on the MI355X box BEFORE a change of
the prompt GEMM that must keep its bits; the test then holds the change to them.  The case list, the inputs and the digest are the test module's.

    python tools/record_gemm_bits.py [--out tests/golden/gemm_f16_bits.json]
"""
import argparse
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gemm_f16_bits_pinned as T  # noqa: E402
from ntransformer_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN_FILE)
    a = ap.parse_args()
    src = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "ntransformer_amd", "csrc", "gemm_f16*"))):
        with open(path, "rb") as f:
            src[os.path.relpath(path, ROOT)] = hashlib.sha256(f.read()).hexdigest()
    ops.init(0)
    cases = {}
    for c in T.CASES:
        outs = T.run_case(c)
        T.check(c, outs)
        cases[c["id"]] = T.digest(outs)
    with open(a.out, "w") as f:
        json.dump({"recorded_from": src, "cases": cases}, f, indent=0)
        f.write("\n")
    print("%d cases -> %s (%d bytes)" % (len(cases), a.out, os.path.getsize(a.out)))
    for s, h in src.items():
        print(h, s)


if __name__ == "__main__":
    main()
