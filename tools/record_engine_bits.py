#!/usr/bin/env python3
"""Record tests/golden/engine_pass_bits.json: the SHA-256 of everything each case of tests/test_engine_pass_bits_pinned.py returns, computed by the
library as built (or the one NTK_LIB_PATH names), with the commit that library was built from in the header.  Run on the MI355X box on the PARENT of a
change that must keep the engine's passes bit for bit; the test then holds the change to them.  The case list, the calls and the digest are the test
module's.  Record twice, in separate processes (--out to two files): a case whose digests differ is not reproducible on the parent itself and must
be replaced, not pinned.

    NTK_LIB_PATH=<parent build>/libntransformer_hip.so python tools/record_engine_bits.py --commit <parent hash> [--out tests/golden/engine_pass_bits.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_engine_pass_bits_pinned as T  # noqa: E402
from ntransformer_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN_FILE)
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    a = ap.parse_args()
    cases = {}
    with tempfile.TemporaryDirectory() as root:
        for c in T.CASES:
            outs = T.run_case(c, root)
            T.check(c, outs)
            cases[c["id"]] = T.digest(outs)
    with open(a.out, "w") as f:
        json.dump({"recorded_from": a.commit, "cases": cases}, f, indent=0)
        f.write("\n")
    print("%d cases from %s (%s) -> %s (%d bytes)" % (len(cases), a.commit, _lib.LIB_PATH, a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
