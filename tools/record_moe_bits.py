#!/usr/bin/env python3
"""Record tests/golden/moe_pass_bits.json: one SHA-256 per (model, pass) of tests/moe_bits.py over the four mixture-of-experts models of tests/moe_ref.py,
computed by the library as built (or the one NTK_LIB_PATH names), with the commit that library was built from in the header.  Run on the MI355X box on the
build BEFORE the grouped expert GEMM (or, later, with moe_gemm = 0, which must be the same thing -- tests/test_engine_moe_gemm_gpu.py holds it to that).
Every pass runs twice, on two engines: a pass whose digests differ is not reproducible and is refused, not pinned.

    NTK_LIB_PATH=<parent build>/libntransformer_hip.so python tools/record_moe_bits.py --commit <parent hash> [--out tests/golden/moe_pass_bits.json]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import moe_bits as B  # noqa: E402
from ntransformer_amd import _lib  # noqa: E402
from ntransformer_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=B.GOLDEN_FILE)
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--option", action="append", default=[], help="key=value engine options set before the load (e.g. moe_gemm=0 on a later build)")
    a = ap.parse_args()
    cases = {}
    with tempfile.TemporaryDirectory() as root:
        dirs = B.TmpDirs(root)
        for name in B.NAMES:
            path = B.model_path(name, dirs)
            runs = []
            for _ in range(2):
                e = E.Engine()
                for kv in a.option:
                    e.set_option(*kv.split("=", 1))
                e.load(path, 1024)
                runs.append({k: B.digest(v) for k, v in B.run_passes(e).items()})
                e.close()
            assert runs[0] == runs[1], (name, "not reproducible", runs)
            for k, v in runs[0].items():
                cases["%s/%s" % (name, k)] = v
    with open(a.out, "w") as f:
        json.dump({"recorded_from": a.commit, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d cases from %s (%s) -> %s (%d bytes)" % (len(cases), a.commit, _lib.LIB_PATH, a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
