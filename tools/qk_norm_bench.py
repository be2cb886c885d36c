#!/usr/bin/env python3
"""Per-launch cost of ntk_qk_norm (csrc/qk_norm.hip) against the code it stands in for: two ntk_rmsnorm launches, one over the q heads and one over the k
heads, with batch = rows x heads and hidden = head_dim.  Both forms run in this process on the same buffers, alternated; a round enqueues `--launches`
back-to-back launches of a form between two synchronisations and divides; a repeat is the median of `--rounds` rounds; `--repeats` repeats give each
form's median and the run-to-run spread of those medians (max - min).  The new launch must not be slower than the two-launch form beyond that spread.
usage: python tools/qk_norm_bench.py [--shapes 1x32x8x128,1024x32x8x128] [--out profiles/qk_norm.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntransformer_amd import ops  # noqa: E402
from ntransformer_amd.ops import DeviceBuffer as DB  # noqa: E402

EPS = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x32x8x128,1024x32x8x128", help="rows x heads x kv_heads x head_dim, comma separated")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    ops.init(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for shape in a.shapes.split(","):
        rows, nh, nkv, hd = [int(v) for v in shape.split("x")]
        r = np.random.Generator(np.random.Philox(key=[20261022, rows + hd]))
        q = DB.from_numpy(r.standard_normal(rows * nh * hd).astype(np.float32))
        k = DB.from_numpy(r.standard_normal(rows * nkv * hd).astype(np.float32))
        wq = DB.from_numpy((1 + 0.5 * r.uniform(-1, 1, hd)).astype(np.float32))
        wk = DB.from_numpy((1 + 0.5 * r.uniform(-1, 1, hd)).astype(np.float32))
        n = max(10, a.launches // (8 if rows >= 256 else 1))

        def one():
            ops.qk_norm(q, k, wq, wk, rows, nh, nkv, hd, EPS)

        def two():
            ops.launch_rmsnorm(q, q, wq, rows * nh, hd, EPS)
            ops.launch_rmsnorm(k, k, wk, rows * nkv, hd, EPS)

        def round_us(fn):
            ops.synchronize()
            t0 = time.perf_counter()
            for _ in range(n): fn()
            ops.synchronize()
            return (time.perf_counter() - t0) / n * 1e6

        for fn in (one, two): round_us(fn)          # warm-up: code objects, clocks
        meds = {"one": [], "two": []}
        for _ in range(a.repeats):
            ts = {"one": [], "two": []}
            for _ in range(a.rounds):
                ts["one"].append(round_us(one))
                ts["two"].append(round_us(two))
            for key in ts: meds[key].append(float(np.median(ts[key])))
        m1, m2 = float(np.median(meds["one"])), float(np.median(meds["two"]))
        spread = max(max(v) - min(v) for v in meds.values())
        mb = 2.0 * 4 * rows * (nh + nkv) * hd / 1e6
        say("(%d, %d, %d, %d): ntk_qk_norm %.2f us [%s]   two ntk_rmsnorm launches %.2f us [%s]   spread of the medians %.2f us   %s" %
            (rows, nh, nkv, hd, m1, " ".join("%.2f" % v for v in meds["one"]), m2, " ".join("%.2f" % v for v in meds["two"]), spread,
             "not slower" if m1 <= m2 + spread else "SLOWER than the two-launch form beyond the spread"))
        say("    %d back-to-back launches per round, median of %d rounds per repeat, %d repeats; %.2f MB read + written per launch: %.0f GB/s in one launch, %.0f GB/s in two" %
            (n, a.rounds, a.repeats, mb, mb / m1 * 1e3, mb / m2 * 1e3))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
