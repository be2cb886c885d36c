#!/usr/bin/env python3
"""The packed prompt pass against the slot-by-slot prefill, on the same box, the same build and the same loaded model (--synthetic 8b:Q8_0,
"sequences" = 16, F16 KV cache):
  packed  -- Engine.forward_batch: B prompts of L tokens, prompt i into slot i, ONE pass over the weights (nt_engine_forward_batch);
  loop    -- B calls of Engine.seq_forward, one pass over the weights per prompt (what generate_batch does without "batch_prefill").
For every B x L the two are alternated --repeats times (after one untimed run of each: first-use allocations, the launch forms' first run) and the
MEDIAN of each is reported with every run listed, prompt tokens / s of both and the ratio loop / packed (> 1: the packed pass is faster).  Both calls
download their logits ([B][vocab] at once / [vocab] per call) and synchronise once per call; the clock is the host's, around the call(s).
The MIXED step: 15 decoding sequences at position 512 plus one 256-token prompt chunk (slot 15, positions 256 .. 511) in one forward_batch, against what
a caller has without it: one decode_batch of the 15 rows followed by one seq_forward of the chunk.  (No claim is made for one-token segments at long
contexts: the prompt attention kernel spends a 64-query tile on one query, and each one-token segment is a launch of its own.)

Every case runs in a child process of its own under its own `timeout`; the driver stops at the first child that does not end clean, and writes
what it has to --out.

  python tools/batch_prefill_bench.py --out profiles/batch_prefill.txt
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ["16x16", "16x64", "4x256", "16x256", "mixed"]
CTX = 4096          # 16 x 256 rows fill it exactly


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def child(a):
    import numpy as np
    from ntransformer_amd import engine as E, ops
    eng = E.Engine()
    eng.set_option("sequences", 16)
    spec = E.synth_spec(a.model, a.mix, layers=a.layers) if a.layers else E.synth_spec(a.model, a.mix)
    eng.load_synthetic(spec, CTX)
    r = np.random.Generator(np.random.Philox(key=[20261019, 31]))
    ids = lambda n: [1] + [int(t) for t in r.integers(2, min(eng.vocab_size, 32000), n - 1)]

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    cell = lambda ms: "%8.3f ms (%s)" % (median(ms), " / ".join("%.3f" % x for x in ms))
    if a.case == "mixed":
        slots, toks, chunk = list(range(15)), [2 + 3 * b for b in range(15)], ids(256)
        packed = lambda: eng.forward_batch(slots + [15], [[t] for t in toks] + [chunk], [512] * 15 + [256])
        apart = lambda: (eng.decode_batch(slots, toks, [512] * 15), eng.seq_forward(15, chunk, 256))
        packed(); apart()
        tp, ta = [], []
        for _ in range(a.repeats):
            tp.append(timed(packed)); ta.append(timed(apart))
        print("mixed: 15 decode rows at position 512 + one 256-token chunk | forward_batch %s | decode_batch + seq_forward %s | ratio %.3f" %
              (cell(tp), cell(ta), median(ta) / median(tp)))
    else:
        B, L = (int(x) for x in a.case.split("x"))
        ps = [ids(L) for _ in range(B)]
        slots = list(range(B))
        packed = lambda: eng.forward_batch(slots, ps, [0] * B)
        loop = lambda: [eng.seq_forward(s, p, 0) for s, p in zip(slots, ps)]
        packed(); loop()
        tp, tl = [], []
        for _ in range(a.repeats):
            tp.append(timed(packed)); tl.append(timed(loop))
        n = B * L
        print("%2d x %3d = %4d rows | forward_batch %s %9.0f tok/s | %2d x seq_forward %s %9.0f tok/s | ratio %.3f" %
              (B, L, n, cell(tp), n / (median(tp) / 1e3), B, cell(tl), n / (median(tl) / 1e3), median(tl) / median(tp)))
    print("# shader clock behind the runs: %.0f MHz" % ops.sclk_mhz(), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="8b")
    ap.add_argument("--mix", default="Q8_0")
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the preset (a quick look)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--case", help="(the child's) one of " + ", ".join(CASES))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--timeout", type=int, default=170, help="seconds per case (the model is loaded by every case)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_prefill.txt"))
    a = ap.parse_args()
    if a.case:
        return child(a)
    lines = ["# tools/batch_prefill_bench.py: --synthetic %s:%s%s, sequences 16, context %d, F16 KV cache; host clock around the call(s), median of %d "
             "alternated runs (every run listed); ratio = slot-by-slot / packed" % (a.model, a.mix, " (%d layers)" % a.layers if a.layers else "", CTX, a.repeats)]
    rc = 0
    for case in a.cases.split(","):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case, "--model", a.model, "--mix", a.mix,
               "--layers", str(a.layers), "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        kept = [l for l in p.stdout.splitlines() if " | " in l or l.startswith("# shader clock")]
        lines += kept
        for l in kept: print(l, flush=True)
        if p.returncode != 0:          # a fault, an abort or the time limit: nothing more is started on the GPU
            rc = p.returncode
            lines.append("# case %s ended with status %d: stopped here" % (case, rc))
            sys.stderr.write(p.stderr[-2000:])
            break
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
