#!/usr/bin/env python3
"""kv_cache=q8_0 against kv_cache=f16, end to end, on synthetic models (one copy of the weights, two sequences: nt_engine_load_shared).

  speed    8B Q8_0: greedy decode tokens/s (nt_engine_decode_greedy_steps, the loop bench.py times for its ctx workloads) at position 128 and
           behind 3900- and 32768-token prompts, both modes alternating, 3 timed runs of --steps tokens each after a warm-up run.
  quality  8B Q8_0, 8B Q4_K_M and the massive-activation model of tests/test_parity_depth.py (8B width, Q4_K_M, 6 layers, five RMSNorm channels
           x 1000 / x 4000): max and RMS over the vocabulary of (logit_q8 - logit_f16) / RMS(logit_f16) after prompts of 64 / 1024 / 3900 random
           tokens, and the agreement of the two greedy streams over 256 tokens behind the 1024-token prompt.

usage: python tools/kv_q8_eval.py speed|quality [--steps 64]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntransformer_amd import engine as E  # noqa: E402
from ntransformer_amd import ops  # noqa: E402


def pair(load, ctx):
    """(f16 engine, q8_0 engine) over one copy of the weights"""
    f = E.Engine()
    f.set_option("synth_threads", 16)
    load(f, ctx)
    q = E.Engine()
    q.set_option("kv_cache", "q8_0")
    q.load_shared(f, ctx)
    return f, q


def prefill(e, toks):
    lg = None
    for s in range(0, len(toks), 1024):
        lg = e.forward(toks[s:s + 1024], s)
    return lg


def speed(steps):
    spec = E.synth_spec("8b", "Q8_0")
    f, q = pair(lambda e, ctx: e.load_synthetic(spec, ctx), 32768 + 4 * steps + 64)
    r = np.random.default_rng(1)
    print("8B Q8_0 synthetic, greedy decode tokens/s (3 runs of %d tokens, median; all runs listed)" % steps)
    for n_prompt in (128, 3900, 32768):
        toks = [int(t) for t in r.integers(0, 128000, n_prompt)]
        row = {}
        for name, e in (("f16", f), ("q8_0", q)):
            t0 = time.perf_counter()
            lg = prefill(e, toks)
            row[name + "_prefill_s"] = time.perf_counter() - t0
            row[name + "_tok"] = int(np.argmax(lg))
        runs = {"f16": [], "q8_0": []}
        for rep in range(4):                       # (run 0 warms up: graph capture)
            for name, e in (("f16", f), ("q8_0", q)):
                t0 = time.perf_counter()
                e.decode_greedy_steps(row[name + "_tok"], n_prompt, steps)
                dt = time.perf_counter() - t0
                if rep:
                    runs[name].append(steps / dt)
        sclk = ops.sclk_mhz()
        for name in ("f16", "q8_0"):
            print("prompt %6d  kv_cache=%-5s %8.1f tok/s  (runs %s; prompt pass %.2f s; bytes/token %.3f GB)"
                  % (n_prompt, name, float(np.median(runs[name])), " / ".join("%.1f" % x for x in runs[name]), row[name + "_prefill_s"],
                     (f if name == "f16" else q).bytes_per_token(n_prompt) / 1e9), flush=True)
        print("prompt %6d  q8_0 / f16 = %.3f   sclk right after: %.0f MHz" % (n_prompt, np.median(runs["q8_0"]) / np.median(runs["f16"]), sclk), flush=True)
    print("KV cache resident: f16 %.2f GB, q8_0 %.2f GB (incl. the one-layer F16 image)" % (f.kv_cache_bytes() / 1e9, q.kv_cache_bytes() / 1e9))
    q.close(); f.close()


def massive_path():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_parity_depth import _scale_norm_channels
    path = os.path.join(tempfile.mkdtemp(prefix="kvq8_"), "massive.gguf")
    E.synth_write_gguf(path, E.synth_spec("8b", "Q4_K_M", layers=6), 16)
    _scale_norm_channels(path, {5: 1000.0, 1033: 1000.0, 2500: 1000.0, 4000: 1000.0, 3333: 4000.0})
    return path


def quality():
    models = [("8B Q8_0", lambda e, ctx: e.load_synthetic(E.synth_spec("8b", "Q8_0"), ctx)),
              ("8B Q4_K_M", lambda e, ctx: e.load_synthetic(E.synth_spec("8b", "Q4_K_M"), ctx)),
              ("massive activations (8B width, Q4_K_M, 6 layers)", None)]
    r = np.random.default_rng(2)
    prompts = {n: [int(t) for t in r.integers(0, 128000, n)] for n in (64, 1024, 3900)}
    print("%-50s %7s %12s %12s %10s" % ("model", "prompt", "max d/RMS", "RMS d/RMS", "RMS logit"))
    for name, load in models:
        if load is None:
            path = massive_path()
            load = lambda e, ctx, path=path: e.load(path, ctx)
        f, q = pair(load, 4352)
        for n, toks in prompts.items():
            a, b = prefill(f, toks).astype(np.float64), prefill(q, toks).astype(np.float64)
            rms = float(np.sqrt((a * a).mean()))
            d = (b - a) / rms
            print("%-50s %7d %12.3e %12.3e %10.3f   argmax %s" % (name, n, float(np.abs(d).max()), float(np.sqrt((d * d).mean())), rms,
                                                                   "same" if int(np.argmax(a)) == int(np.argmax(b)) else "DIFFERENT"), flush=True)
        toks = prompts[1024]
        first_tok = int(np.argmax(prefill(f, toks)))   # the same first token for both: only the caches differ
        ta = f.decode_greedy_steps(first_tok, 1024, 256)
        prefill(q, toks)
        tb = q.decode_greedy_steps(first_tok, 1024, 256)
        same = [x == y for x, y in zip(ta, tb)]
        first = same.index(False) if False in same else 256
        print("%-50s greedy streams behind 1024 tokens: %d of 256 equal, first difference at step %s" % (name, sum(same), first if first < 256 else "none"), flush=True)
        q.close(); f.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("speed", "quality"))
    ap.add_argument("--steps", type=int, default=64)
    a = ap.parse_args()
    ops.init(0)
    speed(a.steps) if a.what == "speed" else quality()
