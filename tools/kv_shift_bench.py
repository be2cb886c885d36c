#!/usr/bin/env python3
"""One context shift (ntk_kv_shift / ntk_kv_shift_q8, csrc/kv_ops.hip) at the Llama-3.1 8B cache geometry -- 32 layers, 8 KV heads x 128 -- in both cache
formats: the generate loop's shift (keep 1, discard half) at 32 768 and 131 072 positions, and the small-step corner (discard 1 / 64 under a full
context), where the one-launch form has little parallelism.

Timing: HIP events on the compute stream around ONE call, after a warm-up, median of several.  Bytes = rows moved x row bytes x layers x 2 sides, read
once and written once (F16 row: 2 048 bytes; Q8_0 row: 1 088).  Printed beside the recorded 6.29 TB/s copy ceiling of the chip (float4 copy) and -- unless
--no-engine -- beside one greedy decode step of the 8B Q8_0 model at the full context and at the position the shift leaves (wall clock over a run of
decode_greedy_steps, the engine's own loop).

usage: python tools/kv_shift_bench.py [--out profiles/kv_shift.txt] [--contexts 32768,131072] [--layers 32] [--no-engine] [--no-corner]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntransformer_amd import _lib, kv_ops, kv_q8, ops  # noqa: E402
from ntransformer_amd import engine as E  # noqa: E402
from ntransformer_amd.ops import DeviceBuffer as DB  # noqa: E402

NKV, HD, THETA = 8, 128, 500000.0
CEILING_TBS = 6.29


def timed(L, stream, ev0, ev1, call, warm=2, reps=7):
    for _ in range(warm):
        call()
    ops.synchronize(stream)
    ms = []
    for _ in range(reps):
        L.ntk_event_record(ev0, stream)
        call()
        L.ntk_event_record(ev1, stream)
        L.ntk_event_synchronize(ev1)
        t = C.c_float()
        _lib.check(L.ntk_event_elapsed_ms(ev0, ev1, C.byref(t)), "event_elapsed")
        ms.append(float(t.value))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--contexts", default="32768,131072")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-engine", action="store_true", help="skip the decode-step comparison (no model is loaded)")
    ap.add_argument("--no-corner", action="store_true", help="skip the small-step cases")
    a = ap.parse_args()
    contexts = [int(c) for c in a.contexts.split(",")]
    nl, per = a.layers, NKV * HD
    ops.init(0)
    L = _lib.lib()
    stream = L.ntk_stream(0)
    ev0, ev1 = L.ntk_event_create(), L.ntk_event_create()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    name = C.create_string_buffer(256)
    L.ntk_device_name(name, 256)
    say("# tools/kv_shift_bench.py: one context shift, 8B cache geometry (%d layers, %d KV heads x %d); device: %s" % (nl, NKV, HD, name.value.decode()))
    say("# HIP events around one call, 2 warm-up calls, median (min .. max) of 7; GB/s of bytes read + written; copy ceiling %.2f TB/s" % CEILING_TBS)
    rng = np.random.default_rng(0)
    freq = DB.from_numpy(kv_ops.pair_freqs(HD, THETA))
    results = {}
    for ctx in contexts:
        # one random layer image per format, copied into every layer and side (distinct addresses; the values do not matter to the timing)
        h16 = rng.standard_normal(ctx * per, dtype=np.float32).astype(np.float16)
        k16, v16 = DB(nl * ctx * per * 2), DB(nl * ctx * per * 2)
        for l in range(nl):
            k16.upload(h16, l * ctx * per * 2)
            v16.upload(h16, l * ctx * per * 2)
        del h16
        lb = kv_q8.cache_bytes(ctx, NKV, HD)
        h8 = np.zeros(lb, np.uint8)
        h8[:ctx * per] = rng.integers(-127, 128, ctx * per).astype(np.int8).view(np.uint8)
        h8[ctx * per:ctx * per + ctx * (per // 32) * 2] = (rng.uniform(0.5, 1.4, ctx * (per // 32)) / 73.3).astype(np.float16).view(np.uint8)
        k8, v8 = DB(nl * lb), DB(nl * lb)
        for l in range(nl):
            k8.upload(h8, l * lb)
            v8.upload(h8, l * lb)
        del h8
        keep = 1
        cases = [("generate loop: keep 1, discard half", keep, E.context_shift_discard(ctx, keep))]
        if not a.no_corner:
            cases += [("corner: keep 1, discard 64", keep, 64), ("corner: keep 1, discard 1", keep, 1)]
        say()
        say("## context %d positions (n_past = %d)" % (ctx, ctx))
        for what, kp, discard in cases:
            src0, n = kp + discard, ctx - kp - discard
            for kind, row_bytes in (("f16", per * 2), ("q8_0", per * 17 // 16)):
                if kind == "f16":
                    call = lambda: kv_ops.kv_shift(k16, v16, nl, ctx, NKV, HD, src0, kp, n, inv_freq=freq, theta_base=THETA, stream=stream)
                else:
                    call = lambda: kv_ops.kv_shift_q8(k8, v8, nl, ctx, NKV, HD, src0, kp, n, inv_freq=freq, theta_base=THETA, stream=stream)
                reps = 3 if discard < 64 else 7
                med, lo, hi = timed(L, stream, ev0, ev1, call, warm=1 if discard < 64 else 2, reps=reps)
                gb = 2.0 * n * row_bytes * nl * 2 / 1e9
                say("%-38s %-5s rows %6d  %9.3f ms (%.3f .. %.3f, %d calls)  %7.1f GB moved  %7.1f GB/s = %.2f of the ceiling  [1 launch, %d chains]" %
                    (what, kind, n, med, lo, hi, reps, gb, gb / (med / 1e3), gb / (med / 1e3) / (CEILING_TBS * 1e3), min(discard, n)))
                results[(ctx, kind, discard)] = med
        for b in (k16, v16, k8, v8):
            b.free()
    if not a.no_engine:
        say()
        say("## one greedy decode step of 8B Q8_0 (fused, graphs; wall clock over 16 steps of decode_greedy_steps behind a 4-step warm-up) beside the shift")
        for kind in ("f16", "q8_0"):
            e = E.Engine()
            e.set_option("kv_cache", kind)
            e.load_synthetic(E.synth_spec("8b", "Q8_0"), max(contexts))
            for ctx in contexts:
                discard = E.context_shift_discard(ctx, 1)
                for label, pos in (("full context", ctx - 20), ("behind the shift", ctx - discard)):
                    e.decode_greedy_steps(11, pos, 4)
                    t0 = time.perf_counter()
                    e.decode_greedy_steps(11, pos, 16)
                    step = (time.perf_counter() - t0) * 1e3 / 16
                    shift = results.get((ctx, kind, discard))
                    say("%-5s context %6d  %-16s position %6d  %7.3f ms per step%s" %
                        (kind, ctx, label, pos, step, "   (the shift: %.3f ms = %.1f steps)" % (shift, shift / step) if shift else ""))
                # the engine's own call, end to end (host clock around the call and a synchronising read-back)
                t0 = time.perf_counter()
                e.kv_shift(0, 1, discard, ctx)
                e.decode_fused(11, ctx - discard, graph=True)
                say("%-5s context %6d  Engine.kv_shift + the next decode step, host clock: %.3f ms" % (kind, ctx, (time.perf_counter() - t0) * 1e3))
            e.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
