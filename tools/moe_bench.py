#!/usr/bin/env python3
"""What the routed expert FFN (csrc/moe.hip) costs: the engine on the two published mixture-of-experts geometries, and the three launches on their own.

  --engine   decode tokens/s (128 greedy steps behind a 16-token prompt, graph replay: generate_tokens of 129 minus generate_tokens of 1) and the 64- and
             1024-token prompt pass in ms, for `--models` (named shapes of ntransformer_amd.engine.PRESETS, seeded synthetic weights), at the engine's
             default options (the prompt pass on the grouped matrix-core GEMM from Model::kMoeGemmMinRows rows on).
  --kernels  ntk_moe_route / ntk_moe_gate_up / ntk_moe_down per layer of the Qwen3-30B-A3B shape (hidden 2048, E 128, K 8, I_e 768, Q8_0) at T = 1 / 64 /
             1024 from an event-timed loop, with the bytes each streams per token -- K x (gate + up) and K x down -- and, beside the time, what the project's
             launch model for the dense Q8_0 GEMV (README: 3.8 us + MB / 6.9 TB/s, a round-5 figure) gives for those bytes: whether the launch count
             (four per FFN against two) or the bandwidth is the limit.
             At T = 64 and 1024 also the prompt forms, ntk_moe_gemm_gate_up / ntk_moe_gemm_down (csrc/moe_gemm.hip), on the same buffers.
  --ab-moe-gemm  the prompt pass with option moe_gemm = 0 and 1 (moe_gemm_min_rows = 2, so that 1 means the grouped GEMM at every length), alternated in
             one process, median of 3, at 2 / 4 / 8 / 16 / 32 / 64 / 256 / 1024 tokens on `--models`; and the threshold the table yields: the smallest
             measured row count from which the GEMM form is faster at that and every larger measured count, per model and on all of them
             (Model::kMoeGemmMinRows is set from it).
The shader clock is read through ntk_debug_sclk where the build has it.
usage: python tools/moe_bench.py [--engine] [--kernels] [--ab-moe-gemm] [--models qwen3-30b-a3b:Q8_0,mixtral-8x7b:Q4_K_M] [--layers N] [--out profiles/moe.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntransformer_amd import _lib, gguf as G, ops  # noqa: E402
from ntransformer_amd import engine as E  # noqa: E402
from ntransformer_amd.ops import DeviceBuffer as DB  # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def sclk():
    """the 50 us probe: {shader cycles, 10 ns ticks} of one spinning wave"""
    d = DB.zeros(24)
    st = _lib.lib().ntk_debug_sclk(d.ptr, None)
    ops.synchronize()
    cyc, ticks = [int(v) for v in d.numpy(np.uint64, 2)]
    d.free()
    return "%.0f MHz" % (100.0 * cyc / ticks) if st == 0 and ticks else "not read"


def bench_engine(models, layers):
    for item in models.split(","):
        name, mix = item.split(":")
        spec = E.synth_spec(name, mix, layers=layers)
        eng = E.Engine()
        t0 = time.perf_counter()
        eng.load_synthetic(spec, 4096)
        load_s = time.perf_counter() - t0
        n_moe, (n_exp, n_used) = eng.moe(), eng.moe_experts()
        rng = np.random.Generator(np.random.Philox(key=[20261101, 3]))
        prompt = [spec.bos] + [int(t) for t in rng.integers(0, min(spec.vocab, 32000), 1023)]
        say("%s %s: %d layers (%d routed, E %d, K %d), weights %.2f GB, %.2f GB streamed per token at position 16, loaded in %.0f s" %
            (name, mix, eng.n_layers, n_moe, n_exp, n_used, eng.weight_bytes() / 1e9, eng.bytes_per_token(16) / 1e9, load_s))
        for T in (64, 1024):
            eng.forward(prompt[:T], 0)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                eng.forward(prompt[:T], 0)
                ts.append((time.perf_counter() - t0) * 1e3)
            say("    prompt of %4d tokens: median of 3 %9.2f ms = %8.1f tokens/s   [%s]" %
                (T, float(np.median(ts)), T / float(np.median(ts)) * 1e3, " ".join("%.2f" % t for t in ts)))
        per = []
        for _ in range(3):
            t0 = time.perf_counter(); eng.generate_tokens(prompt[:16], 1, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False); t1 = time.perf_counter() - t0
            t0 = time.perf_counter(); eng.generate_tokens(prompt[:16], 129, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False); t129 = time.perf_counter() - t0
            per.append((t129 - t1) / 128 * 1e3)
        med = float(np.median(per))
        say("    decode, 128 steps, graph replay (%s): median of 3 %.4f ms per token = %.1f tokens/s   [%s]" %
            (eng.decode_path(), med, 1e3 / med, " ".join("%.4f" % p for p in per)))
        eng.close()


AB_ROWS = (2, 4, 8, 16, 32, 64, 256, 1024)


def threshold(wins):
    """wins: {rows: the GEMM form was faster}: the smallest measured count from which it is faster at that and every larger one; None: nowhere"""
    best = None
    for T in sorted(wins, reverse=True):
        if not wins[T]:
            break
        best = T
    return best


def bench_ab(models, layers):
    every = {T: True for T in AB_ROWS}
    for item in models.split(","):
        name, mix = item.split(":")
        spec = E.synth_spec(name, mix, layers=layers)
        eng = E.Engine()
        eng.set_option("moe_gemm_min_rows", 2)
        t0 = time.perf_counter()
        eng.load_synthetic(spec, 4096)
        rng = np.random.Generator(np.random.Philox(key=[20261101, 3]))
        prompt = [spec.bos] + [int(t) for t in rng.integers(0, min(spec.vocab, 32000), 1023)]
        say("%s %s: %d layers (%d routed), loaded in %.0f s; prompt pass in ms, moe_gemm 0 / 1 alternated, median of 3" %
            (name, mix, eng.n_layers, eng.moe(), time.perf_counter() - t0))
        wins = {}
        for T in AB_ROWS:
            ts = {0: [], 1: []}
            for on in (0, 1):
                eng.set_option("moe_gemm", on)
                eng.forward(prompt[:T], 0)
            for _ in range(3):
                for on in (0, 1):
                    eng.set_option("moe_gemm", on)
                    t0 = time.perf_counter()
                    eng.forward(prompt[:T], 0)
                    ts[on].append((time.perf_counter() - t0) * 1e3)
            m0, m1 = float(np.median(ts[0])), float(np.median(ts[1]))
            wins[T] = m1 < m0
            every[T] = every[T] and wins[T]
            say("    %4d rows: GEMV %9.2f ms [%s] | GEMM %9.2f ms [%s] | GEMV / GEMM %6.2f" %
                (T, m0, " ".join("%.2f" % t for t in ts[0]), m1, " ".join("%.2f" % t for t in ts[1]), m0 / m1))
        say("    threshold on this shape: %s" % threshold(wins))
        eng.close()
    say("threshold on every shape measured (Model::kMoeGemmMinRows): %s" % threshold(every))


def timed_us(fn, n, rounds=5):
    L = _lib.lib()
    a, b = L.ntk_event_create(), L.ntk_event_create()
    out = []
    for _ in range(rounds):
        ops.synchronize()
        L.ntk_event_record(a, None)
        for _ in range(n):
            fn()
        L.ntk_event_record(b, None)
        L.ntk_event_synchronize(b)
        ms = C.c_float(0)
        L.ntk_event_elapsed_ms(a, b, C.byref(ms))
        out.append(ms.value / n * 1e3)
    L.ntk_event_destroy(a); L.ntk_event_destroy(b)
    return float(np.median(out))


def bench_kernels():
    H, n_exp, K, ie = 2048, 128, 8, 768
    r = np.random.Generator(np.random.Philox(key=[20261101, 9]))
    rb_h, rb_i = G.row_bytes(G.GGML_Q8_0, H), G.row_bytes(G.GGML_Q8_0, ie)
    wg = DB.from_numpy(np.frombuffer(G.synth_tensor(r, G.GGML_Q8_0, n_exp * ie, H), np.uint8))
    wu = DB.from_numpy(np.frombuffer(G.synth_tensor(r, G.GGML_Q8_0, n_exp * ie, H), np.uint8))
    wd = DB.from_numpy(np.frombuffer(G.synth_tensor(r, G.GGML_Q8_0, n_exp * H, ie), np.uint8))
    router = DB.from_numpy((2.0 / np.sqrt(H) * r.standard_normal((n_exp, H))).astype(np.float32))
    say("the three launches on the Qwen3-30B-A3B layer shape (hidden %d, E %d, K %d, I_e %d, Q8_0), event-timed, median of 5 rounds; model: 3.8 us + MB / 6.9 TB/s" % (H, n_exp, K, ie))
    for T in (1, 64, 1024):
        off, total = ops.moe_workspace_layout(T, n_exp, K, ie, H)
        ws = DB(total)
        p = {k: ws.at(v) for k, v in off.items()}
        ws.upload(r.standard_normal(T * H).astype(np.float32), off["xn"])
        hid = DB.from_numpy(r.standard_normal(T * H).astype(np.float32))
        dt = G.DT_Q8_0

        def route(): ops.moe_route(p["xn"], router, T, H, n_exp, K, p["ids"], p["w"], p["offsets"], p["pairs"])
        def gate_up(): ops.moe_gate_up(p["act"], p["xn"], wg, dt, wu, dt, p["offsets"], p["pairs"], T, H, ie, n_exp, K)
        def down(): ops.moe_down(hid, hid, p["act"], wd, dt, p["ids"], p["w"], p["offsets"], p["pairs"], p["part"], T, H, ie, n_exp, K)
        route(); gate_up(); down(); ops.synchronize()
        ids = ws.numpy(np.int32, T * K, off["ids"])
        active = len(set(int(i) for i in ids))
        n = 200 if T == 1 else 20 if T == 64 else 3
        t_r, t_g, t_d = timed_us(route, n), timed_us(gate_up, n), timed_us(down, n)
        # bytes streamed from HBM: every ACTIVE expert's matrices once (T = 1: K experts, i.e. K x (gate + up) and K x down per token)
        mb_g, mb_d = active * 2 * ie * rb_h / 1e6, active * H * rb_i / 1e6
        say("  T %4d (%3d experts active): route %8.2f us | gate|up %9.2f us for %7.2f MB = %6.0f GB/s (model %7.2f us) | down %9.2f us for %7.2f MB = %6.0f GB/s (model %7.2f us)" %
            (T, active, t_r, t_g, mb_g, mb_g / t_g * 1e3, 3.8 + mb_g / 6.9, t_d, mb_d, mb_d / t_d * 1e3, 3.8 + mb_d / 6.9))
        if T > 1:          # the prompt forms on the same buffers (the work list of the route above)
            need = ops.moe_gemm_scratch_bytes(T, n_exp, K, ie, H)
            scratch = DB(need) if need else None

            def g_gate_up(): ops.moe_gemm_gate_up(p["act"], p["xn"], wg, dt, wu, dt, p["offsets"], p["pairs"], T, H, ie, n_exp, K, scratch, need)
            def g_down(): ops.moe_gemm_down(hid, hid, p["act"], wd, dt, p["ids"], p["w"], p["offsets"], p["pairs"], p["part"], T, H, ie, n_exp, K)
            g_gate_up(); g_down(); ops.synchronize()
            t_gg, t_gd = timed_us(g_gate_up, 20), timed_us(g_down, 20)
            fl = 2.0 * T * K * ie * H
            say("         grouped GEMM:            gate|up %9.2f us = %5.1f TFLOP/s (x %5.1f)                       | down %9.2f us = %5.1f TFLOP/s (x %5.1f)" %
                (t_gg, 2 * fl / t_gg / 1e6, t_g / t_gg, t_gd, fl / t_gd / 1e6, t_d / t_gd))
            if scratch:
                scratch.free()
        ws.free(); hid.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--ab-moe-gemm", action="store_true")
    ap.add_argument("--models", default="qwen3-30b-a3b:Q8_0,mixtral-8x7b:Q4_K_M")
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the published model (a quicker run; said in the output)")
    ap.add_argument("--out", default=None, help="append the result lines to this file")
    a = ap.parse_args()
    ops.init(0)
    say("shader clock: %s" % sclk())
    if a.kernels or not (a.engine or a.ab_moe_gemm):
        bench_kernels()
    if a.engine or not (a.kernels or a.ab_moe_gemm):
        bench_engine(a.models, a.layers)
    if a.ab_moe_gemm:
        bench_ab(a.models, a.layers)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
