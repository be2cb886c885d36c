#!/usr/bin/env python3
"""Prompt-processing benchmark: (a) ntk_gemm_quant at the Llama-3.1 8B / 70B projection shapes, 16 tokens per pass,
against the per-token GEMV loop it replaces; (b) the engine's prompt pass (Engine.forward over T prompt tokens) with
batched_prefill on / off on the 8B-shaped synthetic model.
usage: python tools/prefill_bench.py [--mix Q8_0] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntransformer_amd import _lib, engine as E, gguf as G, ops  # noqa: E402
from ntransformer_amd.ops import DeviceBuffer as DB  # noqa: E402

SHAPES = {"8b.q/o": (4096, 4096), "8b.kv": (1024, 4096), "8b.gate/up": (14336, 4096), "8b.down": (4096, 14336),
          "70b.q/o": (8192, 8192), "70b.gate/up": (28672, 8192), "70b.down": (8192, 28672)}
GT = {"Q8_0": G.GGML_Q8_0, "Q4_K": G.GGML_Q4_K, "Q6_K": G.GGML_Q6_K, "F16": G.GGML_F16, "BF16": G.GGML_BF16}   # (F16 / BF16 in the per-matrix table: the F32-MFMA form; the engine part: --ab-dense-mfma16)


def timed(fn, reps):
    L = _lib.lib()
    fn(); ops.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps): fn()
    ops.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mix", default="Q8_0")
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-matrix table")
    ap.add_argument("--mixes", default="Q8_0,Q4_K,Q6_K", help="per-matrix table: weight formats")
    ap.add_argument("--tokens", default="16,64,256,1024", help="engine part: prompt lengths")
    ap.add_argument("--modes", default="2,1,0", help="engine part: 2 = FP16 GEMM, 1 = F32-MFMA GEMM, 0 = per-token loop (<= 64 tokens only)")
    ap.add_argument("--ab-row-max", action="store_true", help="engine part, mode 2: alternate prefill_row_max = 1 / 0 three times (the RMSNorm / SiLU launches leave the token maxima for the GEMM pre-pass, or the pre-pass makes its own pass over X)")
    ap.add_argument("--gemm-tokens", default="64,256", help="per-matrix table: token counts of the FP16 GEMM launches")
    ap.add_argument("--shapes", default="", help="per-matrix table: only the shapes whose name contains one of these comma-separated strings")
    ap.add_argument("--reps", type=int, default=1, help="engine part: timed passes per measurement (the median is printed)")
    ap.add_argument("--repack", type=int, default=-1, help="engine part: the engine's `repack` option (1 both copies of K-quant weights resident, 2 one copy + unpack in front of the prompt launches)")
    ap.add_argument("--model", default="8b", help="engine part: synthetic model preset (8b, 70b)")
    ap.add_argument("--layers", type=int, default=0, help="engine part: layers of the preset to build (0 = all)")
    ap.add_argument("--option", action="append", default=[], help="engine part: key=value engine options (e.g. prefill_fused_split=0)")
    ap.add_argument("--ab-rope-scaling", default="", help="engine part: a rope_scaling option value (e.g. llama3:8,1,4,8192): the prompt pass without and with it, two engines in this process, alternated, median of 3")
    ap.add_argument("--ab-dense-mfma16", action="store_true", help="engine part, F16 / BF16 mixes: alternate dense_mfma16 = 1 / 0 three times per prompt length (the 16-bit matrix cores against the F32-MFMA form of the same tree), medians; then decode tokens/s once with each setting")
    ap.add_argument("--ab-qkv-bias", action="store_true", help="engine part: the prompt pass of the qwen2.5-7b preset (three bias vectors per layer) and of its bias-free twin, two engines in this process, alternated, median of 3")
    ap.add_argument("--ab-qk-norm", action="store_true", help="engine part: the qwen3-8b preset (two Q / K norm vectors per layer) and its norm-free twin: the prompt pass with two engines in this process, alternated, median of 3; then decode tokens/s of 128 greedy steps, each engine loaded alone (it owns the static decode slots), alternated --decode-rounds times")
    ap.add_argument("--decode-rounds", type=int, default=2, help="--ab-qk-norm: how often the pair of decode measurements is repeated")
    ap.add_argument("--bf16-only", action="store_true", help="per-matrix table: only the FP16 GEMM launches (profiling; the flag keeps its round-2 name)")
    a = ap.parse_args()
    ops.init(0)
    import ctypes as C
    from ntransformer_amd import _lib
    L = _lib.lib()
    L.ntk_gemm_quant_workspace_bytes.restype = C.c_size_t
    rng = np.random.default_rng(0)
    res = {"gemm": [], "engine": []}
    T = 16
    for dname, gt in ({} if a.no_kernels else {k: v for k, v in GT.items() if k in a.mixes.split(',')}).items():
        dt = G.GGML_TO_DT[gt]
        for sname, (out_f, in_f) in SHAPES.items():
            if a.shapes and not any(x in sname for x in a.shapes.split(",")): continue
            rb = G.row_bytes(gt, in_f)
            W = DB.from_numpy(rng.integers(0, 60, out_f * rb, dtype=np.uint8))
            X = DB.from_numpy(rng.standard_normal((T, in_f)).astype(np.float32))
            Y = DB.zeros(T * out_f * 4)
            t_gemm = 0.0 if a.bf16_only else timed(lambda: ops.gemm_quant(Y, W, X, T, out_f, in_f, dt), 20)
            if dname in ("Q8_0", "Q4_K", "Q6_K") and out_f % 16 == 0:   # FP16 matrix cores, 64-token chunks
                for TT in [int(t) for t in a.gemm_tokens.split(",")]:
                    XT = DB.from_numpy(rng.standard_normal((TT, in_f)).astype(np.float32))
                    YT = DB.zeros(TT * out_f * 4)
                    t_bf = timed(ops.gemm_quant_f16_prepared([(W, YT, out_f, dt)], XT, TT, in_f), 20)
                    print("%-5s %-12s f16  gemm(%d tok) %8.1f us = %6.1f TFLOP/s (2 products each: %6.1f TFLOP/s on the matrix cores), %.2f us/token vs %.2f"
                          % (dname, sname, TT, t_bf * 1e6, 2.0 * TT * out_f * in_f / t_bf / 1e12, 4.0 * TT * out_f * in_f / t_bf / 1e12, t_bf * 1e6 / TT, t_gemm * 1e6 / 16), flush=True)
            if a.bf16_only: continue
            def loop():
                for t in range(T): ops.launch_gemv(Y.at(4 * t * out_f), W, X.at(4 * t * in_f), out_f, in_f, dt)
            t_loop = timed(loop, 5)
            mb = out_f * rb / 1e6
            row = {"dtype": dname, "shape": sname, "MB": round(mb, 2), "gemm_us": round(t_gemm * 1e6, 1), "gemv_loop_us": round(t_loop * 1e6, 1),
                   "weights_per_s_T": round(out_f * in_f / t_gemm / 1e12, 2), "weight_GBps": round(mb / t_gemm / 1e3, 1),
                   "TFLOPs": round(2.0 * T * out_f * in_f / t_gemm / 1e12, 1)}
            res["gemm"].append(row)
            print("%-5s %-12s %8.2f MB  gemm(16 tok) %8.1f us = %6.1f GB/s of weights, %5.1f TFLOP/s | 16 x gemv %8.1f us  (x%.1f)"
                  % (dname, sname, mb, row["gemm_us"], row["weight_GBps"], row["TFLOPs"], row["gemv_loop_us"], t_loop / t_gemm), flush=True)
    if not a.no_engine and a.ab_rope_scaling:
        # two engines in this process, the same synthetic model without and with the option (it shapes the load), their prompt passes alternated
        engines = []
        for spec in (None, a.ab_rope_scaling):
            eng = E.Engine()
            if spec: eng.set_option("rope_scaling", spec)
            eng.load_synthetic(E.synth_spec(a.model, a.mix, layers=a.layers) if a.layers else E.synth_spec(a.model, a.mix), 4096)
            engines.append((spec or "unscaled", eng))
        r = np.random.Generator(np.random.Philox(key=[20260925, 99]))
        for T in [int(t) for t in a.tokens.split(',')]:
            prompt = [128000] + [int(t) for t in r.integers(0, 128000, T - 1)]
            ts = {name: [] for name, _ in engines}
            for name, eng in engines: eng.forward(prompt, 0)
            for rep in range(3):
                for name, eng in engines:
                    t0 = time.perf_counter(); eng.forward(prompt, 0); ts[name].append(time.perf_counter() - t0)
            for name, eng in engines:
                med = sorted(ts[name])[1]
                res["engine"].append({"mix": a.mix, "prompt_tokens": T, "rope_scaling": name, "rope_factors": eng.rope_factors, "ms": round(med * 1e3, 2),
                                      "all_ms": [round(t * 1e3, 2) for t in ts[name]]})
                print("%s %s prompt of %4d tokens, rope_scaling %-22s (%2d factors): median of 3 %9.2f ms = %9.1f tokens/s   [%s]" %
                      (a.model.upper(), a.mix, T, name, eng.rope_factors, med * 1e3, T / med, " ".join("%.2f" % (t * 1e3) for t in ts[name])), flush=True)
        for _, eng in engines: eng.close()
    elif not a.no_engine and a.ab_qkv_bias:
        # two engines in this process: the Qwen2.5-7B shape with its three bias vectors per layer and its bias-free twin (the same seeded matrices), their
        # prompt passes alternated -- the difference is one ntk_qkv_bias launch per layer
        engines = []
        for preset in ("qwen2.5-7b-nobias", "qwen2.5-7b"):
            eng = E.Engine()
            eng.load_synthetic(E.synth_spec(preset, a.mix, layers=a.layers) if a.layers else E.synth_spec(preset, a.mix), 4096)
            engines.append((preset, eng))
        r = np.random.Generator(np.random.Philox(key=[20260925, 98]))
        for T in [int(t) for t in a.tokens.split(',')]:
            prompt = [151643] + [int(t) for t in r.integers(0, 151000, T - 1)]
            ts = {name: [] for name, _ in engines}
            for name, eng in engines: eng.forward(prompt, 0)
            for rep in range(3):
                for name, eng in engines:
                    t0 = time.perf_counter(); eng.forward(prompt, 0); ts[name].append(time.perf_counter() - t0)
            for name, eng in engines:
                med = sorted(ts[name])[1]
                res["engine"].append({"mix": a.mix, "prompt_tokens": T, "model": name, "qkv_bias_layers": eng.qkv_bias, "ms": round(med * 1e3, 2),
                                      "all_ms": [round(t * 1e3, 2) for t in ts[name]]})
                print("%-18s %s prompt of %4d tokens (%2d biased layers): median of 3 %9.2f ms = %9.1f tokens/s   [%s]" %
                      (name, a.mix, T, eng.qkv_bias, med * 1e3, T / med, " ".join("%.2f" % (t * 1e3) for t in ts[name])), flush=True)
        for _, eng in engines: eng.close()
    elif not a.no_engine and a.ab_qk_norm:
        # the Qwen3-8B shape with its two norm vectors per layer and its norm-free twin (the same seeded matrices): the difference is one ntk_qk_norm launch per layer
        presets = ("qwen3-8b-nonorm", "qwen3-8b")
        spec_of = lambda preset: E.synth_spec(preset, a.mix, layers=a.layers) if a.layers else E.synth_spec(preset, a.mix)
        engines = []
        for preset in presets:
            eng = E.Engine()
            eng.load_synthetic(spec_of(preset), 4096)
            engines.append((preset, eng))
        r = np.random.Generator(np.random.Philox(key=[20260925, 97]))
        for T in [int(t) for t in a.tokens.split(',')]:
            prompt = [151643] + [int(t) for t in r.integers(0, 151000, T - 1)]
            ts = {name: [] for name, _ in engines}
            for name, eng in engines: eng.forward(prompt, 0)
            for rep in range(3):
                for name, eng in engines:
                    t0 = time.perf_counter(); eng.forward(prompt, 0); ts[name].append(time.perf_counter() - t0)
            for name, eng in engines:
                med = sorted(ts[name])[1]
                res["engine"].append({"mix": a.mix, "prompt_tokens": T, "model": name, "qk_norm_layers": eng.qk_norm, "ms": round(med * 1e3, 2),
                                      "all_ms": [round(t * 1e3, 2) for t in ts[name]]})
                print("%-16s %s prompt of %4d tokens (%2d normalising layers): median of 3 %9.2f ms = %9.1f tokens/s   [%s]" %
                      (name, a.mix, T, eng.qk_norm, med * 1e3, T / med, " ".join("%.2f" % (t * 1e3) for t in ts[name])), flush=True)
        for _, eng in engines: eng.close()
        prompt = [151643] + [int(t) for t in r.integers(0, 151000, 15)]
        for rnd in range(a.decode_rounds):
            for preset in presets:
                eng = E.Engine()
                eng.load_synthetic(spec_of(preset), 4096)
                gen = lambda n: eng.generate_tokens(prompt, n, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
                gen(8)
                per = []
                for rep in range(3):
                    t0 = time.perf_counter(); gen(1); t1 = time.perf_counter(); gen(129); t2 = time.perf_counter()
                    per.append(((t2 - t1) - (t1 - t0)) / 128)
                med = sorted(per)[1]
                res["engine"].append({"mix": a.mix, "decode": True, "model": preset, "qk_norm_layers": eng.qk_norm, "ms_per_token": round(med * 1e3, 4),
                                      "all_ms": [round(t * 1e3, 4) for t in per]})
                print("%-16s %s decode, round %d (%2d normalising layers, %s): median of 3 %.4f ms per token = %.1f tokens/s   [%s]" %
                      (preset, a.mix, rnd, eng.qk_norm, eng.decode_path() if hasattr(eng, "decode_path") else "fused + graph", med * 1e3, 1.0 / med,
                       " ".join("%.4f" % (t * 1e3) for t in per)), flush=True)
                eng.close()
    elif not a.no_engine:
        eng = E.Engine()
        if a.repack >= 0: eng.set_option("repack", a.repack)
        for kv in a.option: eng.set_option(kv.split("=")[0], int(kv.split("=")[1]))
        eng.load_synthetic(E.synth_spec(a.model, a.mix, layers=a.layers) if a.layers else E.synth_spec(a.model, a.mix), 4096)
        print("resident weights: %.2f GB (repack level %s)" % (eng.resident_weight_bytes() / 1e9, a.repack if a.repack >= 0 else "default"), flush=True)
        r = np.random.Generator(np.random.Philox(key=[20260925, 99]))
        want_modes = [int(m) for m in a.modes.split(',')]
        for T in [int(t) for t in a.tokens.split(',')]:
            modes = [m for m in want_modes if m > 0 or T <= 64]
            prompt = [128000] + [int(t) for t in r.integers(0, 128000, T - 1)]
            if a.ab_row_max:
                eng.set_option("batched_prefill", 1); eng.set_option("bf16_prefill", 1)
                for rep in range(3):
                    for rm in (1, 0):
                        eng.set_option("prefill_row_max", rm)
                        eng.forward(prompt, 0)
                        t0 = time.perf_counter(); eng.forward(prompt, 0); eng.forward(prompt, 0); dt_ = (time.perf_counter() - t0) / 2
                        print("8B %s prompt of %4d tokens, FP16 GEMM, prefill_row_max=%d (rep %d): %9.2f ms = %9.1f tokens/s" % (a.mix, T, rm, rep, dt_ * 1e3, T / dt_), flush=True)
                eng.set_option("prefill_row_max", 1)
                continue
            if a.ab_dense_mfma16:
                eng.set_option("batched_prefill", 1); eng.set_option("bf16_prefill", 1)
                ts = {1: [], 0: []}
                for on in (1, 0):
                    eng.set_option("dense_mfma16", on); eng.forward(prompt, 0)      # (warm-up of both forms)
                for rep in range(3):
                    for on in (1, 0):
                        eng.set_option("dense_mfma16", on)
                        t0 = time.perf_counter(); eng.forward(prompt, 0); ts[on].append(time.perf_counter() - t0)
                med = {on: sorted(ts[on])[1] for on in ts}
                res["engine"].append({"mix": a.mix, "prompt_tokens": T, "dense_mfma16_ms": {str(on): [round(t * 1e3, 2) for t in ts[on]] for on in ts}})
                print("%s %s prompt of %4d tokens: dense_mfma16=1 %9.2f ms [%s]   dense_mfma16=0 %9.2f ms [%s]   x %.2f" %
                      (a.model.upper(), a.mix, T, med[1] * 1e3, " ".join("%.2f" % (t * 1e3) for t in ts[1]), med[0] * 1e3,
                       " ".join("%.2f" % (t * 1e3) for t in ts[0]), med[0] / med[1]), flush=True)
                print("    shader clock right behind these runs: %.0f MHz" % ops.sclk_mhz(), flush=True)
                eng.set_option("dense_mfma16", 1)
                continue
            for batched in modes:   # 2: FP16 MFMA, 64-token chunks; 1: F32 MFMA, 16 per pass; 0: the reference's per-token loop
                eng.set_option("batched_prefill", batched > 0)
                eng.set_option("bf16_prefill", batched == 2)
                eng.forward(prompt, 0)
                ts = []
                for _ in range(max(1, a.reps)):
                    t0 = time.perf_counter(); eng.forward(prompt, 0); ts.append(time.perf_counter() - t0)
                dt_ = sorted(ts)[len(ts) // 2]
                res["engine"].append({"mix": a.mix, "prompt_tokens": T, "batched": batched, "ms": round(dt_ * 1e3, 2), "tok_s": round(T / dt_, 1)})
                print("%s %s prompt of %4d tokens, batched_prefill=%d: %9.2f ms = %9.1f tokens/s" % (a.model.upper(), a.mix, T, batched, dt_ * 1e3, T / dt_), flush=True)
        if a.ab_dense_mfma16:   # the decode path does not read the option: tokens/s of 64 graph-replayed steps behind a 16-token prompt, once per setting
            for on in (1, 0):
                eng.set_option("dense_mfma16", on)
                eng.forward(prompt[:16], 0)
                for i in range(8): eng.decode_fused(5, 16 + i, True)
                t0 = time.perf_counter()
                for i in range(64): eng.decode_fused(5, 24 + i, True)
                dt_ = (time.perf_counter() - t0) / 64
                print("%s %s decode, dense_mfma16=%d: %.1f tokens/s (%.3f ms per token)" % (a.model.upper(), a.mix, on, 1.0 / dt_, dt_ * 1e3), flush=True)
            eng.set_option("dense_mfma16", 1)
        eng.close()
    if a.json: json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
