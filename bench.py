#!/usr/bin/env python3
"""bench.py -- decode tokens/s of the MI355X-native engine on BASELINE.json's headline configuration.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one greedy decode token (one pass of the hot path over the resident weights, batch 1).  The
workload at N=1 is BASELINE.json configs[1]: Llama-3.1-8B-shaped Q8_0, weights resident in HBM, greedy decode
after a 16-token prompt (seeded synthetic weights: no checkpoint exists offline).  W untimed warm-up tokens, then
exactly K tokens timed between (barrier + device synchronize) pairs; rank 0 prints ONE JSON line.  With N > 1
every rank runs an independent whole-model replica on its own GPU (the path has no exchange step),
`value` = N*K / max-over-ranks time, scaling = weak.

A plain run does only what the headline needs: load, prompt, warm-up, the K timed steps, the JSON line.
--dump-outputs DIR writes, after the timed steps, what the timed path returned (rank 0):
  tokens.npy            -- the K token ids of the timed steps (float64), the last one from the last step
  last_step_logits.npy  -- the last timed step's logits (float32, vocab): that step run once more on the same token and position
Weights and prompt are seeded, so two builds given the same arguments can be compared output for output.

--full adds everything else, each measured in the same process after the headline: the fields below, the
shader clock of the timed workload (`sclk_mhz`) and config.prompt_pass (--prompt-bench).  Besides the contract
fields a --full line carries
  roofline     -- HBM roofline of the dominant kernel (the dequant-fused GEMV): algorithmic bytes per launch /
                  average launch duration measured with HIP event pairs on the compute stream
  cpu_baseline -- the reference's own CLI + host loop (oracle/_ref/ntransformer_cpu: reference src/main.cpp, engine.cpp,
                  transformer.cpp ... compiled unmodified, linked with the CPU restatement of its CUDA kernels) run on the
                  SAME full-size 8B Q8_0 GGUF on this host's cores; its own `Decode: ... tok/s` line is the value
  config.also  -- the other BASELINE configurations timed in the same process the same way, one compact entry each {k, value, ms,
                  frac (end to end, of 8 TB/s), gemv_frac (GEMV launches, live HIP events), prompt_tok_s}: at N = 1 8B Q4_K_M (config 3),
                  70B Q4_K_M -n 64 (config 4), 70B Q6_K -n 64 (config 5, one replica) and the headline model decoding behind a 3900-token
                  prompt (the split-KV attention regime); at N > 1 the 70B Q6_K replicas of config 5 (whole-job value over the N GPUs).
                  The line stays under 5 KB so that a log window of the driver cannot cut an entry off
  vs_baseline  -- whole-job value / the published single-GPU number of BASELINE.md (48.9 tok/s, RTX 3090): with N independent replicas
                  (scaling = weak) that is N x the per-GPU speed-up, which `vs_baseline_per_gpu` states on its own
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md); measured copy ceiling 6290 GB/s
HBM_COPY_CEILING_GBS = 6290.0   # measured float4 copy (79 % of spec), same guide: SURVEY 8(d) asks for the fraction of both
REF_3090_TOK_S = 48.9          # reference, RTX 3090, same metric and model config


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--model", default="8b", choices=["tiny", "small", "8b", "70b"])
    ap.add_argument("--mix", default="Q8_0")
    ap.add_argument("--ctx", type=int, default=4096)
    ap.add_argument("--prompt-len", type=int, default=16)
    ap.add_argument("--no-fuse", action="store_true", help="the reference's 15-launch/layer sequence")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--persistent", type=int, nargs="?", const=1, default=0,
                    help="EXPERIMENTS=1 library only: 1 = the round-2 persistent token kernel, 2 = the round-5 loader / consumer layer engine, instead of fused launches")
    ap.add_argument("--no-repack", action="store_true", help="K-quant decode GEMVs from the raw GGUF blocks (csrc/gemv.hip) instead of the engine's load-time repack (csrc/gemv_rp.hip)")
    ap.add_argument("--attention-merge", action="store_true", help="split-KV decode attention as ONE launch (csrc/attention_merge.hip.h; A/B: identical results, measured slower)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-tokens", type=int, default=128, help="-n of the reference CLI run that is the CPU baseline (BASELINE config 1: 128)")
    ap.add_argument("--no-also", action="store_true", help="skip the other BASELINE configurations (8B Q4_K_M, 70B Q4_K_M, 70B Q6_K, 8B Q8_0 behind 3900- and 32768-token prompts)")
    ap.add_argument("--no-pmc-note", action="store_true")
    ap.add_argument("--prompt-bench", type=int, default=1024, help="also time one prompt pass of this many tokens (0 = skip); reported under config.prompt_pass")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline, shader clock, prompt pass, the other configurations, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last step to DIR/*.npy (see the module docstring)")
    return ap.parse_args()


# ---------------------------------------------------------------------------------------------------
# CPU baseline
# ---------------------------------------------------------------------------------------------------
def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def host_cpu_budget():
    """Threads the CPU baseline uses and everything they were derived from (oracle.host_cpu_budget: affinity mask, SMT
    siblings counted once, cgroup CPU quota), so two boxes that report different `cores` explain themselves."""
    from oracle import oracle as O
    return O.host_cpu_budget()


def _scratch_file(name, need_bytes):
    import shutil
    for d in ("/dev/shm", "/tmp"):
        try:
            if os.path.isdir(d) and os.access(d, os.W_OK) and shutil.disk_usage(d).free > need_bytes * 1.1:
                return os.path.join(d, name)
        except OSError:
            continue
    return None


def cpu_baseline_reference_cli(args, spec):
    """SURVEY 8(d) / BASELINE.md section 3: oracle/_ref/ntransformer_cpu -- the reference's unmodified main.cpp / Engine /
    Transformer host loop, CPU-only -- on the full-size GGUF of the headline workload, greedy; the number is the CLI's own
    `Decode: N tokens, T ms (R tok/s)` statistics line (reference src/inference/engine.cpp:595-600)."""
    from ntransformer_amd import engine as E
    exe = os.path.join(ROOT, "oracle", "_ref", "ntransformer_cpu")
    if not os.path.exists(exe):
        raise FileNotFoundError("oracle/_ref/ntransformer_cpu is not built (make -C oracle ref, needs /root/reference)")
    threads, info = host_cpu_budget()
    gguf_bytes = 9.2e9 if args.model == "8b" else 1e9
    path = _scratch_file("_bench_cpu_%s_%s_%d.gguf" % (args.model, args.mix.lower(), os.getpid()), gguf_bytes)   # (per process: shared directory)
    if path is None:
        raise RuntimeError("no scratch space for the %.1f GB GGUF" % (gguf_bytes / 1e9))
    t0 = time.perf_counter()
    E.synth_write_gguf(path, spec)
    t_write = time.perf_counter() - t0
    try:
        # threads pinned to the first `threads` CPUs of the affinity mask (one per core), two runs, the better one reported with both and the
        # host's load average before and after (the boxes are shared: a 256-thread host has been seen at loadavg 39 with our 16-thread quota)
        cpus = sorted(os.sched_getaffinity(0))[:max(1, threads)] if hasattr(os, "sched_getaffinity") else []
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_PROC_BIND="close", OMP_PLACES="cores", OMP_WAIT_POLICY="passive")
        pin = (lambda: os.sched_setaffinity(0, cpus)) if cpus else None
        # 15 ASCII bytes = BOS + 15 byte-level tokens in the synthetic vocabulary (GPT-2 byte alphabet, no merges): the 16-token prompt
        # length of the GPU run, greedy, -n 128 = BASELINE config 1 / SURVEY 8(d)
        cpu_prompt = "abcdefghijklmno"[:max(1, args.prompt_len - 1)]
        cmd = [exe, "-m", path, "-p", cpu_prompt, "-n", str(args.cpu_tokens), "-t", "0", "--repeat-penalty", "1.0", "-c", str(args.ctx)]
        load0 = os.getloadavg()[0]
        runs, wall = [], 0.0
        for _ in range(2):
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, preexec_fn=pin)
            wall += time.perf_counter() - t0
            txt = r.stderr + r.stdout
            m = re.search(r"Decode:\s+(\d+) tokens,\s+([0-9.]+) ms \(([0-9.]+) tok/s\)", txt)
            if r.returncode != 0 or not m:
                raise RuntimeError("reference CLI failed (rc %d): %s" % (r.returncode, txt[-400:]))
            runs.append((int(m.group(1)), float(m.group(2))))
        load1 = os.getloadavg()[0]
        n_dec, ms_dec = min(runs, key=lambda t: t[1] / t[0])
        return {"value": round(n_dec / (ms_dec * 1e-3), 4), "unit": "tokens/s", "cores": threads, "kind": "port",
                "runs_tok_s": [round(n / (ms * 1e-3), 4) for n, ms in runs], "loadavg_1m_before_after": [round(load0, 1), round(load1, 1)],
                "pinned_cpus": cpus[:4] + (["..."] if len(cpus) > 4 else []),
                "sample": "oracle/_ref/ntransformer_cpu (the reference's unmodified CLI / Engine / Transformer over the CPU restatement of its kernels), full %s %s GGUF "
                          "(%.1f GB), -p <%d tokens> -n %d greedy: its own Decode: line, best of two pinned runs: %d tokens in %.0f ms (%.0f s of runs)"
                          % (args.model, args.mix, os.path.getsize(path) / 1e9, len(cpu_prompt) + 1, args.cpu_tokens, n_dec, ms_dec, wall),
                "host": _cpu_model(), "host_cpus": info}
    finally:
        try:
            os.remove(path)
        except OSError:
            pass


# ---------------------------------------------------------------------------------------------------
# one workload on this rank's GPU
# ---------------------------------------------------------------------------------------------------
def _gemv_bytes_per_token(spec, mix):
    """Bytes of the matrices the GEMV launches stream per token = weights minus the embedding table (gathered, 1 row)."""
    from ntransformer_amd import gguf as G
    shape = G.LlamaShape("b", spec.hidden, spec.inter, spec.layers, spec.heads, spec.kv_heads, spec.vocab)
    types = G.tensor_types(shape, mix if mix == "Q4_K_M" else {"Q4_K": "Q4_K", "Q5_K": "Q5_K"}.get(mix, mix))
    hd = spec.hidden // spec.heads
    dims = {"attn_q": (spec.hidden, spec.heads * hd), "attn_k": (spec.hidden, spec.kv_heads * hd), "attn_v": (spec.hidden, spec.kv_heads * hd),
            "attn_output": (spec.heads * hd, spec.hidden), "ffn_gate": (spec.hidden, spec.inter), "ffn_up": (spec.hidden, spec.inter),
            "ffn_down": (spec.inter, spec.hidden)}
    total = G.row_bytes(types["output.weight"], spec.hidden) * spec.vocab
    for name, t in types.items():
        if name.startswith("blk."):
            i, o = dims[name.split(".")[2]]
            total += G.row_bytes(t, i) * o
    return total


def _gemv_bytes_by_kind(spec, mix):
    """average bytes of the five kinds of GEMV launch of a fused decode token: {"qkv", "wo", "gate_up", "down"} per layer (mean over the layers: the
    Q4_K_M mix changes attn_v / ffn_down types by layer) and "lm_head" -> (bytes, launches per token)"""
    from ntransformer_amd import gguf as G
    shape = G.LlamaShape("b", spec.hidden, spec.inter, spec.layers, spec.heads, spec.kv_heads, spec.vocab)
    types = G.tensor_types(shape, mix if mix == "Q4_K_M" else {"Q4_K": "Q4_K", "Q5_K": "Q5_K"}.get(mix, mix))
    hd = spec.hidden // spec.heads
    dims = {"attn_q": (spec.hidden, spec.heads * hd), "attn_k": (spec.hidden, spec.kv_heads * hd), "attn_v": (spec.hidden, spec.kv_heads * hd),
            "attn_output": (spec.heads * hd, spec.hidden), "ffn_gate": (spec.hidden, spec.inter), "ffn_up": (spec.hidden, spec.inter),
            "ffn_down": (spec.inter, spec.hidden)}
    kind_of = {"attn_q": "qkv", "attn_k": "qkv", "attn_v": "qkv", "attn_output": "wo", "ffn_gate": "gate_up", "ffn_up": "gate_up", "ffn_down": "down"}
    tot = {"qkv": 0, "wo": 0, "gate_up": 0, "down": 0}
    for name, t in types.items():
        if name.startswith("blk."):
            i, o = dims[name.split(".")[2]]
            tot[kind_of[name.split(".")[2]]] += G.row_bytes(t, i) * o
    out = {k: (v / spec.layers, spec.layers) for k, v in tot.items()}
    out["lm_head"] = (G.row_bytes(types["output.weight"], spec.hidden) * spec.vocab, 1)
    return out


def _launch_model(spec, mix, kinds):
    """t = fixed + bytes / rate fitted (least squares over the launches of a token) to the per-kind kernel durations of the committed trace: what a
    reader needs to re-derive the GEMV launches' roofline fraction from this line alone.  DESIGN section 8: the headline's structure."""
    if not kinds:
        return None
    by = _gemv_bytes_by_kind(spec, mix)
    rows = [(by[k][0], kinds[k]["avg_us"], by[k][1]) for k in ("qkv", "wo", "gate_up", "down", "lm_head") if k in kinds and k in by]
    if len(rows) < 3:
        return None
    n = sum(w for _, _, w in rows)
    mx = sum(b * w for b, _, w in rows) / n
    my = sum(t * w for _, t, w in rows) / n
    sxx = sum(w * (b - mx) ** 2 for b, _, w in rows)
    sxy = sum(w * (b - mx) * (t - my) for b, t, w in rows)
    slope = sxy / sxx                      # us per byte
    fixed = my - slope * mx
    return {"form": "t_us = fixed_us + MB / stream_TBs, fitted to per_launch (trace): kind -> [MB, us, launches/token]",
            "fixed_us": round(fixed, 2), "stream_TBs": round(1e-6 / slope, 2) if slope > 0 else None,
            "per_launch": {k: [round(by[k][0] / 1e6, 2), round(kinds[k]["avg_us"], 2), by[k][1]] for k in ("qkv", "wo", "gate_up", "down", "lm_head") if k in kinds},
            "fixed_share_of_gemv_time": round(fixed * n / sum(t * w for _, t, w in rows), 3)}


ACTIVATION_FORMS = {
    "f32": "F32 activations x integer weights, F32 accumulate (csrc/gemv.hip)",
    "int24-block": "K-quant decode: x as 3 int8 digit planes of rint(x 2^(22-e)), e per 256 columns, exact integer dots on v_mfma_i32_16x16x64_i8",
}


def activation_form(mix, repack=True):
    return "f32" if (mix in ("Q8_0", "Q4_0", "F16", "F32") or not repack) else "int24-block"


def dump_outputs(eng, args, out, tok, pos_end, dump_dir):
    """--dump-outputs: the token ids the timed call returned and the logits of its last step.  The path keeps no logits on the host
    (the greedy token is picked on the device), so that step is run once more on its own input token and position: the KV row it
    writes holds the same values, everything before it is unchanged."""
    import numpy as np
    os.makedirs(dump_dir, exist_ok=True)
    last_in = out[-2] if len(out) > 1 else tok
    if args.no_fuse:
        logits = eng.forward([last_in], pos_end - 1)
    else:
        logits = eng.decode_fused(last_in, pos_end - 1, graph=not args.no_graph)
    np.save(os.path.join(dump_dir, "tokens.npy"), np.asarray(out, dtype=np.float64))
    np.save(os.path.join(dump_dir, "last_step_logits.npy"), np.asarray(logits, dtype=np.float32))


def run_workload(args, model, mix, steps, warmup, timed, sync, prompt_len=None, ctx=None, dump_dir=None):
    """Load `model`:`mix` resident, prompt + first token untimed, `warmup` tokens untimed, exactly `steps` greedy decode
    tokens timed by `timed` (replica.timed_steps partial).  Returns the measurements; with --full the rank-local roofline,
    shader clock and prompt pass too."""
    import numpy as np
    from ntransformer_amd import engine as E
    spec = E.synth_spec(model, mix)
    eng = E.Engine()
    eng.set_option("fused", not args.no_fuse)
    eng.set_option("graph", not args.no_graph)
    if args.attention_merge:
        eng.set_option("attention_merge", 1)
    if args.persistent:
        eng.set_option("persistent", args.persistent)
    if args.no_repack:
        eng.set_option("repack", 0)
    ctx = ctx or args.ctx
    t_load = time.perf_counter()
    eng.load_synthetic(spec, ctx)
    t_load = time.perf_counter() - t_load
    rng = np.random.Generator(np.random.Philox(key=[20260925, 99]))
    prompt_len = prompt_len or args.prompt_len
    prompt = [spec.bos] + [int(t) for t in rng.integers(0, spec.vocab, prompt_len - 1)]
    # prefill + first token (untimed), exactly Engine::generate's first half
    first = eng.generate_tokens(prompt, 1, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
    tok, pos = first[0], len(prompt)
    warm = eng.decode_greedy_steps(tok, pos, warmup) if warmup > 0 else []
    if warm:
        tok = warm[-1]
    pos += warmup
    elapsed, _, out = timed(lambda k: eng.decode_greedy_steps(tok, pos, k), steps)
    pos_end = pos + steps
    if dump_dir:
        dump_outputs(eng, args, out, tok, pos_end, dump_dir)
    res = {"spec": spec, "prompt_len": prompt_len, "elapsed": elapsed, "pos": pos, "pos_end": pos_end, "t_load": t_load,
           "b_tok": eng.bytes_per_token(pos + steps // 2), "path": eng.decode_path() if hasattr(eng, "decode_path") else None,
           "resident_bytes": eng.resident_weight_bytes() if hasattr(eng, "resident_weight_bytes") else None, "ctx": ctx}
    if not args.full:
        eng.close()
        return res
    sclk = None
    try:   # the average shader clock of the same workload, over 32 more steps right behind the timed region (a one-wave kernel beside them on
        # another stream: ntk_debug_sclk_begin / _end): lets a profiled pass be compared with an un-profiled one
        from ntransformer_amd import ops as _ops
        profiled = (any("ROCPROF" in k or k.startswith("ROCP_") for k in os.environ)
                    or "rocprof" in os.environ.get("LD_PRELOAD", ""))   # rocprofv3 serialises kernels: nothing can run BESIDE the steps
        if profiled:
            sclk = round(_ops.sclk_mhz(), 1)       # ... so there: one wave spinning for 50 us right behind the timed region
        elif pos_end + 32 <= ctx and out:
            with _ops.SclkSpan() as c:
                eng.decode_greedy_steps(out[-1], pos_end, 32)
                sync()
            sclk = round(c.mhz, 1) if c.mhz else None
    except Exception:
        sclk = None
    res["sclk_mhz"] = sclk

    # ---- roofline of the dominant kernel, measured live with HIP events on the compute stream over a few eagerly
    # launched tokens (the fused launch sequence: the persistent token kernel has no per-operator boundaries to put
    # events on).  `coarse`: one event per run of GEMV launches (o, gate|up, down, next qkv between two attention
    # launches), so the events' own cost (~2 us each) is paid once per 4 launches; `fine` (an event pair per launch,
    # reads ~2 us high per launch) is reported beside it.  rocprofv3's kernel trace of this command is in profiles/.
    def prof(coarse, n_prof=4):
        ms, calls = [0.0] * 4, [0] * 4
        for i in range(n_prof):
            m_, c_ = eng.profile_token(out[-1] if out else tok, min(pos_end + i, ctx - 1), coarse)
            ms = [a + b for a, b in zip(ms, m_)]
            calls = [a + b for a, b in zip(calls, c_)]
        return [m / n_prof for m in ms], [c / n_prof for c in calls]
    ms, calls = prof(True)
    ms_fine, calls_fine = prof(False)
    res.update(ms=ms, calls=calls, ms_fine=ms_fine, calls_fine=calls_fine, gemv_bytes_tok=_gemv_bytes_per_token(spec, mix))
    # ---- prompt pass, outside the timed decode region: one 1024-token prompt through the batched
    # projections (FP16 matrix cores) and the matrix-core prompt attention; second of two runs, host-timed around the sync
    res["prompt"] = None
    if getattr(args, "prompt_bench", 0) and ctx >= args.prompt_bench:
        try:
            long_prompt = [spec.bos] + [int(t) for t in rng.integers(0, spec.vocab, args.prompt_bench - 1)]
            eng.forward(long_prompt, 0)
            t0 = time.perf_counter()
            eng.forward(long_prompt, 0)
            dt = time.perf_counter() - t0
            res["prompt"] = {"tokens": args.prompt_bench, "ms": round(dt * 1e3, 2), "tokens_per_s": round(args.prompt_bench / dt, 1)}
        except Exception as e:   # never at the expense of the decode number
            res["prompt"] = {"tokens": args.prompt_bench, "error": repr(e)}
    eng.close()
    return res


def run_sequences(args, model, mix, steps, warmup, sync, nseq=2):
    """`nseq` independent greedy sequences on ONE GPU over ONE resident copy of the weights (nt_engine_load_shared: SURVEY 8(e) shards the path across
    requests): nseq engines, nseq HIP streams, nseq host threads, separate KV caches.  A single stream leaves ~15 % of the chip idle inside its launch
    gaps; further ones fill them.  Returns aggregate and per-sequence tokens/s over exactly `steps` tokens each, device-synchronised on both sides."""
    import threading
    import numpy as np
    from ntransformer_amd import engine as E
    spec = E.synth_spec(model, mix)
    a = E.Engine()
    a.load_synthetic(spec, args.ctx)
    engs, state = [a], []
    for _ in range(nseq - 1):
        b = E.Engine()
        b.load_shared(a, args.ctx)
        engs.append(b)
    for i, eng in enumerate(engs):
        rng = np.random.Generator(np.random.Philox(key=[20260925, 99 + i]))
        prompt = [spec.bos] + [int(t) for t in rng.integers(0, spec.vocab, args.prompt_len - 1)]
        tok = eng.generate_tokens(prompt, 1, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)[0]
        pos = len(prompt)
        if warmup > 0:
            tok = eng.decode_greedy_steps(tok, pos, warmup)[-1]
        state.append((tok, pos + warmup))
    sync()
    # one sequence alone first (same engines, same positions are NOT reused: a fresh pair of start states would need a re-prefill; the solo rate of
    # this workload is the headline of this line)
    done = [0.0] * nseq
    outs = [None] * nseq
    gate = threading.Barrier(nseq + 1)

    def worker(i):
        tok, pos = state[i]
        gate.wait()
        t0 = time.perf_counter()
        outs[i] = engs[i].decode_greedy_steps(tok, pos, steps)
        done[i] = time.perf_counter() - t0
    th = [threading.Thread(target=worker, args=(i,)) for i in range(nseq)]
    for t in th:
        t.start()
    gate.wait()
    t0 = time.perf_counter()
    for t in th:
        t.join()
    sync()
    wall = time.perf_counter() - t0
    res = {"k": "%s_%s_x%d_per_gpu" % (model, mix.lower(), nseq), "value": round(nseq * steps / wall, 2), "ms": round(1e3 * wall / steps, 4), "steps": steps,
           "per_sequence": [round(steps / d, 2) for d in done], "sequences": nseq, "resident_GB": round(a.resident_weight_bytes() / 1e9, 2),
           "frac": round(a.bytes_per_token(state[0][1] + steps // 2) * (nseq * steps / wall) / (HBM_PEAK_GBS * 1e9), 4)}
    for e in engs[1:]:
        e.close()
    a.close()
    return res


def roofline_block(args, model, mix, r):
    launches_tok = r["calls"][0]
    avg_launch_ms = r["ms"][0] / max(r["calls"][0], 1)
    achieved = (r["gemv_bytes_tok"] / max(launches_tok, 1)) / (avg_launch_ms * 1e-3) / 1e9 if avg_launch_ms > 0 else 0.0
    traffic, traffic_src = _pmc_traffic(model, mix)
    tr = _trace_gemv(model, mix, r.get("prompt_len"))
    kern = "gemv_quant_kernel" if activation_form(mix, not args.no_repack) == "f32" else "rp_gemv_kernel"
    return {"bound": "hbm", "kernel": "ntk::%s, %s (all projection launches of a token pooled)" % (kern, mix),
            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "frac_events": round(achieved / HBM_PEAK_GBS, 4),
            # also against the measured copy ceiling of the device (6.29 TB/s float4 copy, MI355X_MICROARCH.md chip table)
            "frac_of_copy_ceiling_6290GBs": round(achieved / HBM_COPY_CEILING_GBS, 4),
            "frac_trace_of_copy_ceiling": round(tr["frac"] * HBM_PEAK_GBS / HBM_COPY_CEILING_GBS, 4) if tr.get("frac") else None,
            "launch_model": _launch_model(r["spec"], mix, tr.get("kinds")),
            # the same quantity from the committed rocprofv3 --kernel-trace of this workload (tools/prof_summary.py --json -> profiles/trace_gemv.json):
            # bytes per launch / average GEMV kernel duration.  frac (= frac_events) carries the cost of the HIP events, frac_trace does not.
            "frac_trace": tr.get("frac"), "avg_launch_us_trace": tr.get("avg_us"),   # (profiles/trace_gemv.json)
            "traffic": traffic,                                                       # (profiles/pmc_traffic.json)
            "bytes_per_launch": int(r["gemv_bytes_tok"] / max(launches_tok, 1)), "launches_per_token": launches_tok,
            "avg_launch_us": round(avg_launch_ms * 1e3, 2),
            "avg_launch_us_event_pair_per_launch": round(r["ms_fine"][0] / max(r["calls_fine"][0], 1) * 1e3, 2),
            "timed_runs_per_token": r["calls"][3],
            "token_ms_by_class_eager": {"gemv": round(r["ms"][0], 4), "attention": round(r["ms"][1], 4), "other": round(r["ms"][2], 4)}}


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and world != args.gpus:
        print("bench.py: WORLD_SIZE=%d but --gpus %d" % (world, args.gpus), file=sys.stderr)
    os.environ["NTK_DEVICE"] = str(local_rank)

    from ntransformer_amd import replica
    # torch only as rendezvous / barrier / max-reduce plumbing: replicas exchange no data, so 8 bytes per run go over gloo
    # (NT_DIST_BACKEND=nccl for RCCL)
    dist, backend = replica.init_distributed("gloo", local_rank) if world > 1 else (None, None)

    from ntransformer_amd import _lib
    from ntransformer_amd import engine as E
    L = _lib.lib()
    ndev = L.ntk_device_count()
    dev = local_rank
    if ndev > 0 and local_rank >= ndev:   # more ranks than GPUs (only ever a test of the multi-rank plumbing): share devices
        dev = local_rank % ndev
        print("bench.py: rank %d shares GPU %d (%d visible)" % (rank, dev, ndev), file=sys.stderr)
    os.environ["NTK_DEVICE"] = str(dev)
    _lib.check(L.ntk_device_init(dev), "ntk_device_init(%d)" % dev)

    def sync():
        _lib.check(L.ntk_device_synchronize(), "device sync")

    def timed_all_ranks(fn, k):
        return replica.timed_steps(fn, k, sync, dist, backend)

    def timed_local(fn, k):
        return replica.timed_steps(fn, k, sync, None, None)

    r = run_workload(args, args.model, args.mix, args.steps, args.warmup, timed_all_ranks, sync,
                     dump_dir=args.dump_outputs if rank == 0 else None)
    headline = (args.model, args.mix) == ("8b", "Q8_0")
    if args.full and rank != 0 and world > 1 and headline and not args.no_also:   # (rank 0 runs it below, inside the collective timing: same order on every rank)
        try:
            keep_pb, args.prompt_bench = args.prompt_bench, 0
            run_workload(args, "70b", "Q6_K", 64, min(args.warmup, 8), timed_all_ranks, sync)
            args.prompt_bench = keep_pb
        except Exception as e:
            print("bench.py: rank %d: 70B Q6_K replica failed: %r" % (rank, e), file=sys.stderr)

    if rank == 0:
        elapsed = r["elapsed"]
        tok_s = world * args.steps / elapsed
        line = {
            "metric": "decode tokens/sec (Llama-3.1-8B Q8_0 class, resident weights, greedy, batch 1)" if headline
                      else "decode tokens/sec (%s %s, resident weights, greedy, batch 1)" % (args.model, args.mix),
            "value": round(tok_s, 3), "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4), "sclk_mhz": r.get("sclk_mhz"), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": round(tok_s / REF_3090_TOK_S, 3) if headline else None,   # whole-job value / the published single-GPU number
            "vs_baseline_per_gpu": round(tok_s / world / REF_3090_TOK_S, 3) if headline else None,
            "dtype": "f32", "activation_form": activation_form(args.mix, not args.no_repack), "data": "synthetic",   # (forms: ACTIVATION_FORMS above / DESIGN 3.1-3.2)
            "config": {"workload": "Llama-3.1-%s-shaped %s GGUF tensors (seed 20260925), resident in HBM, %d-token prompt, greedy decode"
                                   % (args.model.upper(), args.mix, args.prompt_len),
                       "ctx": args.ctx, "decode_positions": [r["pos"], r["pos_end"]], "replicas": world,
                       "path": "1:1 launchers (15/layer)" if args.no_fuse else (r["path"] or "fused (5 launches/layer)"),
                       "hipgraph": not args.no_graph and not args.no_fuse,
                       "algorithmic_bytes_per_token": r["b_tok"], "load_seconds": round(r["t_load"], 2),
                       "prompt_pass": r.get("prompt")},
            "hbm_fraction_of_8TBs_end_to_end": round(r["b_tok"] * tok_s / world / (HBM_PEAK_GBS * 1e9), 4),
            "roofline": roofline_block(args, args.model, args.mix, r) if args.full else None,
        }
        if not args.full:   # measured by --full only
            del line["sclk_mhz"], line["roofline"], line["config"]["prompt_pass"]
        # ---- the other BASELINE configurations under the same clock: compact entries (the whole line stays under 5 KB) ----
        def also_entry(key, model, mix, steps, a, nrep):
            a_tok_s = nrep * steps / a["elapsed"]
            rb = roofline_block(args, model, mix, a)
            e = {"k": key, "value": round(a_tok_s, 2), "ms": round(1e3 * a["elapsed"] / steps, 4), "steps": steps,
                 "frac": round(a["b_tok"] * a_tok_s / nrep / (HBM_PEAK_GBS * 1e9), 4), "gemv_us": rb["avg_launch_us"],
                 "roofline": {"frac_events": rb["frac_events"], "frac_trace": rb["frac_trace"], "us_trace": rb["avg_launch_us_trace"],
                              "traffic": rb["traffic"], "bytes_per_launch": rb["bytes_per_launch"]},
                 "pos": [a["pos"], a["pos_end"]], "form": activation_form(mix, not args.no_repack), "sclk_mhz": a["sclk_mhz"],
                 "resident_GB": round(a["resident_bytes"] / 1e9, 2) if a.get("resident_bytes") else None}
            if a.get("kv_frac") is not None:
                e["kv_frac"] = a["kv_frac"]
            if a.get("prompt") and "tokens_per_s" in a["prompt"]:
                e["prompt_tok_s"] = a["prompt"]["tokens_per_s"]
            return e
        if args.full:
            line["config"]["also_legend"] = ("k = model_mix[_ctx<prompt tokens>]; value tokens/s; frac = algorithmic bytes/token x tokens/s / 8 TB/s; roofline (GEMV launches): frac_events (live HIP "
                                             "events), frac_trace / us_trace (committed rocprofv3 trace), traffic (PMC bytes per launch); resident_GB = weights in HBM; prompt_tok_s = 1024-token "
                                             "prompt pass; _xN_per_gpu = N sequences / streams over ONE copy of the weights (nt_engine_load_shared), no batching: all tokens / wall time")
        if args.full and headline and not args.no_also:
            also = []
            # (the last one: decode behind a 32768-token prompt -- 4.3 GB of KV cache per token, a third of the bytes: contexts beyond 4096)
            plan = ((("8b", "Q4_K_M", 128, None), ("70b", "Q4_K_M", 64, None), ("70b", "Q6_K", 64, None), ("8b", "Q8_0", 64, 3900), ("8b", "Q8_0", 32, 32768))
                    if world == 1 else (("70b", "Q6_K", 64, None),))   # N > 1: BASELINE config 5, one whole-model replica per GPU
            for model, mix, steps, plen in plan:
                key = "%s_%s%s" % (model, mix.lower(), "_ctx%d" % plen if plen else "")
                try:
                    keep_pb = args.prompt_bench
                    if plen or world > 1:
                        args.prompt_bench = 0
                    a = run_workload(args, model, mix, steps, min(args.warmup, 8), timed_local if world == 1 else timed_all_ranks, sync, prompt_len=plen,
                                     ctx=(plen + 256 if plen and plen + 256 > args.ctx else None))
                    args.prompt_bench = keep_pb
                    also.append(also_entry(key, model, mix, steps, a, world))
                except Exception as e:   # the headline must survive a problem in an extra workload
                    also.append({"k": key, "value": None, "error": repr(e)[:200]})
            if world == 1:
                for nseq in (2, 4):
                    try:
                        also.append(run_sequences(args, "8b", "Q8_0", 128, min(args.warmup, 8), sync, nseq))
                    except Exception as e:
                        also.append({"k": "8b_q8_0_x%d_per_gpu" % nseq, "value": None, "error": repr(e)[:200]})
            line["config"]["also"] = also
        if args.full and not args.no_cpu_baseline and world == 1:   # rank 0 at N = 1 only (the replicas of an N > 1 run would wait on it)
            try:
                line["cpu_baseline"] = cpu_baseline_reference_cli(args, r["spec"])
            except Exception as e:   # the GPU number must survive a CPU-side problem
                line["cpu_baseline"] = {"value": None, "unit": "tokens/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def _trace_gemv(model, mix, prompt_len=None):
    """GEMV launches of the workload in the committed rocprofv3 kernel trace (evidence pass of the round, tools/gpu_round_final.sh ->
    tools/prof_summary.py --json): average duration and bytes / duration / 8 TB/s.  Read back like the PMC traffic."""
    key = "%s_%s%s" % (model, mix.lower(), "_ctx%d" % prompt_len if prompt_len and prompt_len > 64 else "")
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "trace_gemv.json")))[key]
        return {"frac": d["frac"], "avg_us": d["avg_us"], "kinds": d.get("kinds"), "source": "profiles/trace_gemv.json[%s] (%s)" % (key, d.get("file", ""))}
    except Exception:
        return {}


def _pmc_traffic(model, mix):
    """HBM bytes per GEMV launch from the committed rocprofv3 PMC passes (FETCH_SIZE + WRITE_SIZE, separate runs of this
    command, decode window, gfx950 x2 correction on FETCH_SIZE: tools/pmc_summary.py -> profiles/pmc_traffic.json).
    PMC collection needs rocprofv3 around the process, so the number is read back, not measured in this run."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    key = "%s_%s" % (model, mix.lower())
    try:
        d = json.load(open(path))[key]
        g = d.get("ntk::gemv_quant_*") or d["ntk::gemv_quant_kernel"]   # all forms of the GEMV pooled, rp_gemv_kernel included (tools/pmc_summary.py)
        return int(g["fetch_bytes_per_launch"] + g["write_bytes_per_launch_raw"]), "profiles/pmc_traffic.json[%s]" % key
    except Exception:
        return None, None


if __name__ == "__main__":
    main()
