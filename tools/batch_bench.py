#!/usr/bin/env python3
"""Aggregate decode rate of B sequences over one copy of the weights, two routes on the same box and the same loaded model:
  batched  -- Engine.generate_batch: ONE batched step per token for all B sequences (option "sequences", csrc/attention_batch.hip);
  threads  -- B sequences on B host threads: the loaded engine + B - 1 nt_engine_load_shared engines, each with its own batch-1 fused
              launch chain on its own stream (the route before the batched step).
Short prompts (8 tokens, different per sequence), --tokens generated tokens per sequence (default 128), greedy, no EOS stop.  Rates are
generated tokens / decode wall time (threads: the slowest thread's span): the MEDIAN of --repeats with the spread (max - min) and every repeat listed.  The shader clock
(50 us probe, ntk_debug_sclk) is recorded behind each model's runs.  Run the whole thing under one `timeout`.

  python tools/batch_bench.py --mix Q8_0 --mix Q4_K_M > profiles/batch_decode.txt

--sampled: the SAMPLED batch instead, three routes on the same loaded model (default mix Q8_0 alone), the reference's default settings (temperature 0.7,
top_k 40, top_p 0.9, repeat penalty 1.1 over 64 tokens, one seed per sequence):
  device   -- Engine.generate_batch_ex: every row sampled on the device inside the batched step (csrc/sampling_batch.hip);
  greedy   -- Engine.generate_batch beside it (what the step costs without any sampling);
  host     -- what there was before generate_batch_ex: a loop of Engine.decode_batch WITH its [B][vocab] logits and the host sampler on every row
              (nt_sampler_draw_nth), timed from the first step to the last.
The three columns are NOT timed by one clock: device and greedy are the engine's own decode_ms (taken inside the C loop), the host column is Python's
wall clock around a Python loop, so it also pays ctypes marshalling per row and nt_sampler_draw_nth's re-seeding and skipping of k draws per row and
step -- a few microseconds each, but a bias against the host column all the same.  The printed header says so.

  python tools/batch_bench.py --sampled > profiles/batch_sampling.txt

--kv-cache f16|q8_0 (repeatable; default f16): the KV cache format of the engines; q8_0 also sets "batch_kv_q8" (the batched step over the 8-bit cache).

--start-pos P (repeatable): the batched STEP at long context instead of generation from short prompts -- rows [0, P) of every layer of every slot are
seeded through the debug writes (nt_engine_debug_kv_write_slot / _write_q8_slot: unit-variance values, the same image in every slot and layer -- the step's
time does not depend on what the rows hold), so a step at 32K positions needs no 32K prefill; then --tokens steps of Engine.decode_batch (greedy, no logits
copied) from position P on, timed by the host's clock around the loop (each step synchronises once).  All --kv-cache formats run in one invocation over ONE
copy of the weights (the second format's engine is an nt_engine_load_shared sequence), interleaved per (P, B).  --ctx must hold P + --tokens positions.

  python tools/batch_bench.py --mix Q8_0 --batches 1,4,16 --kv-cache f16 --kv-cache q8_0 --start-pos 3900 --start-pos 32768 --ctx 32832 --tokens 32
"""
import argparse
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ntransformer_amd import engine as E, kv_q8, ops


def prompts(n, vocab):
    r = np.random.Generator(np.random.Philox(key=[20261018, 5]))
    return [[1] + [int(t) for t in r.integers(2, min(vocab, 32000), 7)] for _ in range(n)]


def run_batched(eng, ps, n_tok):
    eng.generate_batch(ps, n_tok, stop_at_eos=False)
    st = eng.stats()
    return st.gen_tokens / (st.decode_ms / 1e3)


def run_threads(engs, ps, n_tok):
    spans, bar = [None] * len(engs), threading.Barrier(len(engs))

    def one(k):
        bar.wait()
        engs[k].generate_tokens(ps[k], n_tok, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
        st = engs[k].stats()
        spans[k] = (st.gen_tokens, st.decode_ms / 1e3)

    th = [threading.Thread(target=one, args=(k,)) for k in range(len(engs))]
    for t in th: t.start()
    for t in th: t.join()
    return sum(g for g, _ in spans) / max(s for _, s in spans)


def default_params(n, n_tok):
    return [E.GenParams(n_tok, 0.7, 40, 0.9, 1.1, 64, 42 + i, 0) for i in range(n)]


def run_sampled(eng, ps, n_tok):
    eng.generate_batch_ex(ps, default_params(len(ps), n_tok))
    st = eng.stats()
    return st.gen_tokens / (st.decode_ms / 1e3)


def run_host_loop(eng, ps, n_tok):
    params = default_params(len(ps), n_tok)
    seqs = [list(p) for p in ps]
    for i, p in enumerate(ps):
        seqs[i].append(E.sampler_draw_nth(eng.seq_forward(i, p, 0), params[i], seqs[i], 0))
    slots = list(range(len(ps)))
    t0 = time.perf_counter()
    for k in range(1, n_tok):
        lg, _ = eng.decode_batch(slots, [s[-1] for s in seqs], [len(s) - 1 for s in seqs])
        for i in slots:
            seqs[i].append(E.sampler_draw_nth(lg[i], params[i], seqs[i][-params[i].repeat_window:], k))   # (the window the sampler would cut itself)
    return len(ps) * (n_tok - 1) / (time.perf_counter() - t0)


def main_sampled(a, batches):
    for mix in a.mix or ["Q8_0"]:
        eng = E.Engine()
        eng.set_option("sequences", max(batches))
        spec = E.synth_spec(a.model, mix, layers=a.layers) if a.layers else E.synth_spec(a.model, mix)
        eng.load_synthetic(spec, a.ctx)
        ps = prompts(max(batches), eng.vocab_size)
        print("# --synthetic %s:%s, %d-token prompts, %d tokens per sequence, context %d, median of %d; temperature 0.7, top_k 40, top_p 0.9, repeat penalty 1.1 / 64" %
              (a.model, mix, len(ps[0]), a.tokens, a.ctx, a.repeats))
        print("# clocks: the first two columns are the engine's decode_ms (inside its C loop); the host-sampler column is Python's wall clock around a Python loop "
              "(ctypes calls, a re-seeded generator per draw): biased slow by that overhead")
        print("# B | generate_batch_ex (device sampler): aggregate tok/s median +- spread (runs) | generate_batch (greedy): the same | decode_batch + logits + host sampler: the same")
        for B in batches:
            rd = [run_sampled(eng, ps[:B], a.tokens) for _ in range(a.repeats)]
            rg = [run_batched(eng, ps[:B], a.tokens) for _ in range(a.repeats)]
            rh = [run_host_loop(eng, ps[:B], a.tokens) for _ in range(a.repeats)]
            cell = lambda r: "%8.1f +- %5.1f (%s)" % (float(np.median(r)), max(r) - min(r), " / ".join("%.1f" % x for x in r))
            print("%2d | %s | %s | %s" % (B, cell(rd), cell(rg), cell(rh)), flush=True)
        print("# shader clock behind the runs: %.0f MHz" % ops.sclk_mhz(), flush=True)
        eng.close()


def set_kv(eng, kv):
    eng.set_option("kv_cache", kv)
    if kv == "q8_0":
        eng.set_option("batch_kv_q8", 1)


def seed_rows(eng, kv, n_slots, n_rows, layers, row_elems):
    """rows [0, n_rows) of every layer of slots 0 .. n_slots - 1 <- one image of 4096 unit-variance rows, repeated"""
    r = np.random.Generator(np.random.Philox(key=[20261019, 9]))
    chunk = min(n_rows, 4096)
    if kv == "q8_0":
        nb = row_elems // 32
        img = kv_q8.to_blocks((r.uniform(0.5, 1.4, (chunk, nb)) / 73.3).astype(np.float16), r.integers(-127, 128, (chunk, nb, 32)).astype(np.int8))
        write = eng.kv_write_q8_slot
    else:
        img = r.standard_normal((chunk, row_elems)).astype(np.float16).view(np.uint16)
        write = eng.kv_write_slot
    for slot in range(n_slots):
        for layer in range(layers):
            for p0 in range(0, n_rows, chunk):
                n = min(chunk, n_rows - p0)
                write(slot, layer, p0, img[:n], img[:n])


def run_steps(eng, B, start, n_tok):
    slots, toks = list(range(B)), [2 + 3 * b for b in range(B)]
    eng.decode_batch(slots, toks, [start] * B, logits=False)   # (not timed: first-use allocations, the launch forms' first run)
    t0 = time.perf_counter()
    for i in range(n_tok):
        _, toks = eng.decode_batch(slots, toks, [start + i] * B, logits=False)
    return B * n_tok / (time.perf_counter() - t0)


def main_steps(a, batches):
    kinds = a.kv_cache or ["f16"]
    for mix in a.mix or ["Q8_0"]:
        spec = E.synth_spec(a.model, mix, layers=a.layers) if a.layers else E.synth_spec(a.model, mix)
        engs = []
        for kv in kinds:   # one copy of the weights: the later formats share the first engine's
            eng = E.Engine()
            eng.set_option("sequences", max(batches))
            set_kv(eng, kv)
            if engs: eng.load_shared(engs[0], a.ctx)
            else: eng.load_synthetic(spec, a.ctx)
            seed_rows(eng, kv, max(batches), max(a.start_pos), spec.layers, spec.kv_heads * (spec.hidden // spec.heads))
            engs.append(eng)
        print("# --synthetic %s:%s, context %d, slots seeded to %d rows; %d batched steps per run from the start position, median of %d; host clock around the loop" %
              (a.model, mix, a.ctx, max(a.start_pos), a.tokens, a.repeats))
        print("# KV cache bytes (all slots): " + ", ".join("%s %.2f GiB" % (kv, e.kv_cache_bytes() / 2 ** 30) for kv, e in zip(kinds, engs)))
        print("# start | B | " + " | ".join("%s: aggregate tok/s median +- spread (runs), ms per step" % kv for kv in kinds) + (" | q8_0 / f16" if kinds == ["f16", "q8_0"] else ""))
        for start in a.start_pos:
            for B in batches:
                runs = [[run_steps(e, B, start, a.tokens) for _ in range(a.repeats)] for e in engs]
                cell = lambda r: "%8.1f +- %5.1f (%s) %7.3f ms" % (float(np.median(r)), max(r) - min(r), " / ".join("%.1f" % x for x in r), 1e3 * B / float(np.median(r)))
                ratio = " | %.3f" % (float(np.median(runs[1])) / float(np.median(runs[0]))) if kinds == ["f16", "q8_0"] else ""
                print("%6d | %2d | %s%s" % (start, B, " | ".join(cell(r) for r in runs), ratio), flush=True)
        print("# shader clock behind the runs: %.0f MHz" % ops.sclk_mhz(), flush=True)
        for e in reversed(engs): e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="8b")
    ap.add_argument("--mix", action="append", help="weight mix of the synthetic model (repeatable; default Q8_0 and Q4_K_M)")
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the preset (a quick look)")
    ap.add_argument("--sampled", action="store_true", help="the sampled batch: device sampler / greedy / host-sampler loop (see above)")
    ap.add_argument("--kv-cache", action="append", choices=["f16", "q8_0"], help="KV cache format (repeatable; q8_0 sets batch_kv_q8; default f16)")
    ap.add_argument("--start-pos", action="append", type=int, help="time the batched step from this position on over seeded caches (repeatable; see above)")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    if a.sampled:
        return main_sampled(a, batches)
    if a.start_pos:
        return main_steps(a, batches)
    for mix, kv in [(m, k) for m in a.mix or ["Q8_0", "Q4_K_M"] for k in a.kv_cache or ["f16"]]:
        eng = E.Engine()
        eng.set_option("sequences", max(batches))
        set_kv(eng, kv)
        spec = E.synth_spec(a.model, mix, layers=a.layers) if a.layers else E.synth_spec(a.model, mix)
        eng.load_synthetic(spec, a.ctx)
        shared = []
        for _ in range(max(batches) - 1):
            s = E.Engine()
            s.set_option("kv_cache", kv)
            s.load_shared(eng, a.ctx)
            shared.append(s)
        ps = prompts(max(batches), eng.vocab_size)
        print("# --synthetic %s:%s, KV cache %s, %d-token prompts, %d tokens per sequence, context %d, median of %d" %
              (a.model, mix, kv, len(ps[0]), a.tokens, a.ctx, a.repeats))
        print("# B | batched step: aggregate tok/s median +- spread (runs) | B threads over shared weights: the same")
        for B in batches:
            rb = [run_batched(eng, ps[:B], a.tokens) for _ in range(a.repeats)]
            rt = [run_threads([eng] + shared[: B - 1], ps[:B], a.tokens) for _ in range(a.repeats)]
            cell = lambda r: "%8.1f +- %5.1f (%s)" % (float(np.median(r)), max(r) - min(r), " / ".join("%.1f" % x for x in r))
            print("%2d | %s | %s" % (B, cell(rb), cell(rt)), flush=True)
        print("# shader clock behind the runs: %.0f MHz" % ops.sclk_mhz(), flush=True)
        for s in shared: s.close()
        eng.close()


if __name__ == "__main__":
    main()
