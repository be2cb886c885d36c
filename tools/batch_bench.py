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
"""
import argparse
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ntransformer_amd import engine as E, ops


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
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    if a.sampled:
        return main_sampled(a, batches)
    for mix in a.mix or ["Q8_0", "Q4_K_M"]:
        eng = E.Engine()
        eng.set_option("sequences", max(batches))
        spec = E.synth_spec(a.model, mix, layers=a.layers) if a.layers else E.synth_spec(a.model, mix)
        eng.load_synthetic(spec, a.ctx)
        shared = []
        for _ in range(max(batches) - 1):
            s = E.Engine()
            s.load_shared(eng, a.ctx)
            shared.append(s)
        ps = prompts(max(batches), eng.vocab_size)
        print("# --synthetic %s:%s, %d-token prompts, %d tokens per sequence, context %d, median of %d" % (a.model, mix, len(ps[0]), a.tokens, a.ctx, a.repeats))
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
