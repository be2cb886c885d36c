"""GPU test: the engine's host-driven passes (csrc/engine/model_prompt.cpp, model_batch.cpp) give the BITS recorded in tests/golden/engine_pass_bits.json.

The other engine tests hold these passes to the oracle within 1e-3: a launch that moved, a fallback taken in another order or a buffer that changed
hands would pass most of them.  Here every entry point -- forward, score, decode_batch, decode_batch_sample, forward_batch -- and every branch of their
shared layer loop is pinned to the bytes of the commit the golden file was recorded from (tools/record_engine_bits.py, which takes CASES and run_case
from this module: the two cannot disagree).  A case loads a tiny synthetic model (gguf.make_synthetic_llama, ctx 256), sets options, makes a fixed
series of engine calls and takes ONE SHA-256 over the bytes of everything returned: logits, tokens, log-probabilities and top-1, then the cache rows of
every layer of every slot the case wrote (kv_read_slot / kv_read_q8_slot), then the logits of two decode_fused steps run afterwards (the passes left
the fused path's state alone).  A case without a recorded digest FAILS.

Models (2 layers each, so the next layer's norm runs with the down projection):
  d64   hidden 256, inter 768, 4 / 2 heads of 64, vocab 512; Q8_0, Q4_0, Q4_K_M (two formats under one X: grouped and single projections in a layer)
  d128  hidden 512, inter 1024, 4 / 2 heads of 128, vocab 512; Q8_0, Q4_K_M -- the only head size the 8-bit cache takes
  w320  tests/test_engine_narrow_widths_gpu.py's; Q8_0 -- the FP16 GEMM refuses every matrix: ntk_gemm_quant, the plain norm forms
  bigv  hidden 256, inter 512, vocab 4096; Q8_0 -- the LM head outgrows the load-time GEMM workspace: lm_head_workspace allocates
        (tests/test_engine_pass_cases_cpu.py asserts that with ntk_gemm_quant_workspace_bytes)

Calls:
  fwd-a   forward of 1, 3, 7, 17, 40, 70 tokens from position 0 (3: below the 4-token rotation form; 17, 40: the GEMM's short forms; 70: beyond the
          64-token bound of the split form -- the row-max form)
  fwd-b   a prompt of 37, 33 more at position 37, one token at position 40 (the T == 1 attention)
  opt-*   d64 Q8_0 at 17 and 70 tokens under batched_prefill=0, f16_prefill=0, prefill_row_max=0, prefill_fused_split=0, repack=0 / 1 / 2; repack=2
          also on Q4_K_M (the GEMM reads the repack itself)
  rope    d128, rope_scaling=llama3:8,1,4,64: forward of 7 and of 3 tokens (the table argument on both rotation forms)
  kvq8    d128, kv_cache=q8_0: forward of 3, of 7 (the two 8-bit store forms), 33 more; kvq8-batch: batch_kv_q8=1, sequences=3, a decode_batch of 3 rows
  score   40 tokens with score_rows=16 (chunks of 16, 16, 8), with and without top-1; on bigv too
  batch   sequences=4, seq_forward prefills of unequal length, then decode_batch of 1 row, of 3 rows at three positions (with and without logits);
          sample: decode_batch_sample of two greedy rows and one sampled row (fixed r, top_k 8, a 5-token window, penalty 1.3); rowlogits:
          generate_batch_ex with one row the device sampler does not take (top_k 100) -- decode_batch_sample's row_logits
  packed  forward_batch of segments of 5, 1 and 12 tokens at positions 0, 9, 0 (slot 1 prefilled with 9 tokens), with logits and with next_out alone

Run on the MI355X box:  python -m pytest tests/test_engine_pass_bits_pinned.py -m gpu -x -q
"""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "engine_pass_bits.json")
CTX = 256
SEED = 20261020


def _shape(name, hidden, inter, heads, kv_heads, vocab):
    return G.LlamaShape(name, hidden, inter, 2, heads, kv_heads, vocab, ctx=CTX, bos=256, eos=257)


SHAPES = {"d64": _shape("d64", 256, 768, 4, 2, 512), "d128": _shape("d128", 512, 1024, 4, 2, 512),
          "w320": _shape("w320", 320, 864, 5, 1, 512),                           # tests/test_engine_narrow_widths_gpu.py
          "bigv": _shape("bigv", 256, 512, 4, 2, 4096)}
MODELS = [("d64", "Q8_0"), ("d64", "Q4_0"), ("d64", "Q4_K_M"), ("d128", "Q8_0"), ("d128", "Q4_K_M"), ("w320", "Q8_0"), ("bigv", "Q8_0")]


def tokens_of(n, seed=0):
    r = np.random.Generator(np.random.Philox(key=[SEED, 1000 * seed + n]))
    return [256] + [int(t) for t in r.integers(0, 256, n - 1)]


def _case(cid, model, mix, steps, **opts):
    return dict(id="%s-%s-%s" % (model, mix, cid), model=model, mix=mix, steps=steps, opts=opts)


def _cases():
    out = []
    for model, mix in MODELS:
        out.append(_case("fwd-a", model, mix, [("forward", n, 0) for n in (1, 3, 7, 17, 40, 70)]))
        out.append(_case("fwd-b", model, mix, [("forward", 37, 0), ("forward", 33, 37), ("forward", 1, 40)]))
    at = [("forward", 17, 0), ("forward", 70, 0)]
    for key, val in (("batched_prefill", 0), ("f16_prefill", 0), ("prefill_row_max", 0), ("prefill_fused_split", 0), ("repack", 0), ("repack", 1), ("repack", 2)):
        out.append(_case("opt-%s%d" % (key, val), "d64", "Q8_0", at, **{key: val}))
    out.append(_case("opt-repack2", "d64", "Q4_K_M", at, repack=2))
    for mix in ("Q8_0", "Q4_K_M"):
        out.append(_case("rope", "d128", mix, [("forward", 7, 0), ("forward", 3, 7)], rope_scaling="llama3:8,1,4,64"))
        out.append(_case("kvq8", "d128", mix, [("forward", 3, 0), ("forward", 7, 3), ("forward", 33, 10)], kv_cache="q8_0"))
        out.append(_case("kvq8-batch", "d128", mix, [("prefill", 0, 9), ("prefill", 1, 3), ("prefill", 2, 21), ("decode_batch", (2, 0, 1), True)],
                         kv_cache="q8_0", batch_kv_q8=1, sequences=3))
    for model, mix in (("d64", "Q8_0"), ("d64", "Q4_K_M"), ("d128", "Q8_0"), ("w320", "Q8_0"), ("bigv", "Q8_0")):
        out.append(_case("score", model, mix, [("score", 40, True), ("score", 40, False)], score_rows=16))
        prefills = [("prefill", 0, 7), ("prefill", 1, 17), ("prefill", 2, 3), ("prefill", 3, 40)]
        out.append(_case("batch", model, mix, prefills + [("decode_batch", (1,), True), ("decode_batch", (3, 0, 2), True), ("decode_batch", (0, 2, 3), False)],
                         sequences=4))
        out.append(_case("sample", model, mix, prefills + [("sample", (2, 0, 3))], sequences=4))
        out.append(_case("packed", model, mix, [("prefill", 1, 9), ("forward_batch", (0, 1, 2), (5, 1, 12), (0, 9, 0), True),
                                                ("forward_batch", (2, 0, 1), (12, 5, 1), (12, 5, 10), False)], sequences=4))
    out.append(_case("rowlogits", "d64", "Q8_0", [("generate_ex",)], sequences=4))
    return out


CASES = _cases()
assert len({c["id"] for c in CASES}) == len(CASES)

_files = {}


def model_path(root, model, mix):
    """the model's GGUF file under `root`, written once per process"""
    if (model, mix) not in _files:
        path = os.path.join(str(root), "%s_%s.gguf" % (model, mix.lower()))
        G.make_synthetic_llama(path, SHAPES[model], mix, seed=SEED)
        _files[(model, mix)] = path
    return _files[(model, mix)]


def run_case(c, root):
    """the calls of case c on a fresh engine -> everything they returned, then the cache rows, then two fused steps: a list of arrays"""
    shape = SHAPES[c["model"]]
    eng = E.Engine()
    for k, v in c["opts"].items():
        eng.set_option(k, v)
    eng.load(model_path(root, c["model"], c["mix"]), CTX)
    outs, pos = [], {}                                 # pos[slot]: how many cache rows of the slot the case has written

    def wrote(slot, upto):
        pos[slot] = max(pos.get(slot, 0), upto)

    for i, st in enumerate(c["steps"]):
        kind = st[0]
        if kind == "forward":
            _, n, start = st
            outs.append(eng.forward(tokens_of(n, seed=i), start))
            wrote(0, start + n)
        elif kind == "prefill":
            _, slot, n = st
            outs.append(eng.seq_forward(slot, tokens_of(n, seed=10 + slot), 0))
            wrote(slot, n)
        elif kind == "score":
            _, n, top1 = st
            got = eng.score(tokens_of(n, seed=i), 0, top1=top1)
            outs += list(got) if top1 else [got]
            wrote(0, n)
        elif kind == "decode_batch":
            _, slots, logits = st
            lg, nxt = eng.decode_batch(slots, [40 + 7 * s + i for s in slots], [pos[s] for s in slots], logits=logits)
            outs += ([lg] if logits else []) + [np.array(nxt, np.int32)]
            for s in slots: wrote(s, pos[s] + 1)
        elif kind == "sample":
            _, slots = st
            greedy = E.GenParams(1, 0.0, 40, 0.9, 1.0, 64, 42, 0)
            sampled = E.GenParams(1, 0.8, 8, 0.9, 1.3, 5, 42, 0)
            window = tokens_of(5, seed=77)
            lg, nxt = eng.decode_batch_sample(slots, [40 + 7 * s for s in slots], [pos[s] for s in slots], [greedy, sampled, greedy],
                                              [[], window, []], [0.0, 0.37, 0.0])
            outs += [lg, np.array(nxt, np.int32)]
            for s in slots: wrote(s, pos[s] + 1)
        elif kind == "forward_batch":
            _, slots, lens, starts, logits = st
            lg, nxt = eng.forward_batch(slots, [tokens_of(n, seed=20 + s + i) for s, n in zip(slots, lens)], starts, logits=logits)
            outs += ([lg] if logits else []) + [np.array(nxt, np.int32)]
            for s, n, p0 in zip(slots, lens, starts): wrote(s, p0 + n)
        else:
            assert kind == "generate_ex"               # row 1 is sampled on the host from its own row of logits (top_k 100: not the device sampler's)
            params = [E.GenParams(4, 0.0, 40, 0.9, 1.0, 64, 42, 0), E.GenParams(4, 0.8, 100, 0.9, 1.1, 16, 7, 0), E.GenParams(4, 0.7, 8, 0.9, 1.3, 5, 9, 0)]
            prompts = [tokens_of(7, seed=30), tokens_of(17, seed=31), tokens_of(3, seed=32)]
            gen = eng.generate_batch_ex(prompts, params)
            outs.append(np.array(gen, np.int32))
            for s, p in enumerate(prompts): wrote(s, len(p) + 3)   # (the last generated token is not fed back)
    row = shape.kv_heads * (shape.hidden // shape.heads)
    q8 = c["opts"].get("kv_cache") == "q8_0"
    for slot in sorted(pos):
        for layer in range(shape.layers):
            outs += list(eng.kv_read_q8_slot(slot, layer, 0, pos[slot], row) if q8 and c["opts"].get("batch_kv_q8") else
                         eng.kv_read_q8(layer, 0, pos[slot], row) if q8 else eng.kv_read_slot(slot, layer, 0, pos[slot], row))
    p0 = pos.get(0, 0)
    outs += [eng.decode_fused(300, p0), eng.decode_fused(301, p0 + 1, graph=True)]
    eng.close()
    return outs


def digest(outs):
    h = hashlib.sha256()
    for y in outs:
        h.update(np.ascontiguousarray(y).view(np.uint8).tobytes())
    return h.hexdigest()


def check(c, outs):
    """what must hold of a case's outputs whatever was recorded"""
    for y in outs:
        if y.dtype == np.float32: assert np.isfinite(y).all(), c["id"]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("pass_bits")


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_pass_bits_are_the_recorded_ones(c, golden, root):
    outs = run_case(c, root)
    check(c, outs)
    assert c["id"] in golden, "no digest recorded for %s (tools/record_engine_bits.py)" % c["id"]
    assert digest(outs) == golden[c["id"]]
