"""The batched decode step through the ENGINE where tests/test_batch_decode_gpu.py does not take it: 16 rows, every attention regime and the borders
between them (Model::attention_regime picks by the batch's LARGEST position: single pass below 544, 8 splits from 544, head_dim 128 the matrix-core
form with 32 splits from 3072, other head sizes the walk with 16 splits from 16384), the last position of a context, the prompt-pass option forms,
chunked prefill into a slot, a slot refilled with a shorter sequence, and generate_batch running into the end of the context.

The reference is one O.OracleModel per sequence.  Long sequences are not prefilled: rows [0, start) of every layer's K and V cache are seeded halves of
0.5 N(0, 1) -- windows of one Philox-keyed pool -- written into the engine's slot (Engine.kv_write_slot) and into the oracle's k_cache / v_cache
alike; the steps behind them are teacher-forced on a fixed seeded token stream.  TOL and the clear-margin rule are test_batch_decode_gpu.py's."""
import dataclasses

import numpy as np
import pytest

from ntransformer_amd import gguf as G
from ntransformer_amd import engine as E
from oracle import oracle as O
from test_batch_decode_gpu import TOL, engine_for, oracle_run, prompts_of, step_all
from test_oracle_golden import CASES, golden_model

pytestmark = pytest.mark.gpu
KEY = 20261018
KBAR = 2e-3                   # cache rows against the oracle's: KBAR max(1, |row|max), both sides (test_batch_decode_gpu.py)

_pool = {}
_oracle = {}
_models = {}


def _halves(n, salt):
    """n halves of 0.5 N(0, 1): a window (by `salt`) of one pool drawn once"""
    if "h" not in _pool:
        r = np.random.Generator(np.random.Philox(key=[KEY, 1]))
        _pool["h"] = (0.5 * r.standard_normal(1 << 22)).astype(np.float16).view(np.uint16)
    h = _pool["h"]
    assert n <= h.size
    off = (salt * 104729) % (h.size - n + 1)
    return h[off: off + n]


def seeded_rows(tag, s, layer, side, n, per):
    """rows [0, n) of side 0 (K) / 1 (V) of sequence s's cache in layer `layer`, [n][per] halves"""
    salt = ((sum(tag.encode()) * 16 + s) * 8 + layer) * 2 + side
    return _halves(n * per, salt).reshape(n, per)


def f32(u16):
    return np.asarray(u16).view(np.float16).astype(np.float32)


def rows_close(got, want):
    w = f32(want)
    return float(np.abs(f32(got) - w).max()) <= KBAR * max(1.0, float(np.abs(w).max()))


def check_logits(label, got, nxt, want):
    """the file's rules: logits within TOL, next = the oracle's arg-max wherever its top-two margin exceeds 2 TOL, at most one pair in ten under it"""
    got, nxt, want = np.asarray(got), np.asarray(nxt), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all(), label
    err = float(np.abs(got - want).max())
    top2 = np.sort(want, axis=-1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 2 * TOL
    share = 1.0 - float(clear.mean())
    print(label, "max |dlogit| = %.3g, share of (step, row) pairs under the margin = %.3g" % (err, share))
    assert err <= TOL, (label, err)
    assert share <= 0.1, (label, share)
    assert np.array_equal(nxt[clear], want.argmax(-1)[clear]), label
    return err


def synthetic_model(tmp_path_factory, name, shape, seed):
    if name not in _models:
        path = str(tmp_path_factory.mktemp(name) / (name + "_q8_0.gguf"))
        G.make_synthetic_llama(path, shape, "Q8_0", seed=seed)
        _models[name] = path
    return _models[name]


def oracle_seeded(tag, path, shape, starts, steps):
    """Per sequence s: rows [0, starts[s]) seeded, then `steps` single-token forwards on a seeded token stream.  toks [steps], logits [steps][V],
    k / v [layers][steps][per]: the rows the steps wrote.  Computed once per tag and shared (read only)."""
    if tag not in _oracle:
        per = shape.kv_heads * (shape.hidden // shape.heads)
        seqs = []
        for s, start in enumerate(starts):
            r = np.random.Generator(np.random.Philox(key=[KEY, 100 * sum(tag.encode()) + s]))
            toks = [int(t) for t in r.integers(0, 256, steps)]
            m = O.OracleModel(path, shape.ctx)
            for layer in range(shape.layers):
                m.k_cache[layer][: start * per] = seeded_rows(tag, s, layer, 0, start, per).reshape(-1)
                m.v_cache[layer][: start * per] = seeded_rows(tag, s, layer, 1, start, per).reshape(-1)
            logits = np.stack([m.forward([t], start + i) for i, t in enumerate(toks)])
            cut = slice(start * per, (start + steps) * per)
            seqs.append(dict(start=start, toks=toks, logits=logits, k=[m.k_cache[l][cut].reshape(steps, per).copy() for l in range(shape.layers)],
                             v=[m.v_cache[l][cut].reshape(steps, per).copy() for l in range(shape.layers)]))
        _oracle[tag] = seqs
    return _oracle[tag]


def seeded_engine(tag, path, shape, sequences, seqs, slot_of):
    eng = E.Engine()
    eng.set_option("sequences", sequences)
    eng.load(path, shape.ctx)
    per = shape.kv_heads * (shape.hidden // shape.heads)
    for s, seq in enumerate(seqs):
        if s in slot_of and seq["start"] > 0:
            for layer in range(shape.layers):
                eng.kv_write_slot(slot_of[s], layer, 0, seeded_rows(tag, s, layer, 0, seq["start"], per), seeded_rows(tag, s, layer, 1, seq["start"], per))
    return eng


def whole_caches(eng, sequences, shape, per):
    return {(slot, l): eng.kv_read_slot(slot, l, 0, shape.ctx, per) for slot in range(sequences) for l in range(shape.layers)}


def run_seeded(label, eng, shape, sequences, seqs, rows, slot_of, steps, whole_at=None):
    """`steps` batched steps over the sequences `rows` (in that row order, sequence s in slot slot_of[s]) with every check of the regimes tests against
    the oracle; returns logits [steps][len(seqs)][V] indexed by SEQUENCE"""
    per = shape.kv_heads * (shape.hidden // shape.heads)
    slots = [slot_of[s] for s in rows]
    got = np.zeros((steps, len(rows), seqs[0]["logits"].shape[1]), np.float32)
    nxt = np.zeros((steps, len(rows)), np.int64)
    for i in range(steps):
        poss = [seqs[s]["start"] + i for s in rows]
        before = whole_caches(eng, sequences, shape, per) if i == whole_at else None
        lg, nx = eng.decode_batch(slots, [seqs[s]["toks"][i] for s in rows], poss)
        for j, s in enumerate(rows):
            got[i, s], nxt[i, s] = lg[j], nx[j]
            for layer in range(shape.layers):   # the row this slot wrote, K bar on both sides
                k, v = eng.kv_read_slot(slot_of[s], layer, poss[j], 1, per)
                assert rows_close(k[0], seqs[s]["k"][layer][i]) and rows_close(v[0], seqs[s]["v"][layer][i]), (label, i, s, layer)
        if before is not None:   # nothing but the written rows changed: slots outside the batch bit-unchanged, slots inside but for one row
            after = whole_caches(eng, sequences, shape, per)
            written = dict(zip(slots, poss))
            for (slot, layer), (k0, v0) in before.items():
                k1, v1 = after[(slot, layer)]
                keep = np.ones(shape.ctx, bool)
                if slot in written:
                    keep[written[slot]] = False
                assert np.array_equal(k0[keep], k1[keep]) and np.array_equal(v0[keep], v1[keep]), (label, i, slot, layer)
    check_logits(label, got, nxt, np.stack([q["logits"] for q in seqs], axis=1))
    return got


def regimes_case(label, path, shape, sequences, starts, steps, slots_a, slots_b, whole_at):
    """One batch against its oracles (rows in sequence order, slots slots_a), and again on a second engine with the rows REVERSED in slots slots_b:
    each sequence's logits bit-identical at every step (a regime taken from any one row instead of the largest position would differ between the
    two orders: row 0 is the shortest sequence in one, the longest in the other)."""
    seqs = oracle_seeded(label, path, shape, starts, steps)
    n = len(starts)
    assert sorted(starts)[0] == starts[0] and max(starts) == starts[-1]
    a_of, b_of = dict(zip(range(n), slots_a)), dict(zip(range(n), slots_b))
    eng = seeded_engine(label, path, shape, sequences, seqs, a_of)
    a = run_seeded(label, eng, shape, sequences, seqs, list(range(n)), a_of, steps, whole_at)
    eng.close()
    eng = seeded_engine(label, path, shape, sequences, seqs, b_of)
    b = run_seeded(label + " (rows reversed, other slots)", eng, shape, sequences, seqs, list(range(n))[::-1], b_of, steps)
    eng.close()
    for i in range(steps):
        for s in range(n):
            assert np.array_equal(a[i, s], b[i, s]), (label, i, s, float(np.abs(a[i, s] - b[i, s]).max()))


# ---- a. sixteen rows on the golden models ---------------------------------------------------------------------------------------------------
STEPS16 = 3
ORDER16 = [(5 * j + 3) % 16 for j in range(16)]          # a permutation of the slots that is not the identity


def oracle_sixteen(name, path, z):
    """sixteen seeded prompts of lengths 1 .. 16 (prompt s: the golden prompt's first token + s seeded ids), 3 steps on a seeded token stream"""
    if name not in _oracle:
        seqs = []
        for s in range(16):
            r = np.random.Generator(np.random.Philox(key=[KEY, 1600 + s]))
            prompt = [int(z["prompt"][0])] + [int(t) for t in r.integers(0, 256, s)]
            toks = [int(t) for t in r.integers(0, 256, STEPS16)]
            m = O.OracleModel(path, int(z["ctx"]))
            m.forward(prompt, 0)
            logits = np.stack([m.forward([t], len(prompt) + i) for i, t in enumerate(toks)])
            seqs.append(dict(prompt=prompt, toks=toks, logits=logits, k=m.k_cache, v=m.v_cache))
        _oracle[name] = seqs
    return _oracle[name]


@pytest.mark.parametrize("name,shape,mix", [CASES[0], CASES[2], CASES[3], CASES[4]])
def test_sixteen_rows_match_sixteen_oracle_models(name, shape, mix, tmp_path):
    """sequences = 16: prompts of 1 .. 16 tokens prefilled with seq_forward into slots 0 .. 15 (1 and 3 tokens: the non-batched rotation and store;
    4 and up: the prompt form), 3 teacher-forced decode_batch steps over all 16 slots in the order (5 j + 3) mod 16: logits / next_out by the file's
    rules, every slot's cache rows against its oracle's at the K bar on both sides; the same sequences stepped as four batches of 4 on a second engine
    are within TOL of the oracle too (no bit claim across batch sizes).  Rows 4 .. 15 of the pointer table, of the tokens | positions block and of
    the logits buffer are used here for the first time: a table cut at 4 rows sends rows 4 .. 15 to another sequence's cache.
    Seeds chosen on the CPU with the oracle alone; (step, row) pairs under the 2 TOL margin: 0 of 48 on each of the four models (smallest margin
    4.1e-3, tiny_q8_0)."""
    path, z = golden_model(name, shape, mix, tmp_path)
    seqs = oracle_sixteen("sixteen/" + name, path, z)
    want = np.stack([q["logits"] for q in seqs], axis=1)          # [steps][16][V]
    eng = engine_for(path, z, sequences=16)
    for s, q in enumerate(seqs):
        eng.seq_forward(s, q["prompt"], 0)
    got, nxt = np.zeros_like(want), np.zeros(want.shape[:2], np.int64)
    for i in range(STEPS16):
        lg, nx = eng.decode_batch(ORDER16, [seqs[s]["toks"][i] for s in ORDER16], [len(seqs[s]["prompt"]) + i for s in ORDER16])
        got[i, ORDER16], nxt[i, ORDER16] = lg, nx
    check_logits(name + " 16 rows", got, nxt, want)
    ctx = int(z["ctx"])
    for s, q in enumerate(seqs):
        n = len(q["prompt"]) + STEPS16
        for layer in range(eng.n_layers):
            per = q["k"][layer].size // ctx
            k, v = eng.kv_read_slot(s, layer, 0, n, per)
            assert rows_close(k, q["k"][layer][: n * per].reshape(n, per)) and rows_close(v, q["v"][layer][: n * per].reshape(n, per)), (s, layer)
    eng.close()
    eng = engine_for(path, z, sequences=16)
    for s, q in enumerate(seqs):
        eng.seq_forward(s, q["prompt"], 0)
    for i in range(STEPS16):
        for g in range(4):
            four = ORDER16[4 * g: 4 * g + 4]
            lg, nx = eng.decode_batch(four, [seqs[s]["toks"][i] for s in four], [len(seqs[s]["prompt"]) + i for s in four])
            got[i, four], nxt[i, four] = lg, nx
    check_logits(name + " four batches of 4", got, nxt, want)
    eng.close()


# ---- b. regimes and their borders, head_dim 128 ---------------------------------------------------------------------------------------------
SMALL4K = dataclasses.replace(G.SMALL, name="small4k", layers=2, ctx=4096)
BATCHES = {
    # 16 rows, the largest position 541 -> 544: three single-pass steps, then 8 splits beside a row at position 3
    "b1": dict(starts=[0, 1, 15, 31, 32, 100, 200, 300, 400, 500, 520, 530, 538, 539, 540, 541], steps=4, whole_at=3,
               slots_a=list(range(16)), slots_b=ORDER16),
    # 6 rows, the largest 3068 -> 3073: the 8-split walk, from 3072 the matrix-core form with 32 splits beside rows with fewer positions than splits
    "b2": dict(starts=[0, 7, 543, 544, 1000, 3068], steps=6, whole_at=4, slots_a=[2, 3, 5, 7, 11, 13], slots_b=[9, 0, 15, 4, 12, 1]),
    # 16 rows in all 16 scratch rows at 32 splits; the last row decodes positions 4092 .. 4095, the last of the context
    "b3": dict(starts=[0, 1, 31, 200, 543, 544, 1000, 1500, 2047, 2048, 2600, 3071, 3072, 3500, 4000, 4092], steps=4, whole_at=3,
               slots_a=ORDER16, slots_b=list(range(16))),
}


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_batches_across_the_attention_regimes_match_the_oracle(batch, tmp_path_factory):
    """The `small` shape (head_dim 128, GQA 4) with 2 layers and a 4096-token context, Q8_0, sequences = 16, cache rows seeded.  Per batch (BATCHES):
    at every step logits / next_out by the file's rules and the row each slot wrote at the K bar (K and V); around one step (the first of the new
    regime, or the context's last position) whole caches before and after: slots outside the batch bit-unchanged in every layer, slots inside but
    for the written row; and the batch again with its rows reversed in other slots: every sequence's logits bit-identical at every step, the
    border steps included.  The scratch of row b lies b x the 32-split single-row scratch (header included) behind row 0's: b3 uses all 16 at 32
    splits, a stride without the header or a buffer of 4 rows would put rows' states on each other.
    Seeds chosen on the CPU with the oracle alone; (step, row) pairs under the 2 TOL margin: b1 0 of 64, b2 0 of 36, b3 0 of 64."""
    path = synthetic_model(tmp_path_factory, "small4k", SMALL4K, 20260926)
    regimes_case(batch, path, SMALL4K, 16, **BATCHES[batch])


# ---- c. the other head sizes' second regime -------------------------------------------------------------------------------------------------
TINY16K = dataclasses.replace(G.TINY, name="tiny16k", ctx=16400)


def test_head_dim_64_crosses_16384_positions_in_the_walk_with_16_splits(tmp_path_factory):
    """The `tiny` shape (head_dim 64) with a 16 400-token context, Q8_0, sequences = 3, rows at 0, 600 and 16382, 4 steps: the largest position crosses
    16384 -- 8 -> 16 splits of the per-head walk, never the matrix-core form -- with the bars of the head_dim 128 batches (whole caches around the
    step at 16384).  (step, row) pairs under the 2 TOL margin, found on the CPU: 0 of 12."""
    path = synthetic_model(tmp_path_factory, "tiny16k", TINY16K, 20260930)
    regimes_case("c", path, TINY16K, 3, starts=[0, 600, 16382], steps=4, slots_a=[0, 1, 2], slots_b=[1, 2, 0], whole_at=2)


# ---- d. the option forms --------------------------------------------------------------------------------------------------------------------
OPTION_FORMS = [("batched_prefill", 0), ("f16_prefill", 0), ("prefill_row_max", 0), ("prefill_fused_split", 0), ("repack", 0), ("repack", 1)]
SAME_BITS = {("prefill_row_max", 0), ("prefill_fused_split", 0), ("repack", 0), ("repack", 1)}


@pytest.mark.parametrize("name,shape,mix", [CASES[4], CASES[2]])
def test_batched_steps_under_the_prompt_pass_options(name, shape, mix, tmp_path):
    """decode_batch runs layers_1to1 and the LM head of score(): every prompt-pass option changes its launches.  sequences = 4, the four prompts of
    test_batch_decode_gpu.py, 3 teacher-forced steps within TOL of the four oracles under each of OPTION_FORMS.  Bits: "prefill_row_max" = 0 and
    "prefill_fused_split" = 0 are documented as forward's bits (test_prompt_pass_with_folded_launches_gives_the_same_bits,
    test_gate_and_up_of_two_formats_take_one_silu_form) and "repack" = 1 as the default's (test_one_resident_copy_gives_the_same_bits_as_two): the
    same is asserted of decode_batch against the default engine; "repack" = 0 too -- a batched step of 4 rows reads a matrix through the prompt GEMM
    or, where that does not take its format, the per-token GEMV over the GGUF bytes, neither of which looks at the decode repack below level 2.
    "batched_prefill" = 0 (per-token GEMV) and "f16_prefill" = 0 (the F32 matrix-core form) are other arithmetic: TOL only.
    Then the inheritance case: decode_batch never sets the prompt-pass form itself; after generate_tokens on slot 0, "batched_prefill" = 0 and back
    to 1, both batched calls are within TOL."""
    path, z = golden_model(name, shape, mix, tmp_path)
    seqs = oracle_run(name, path, z)
    want = np.stack([s["logits"] for s in seqs], axis=1)[:3]
    base = engine_for(path, z)
    ref, _ = step_all(base, seqs, [0, 1, 2, 3], steps=3)
    base.close()
    print(name, "defaults: max |dlogit| = %.3g" % float(np.abs(ref - want).max()))
    assert float(np.abs(ref - want).max()) <= TOL
    for key, value in OPTION_FORMS:
        eng = engine_for(path, z, **{key: value})
        got, _ = step_all(eng, seqs, [0, 1, 2, 3], steps=3)
        eng.close()
        err = float(np.abs(got - want).max())
        print(name, "%s = %d: max |dlogit| = %.3g, equal bits: %s" % (key, value, err, np.array_equal(got, ref)))
        assert np.isfinite(got).all() and err <= TOL, (name, key, value, err)
        if (key, value) in SAME_BITS:
            assert np.array_equal(got, ref), (name, key, value, float(np.abs(got - ref).max()))
    eng = engine_for(path, z)
    for s in (1, 2, 3, 0):
        eng.seq_forward(s, seqs[s]["prompt"], 0)
    eng.generate_tokens(seqs[0]["prompt"], 4, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)   # (slot 0: the same prompt rows again)
    args = ([0, 1, 2, 3], [s["fed"][0] for s in seqs], [len(s["prompt"]) for s in seqs])
    for value in (0, 1):
        eng.set_option("batched_prefill", value)
        got, _ = eng.decode_batch(*args)      # (the same step twice: it rewrites its own row)
        err = float(np.abs(got - want[0]).max())
        print(name, "after generate_tokens, batched_prefill = %d: max |dlogit| = %.3g" % (value, err))
        assert err <= TOL, (name, value, err)
    eng.close()


# ---- e. slot life cycle ---------------------------------------------------------------------------------------------------------------------
def test_chunked_prefill_into_a_slot_and_a_slot_refilled_with_a_shorter_sequence(tmp_path):
    """small_q8_0, sequences = 3.
    Chunked prefill: seq_forward(1, prompt[:9], 0) then seq_forward(1, prompt[9:], 9) -- slot 1's rows at the K bar and the returned logits within TOL
    of the oracle's whole prompt; a batched step over slots (1, 0) behind it agrees too.
    Slot reuse, the normal case of continuous batching: slot 2 seeded with 1500 rows and stepped twice beside slot 0 (600 seeded rows), then refilled
    with seq_forward(2, 5 tokens, 0) and stepped three times beside slot 0.  Slot 2's logits are BIT-IDENTICAL to a fresh engine whose slot 2 only ever
    saw the short prompt, beside the same companion in slot 0 at the same positions (there the long sequence lives in slot 1) -- "nothing but its
    own row" (attention_batch.hip) with stale rows behind the new position; the companion is past position 544, so the short row runs in the 8-split
    launch: a stale row entering a split changes bits.  Both are within TOL of their oracles.
    (step, row) pairs under the 2 TOL margin, found on the CPU: 0 of 6."""
    name, shape, mix = CASES[3]
    path, z = golden_model(name, shape, mix, tmp_path)
    ctx = int(z["ctx"])
    per = shape.kv_heads * (shape.hidden // shape.heads)
    prompt = prompts_of(z)[3]
    assert len(prompt) == 14
    m = O.OracleModel(path, ctx)
    want0 = m.forward(prompt, 0)
    eng = engine_for(path, z, sequences=3)
    eng.seq_forward(1, prompt[:9], 0)
    got0 = eng.seq_forward(1, prompt[9:], 9)
    err = float(np.abs(got0 - want0).max())
    print("chunked prefill: max |dlogit| =", err)
    assert err <= TOL
    for layer in range(eng.n_layers):
        k, v = eng.kv_read_slot(1, layer, 0, 14, per)
        assert rows_close(k, m.k_cache[layer][: 14 * per].reshape(14, per)) and rows_close(v, m.v_cache[layer][: 14 * per].reshape(14, per)), layer
    lone = O.OracleModel(path, ctx)
    want1 = np.stack([m.forward([77], 14), lone.forward([99], 0)])
    got1, nx1 = eng.decode_batch([1, 0], [77, 99], [14, 0])
    check_logits("the step behind the chunked prefill", got1, np.array(nx1), want1)
    eng.close()

    # slot reuse at the shape's own context (2048): sequence 0 = the companion (600 rows), 1 = the long one (1500 rows), both seeded; `short` goes
    # in by seq_forward
    ctx = shape.ctx
    starts, pre, post = [600, 1500], 2, 3
    seqs = oracle_seeded("e", path, shape, starts, pre + post)
    r = np.random.Generator(np.random.Philox(key=[KEY, 5]))
    short = [int(z["prompt"][0])] + [int(t) for t in r.integers(0, 256, 4)]
    stream = [int(t) for t in r.integers(0, 256, post)]
    m = O.OracleModel(path, ctx)
    m.forward(short, 0)
    want_short = np.stack([m.forward([t], len(short) + i) for i, t in enumerate(stream)])
    outs = []
    for long_slot in (2, 1):       # the reused slot, then the fresh engine
        eng = seeded_engine("e", path, shape, 3, seqs, {0: 0, 1: long_slot})
        for i in range(pre):
            eng.decode_batch([0, long_slot], [seqs[0]["toks"][i], seqs[1]["toks"][i]], [600 + i, 1500 + i])
        eng.seq_forward(2, short, 0)
        lg, nx = [], []
        for i in range(post):
            a, b = eng.decode_batch([0, 2], [seqs[0]["toks"][pre + i], stream[i]], [600 + pre + i, len(short) + i])
            lg.append(a); nx.append(b)
        eng.close()
        outs.append(np.stack(lg))
        check_logits("slot 2 %s" % ("reused" if long_slot == 2 else "fresh"), outs[-1], np.array(nx),
                     np.stack([seqs[0]["logits"][pre:], want_short], axis=1))
    assert np.array_equal(outs[0][:, 1], outs[1][:, 1]), float(np.abs(outs[0][:, 1] - outs[1][:, 1]).max())
    assert np.array_equal(outs[0][:, 0], outs[1][:, 0])          # (and the companion's)


# ---- f. generate_batch at the end of the context --------------------------------------------------------------------------------------------
def test_generate_batch_stops_each_sequence_at_the_end_of_the_context(tmp_path):
    """tiny_q8_0 (context 256), sequences = 3, prompts of 254, 256 and 5 tokens, max_tokens = 8, stop_at_eos off: a sequence leaves when its position
    reaches the context (the `pos[i] >= max_pos` exit of Engine::generate_batch) -- streams of exactly 1 + 256 - len tokens capped by max_tokens =
    3, 1 and 8, equal to a Python loop of seq_forward + decode_batch that drops a sequence there; no error, gen_tokens = the sum of len - 1, and the
    engine generates again afterwards."""
    name, shape, mix = CASES[0]
    path, z = golden_model(name, shape, mix, tmp_path)
    ctx, n_gen = shape.ctx, 8
    assert ctx == 256
    r = np.random.Generator(np.random.Philox(key=[KEY, 6]))
    prompts = [[int(z["prompt"][0])] + [int(t) for t in r.integers(0, 256, n - 1)] for n in (254, 256, 5)]
    eng = E.Engine()
    eng.set_option("sequences", 3)
    eng.load(path, ctx)
    last = [int(np.argmax(eng.seq_forward(s, p, 0))) for s, p in enumerate(prompts)]
    streams = [[t] for t in last]
    pos = [len(p) for p in prompts]
    while True:
        live = [s for s in range(3) if len(streams[s]) < n_gen and pos[s] < ctx]
        if not live:
            break
        lg, nx = eng.decode_batch(live, [last[s] for s in live], [pos[s] for s in live])
        assert [int(t) for t in lg.argmax(1)] == nx
        for j, s in enumerate(live):
            last[s] = nx[j]
            streams[s].append(nx[j])
            pos[s] += 1
    assert [len(s) for s in streams] == [3, 1, 8]
    assert eng.generate_batch(prompts, n_gen, stop_at_eos=False) == streams
    st = eng.stats()
    assert st.prompt_tokens == 254 + 256 + 5 and st.gen_tokens == sum(len(s) - 1 for s in streams) == 9
    assert eng.generate_batch(prompts, n_gen, stop_at_eos=False) == streams          # ... and again
    eng.close()
