"""GPU tests of the engine on models with head sizes 256, 80 and 96 -- sizes no other engine test loads (64: tiny, w320 / w384; 128: everything else).

  model      hidden  inter  heads / KV heads  head size   attention
  hd256      512     1024   2 / 1             256         the walk's LPR 32 forms, GQA 2; splits at 544 (8) and 16384 (16); the 96 KiB tiled prompt kernel
  hd256mha   512     1024   2 / 2             256         the same, one query head per KV head
  hd80       320     640    4 / 2             80          the generic three-pass kernels in every regime (never split); the causal generic prompt kernel
  hd96       384     768    4 / 1             96          the same, GQA 4

Synthetic Q8_0 models (gguf.make_synthetic_llama: vocabulary 512, 2 layers, context 1024); the oracle is oracle.OracleModel on the same file.  Bars are
tests/test_engine_narrow_widths_gpu.py's: every logits row within TOL = 1e-3 of the oracle's, the greedy choice equal wherever the oracle's top-two
margin exceeds 2 TOL; score() within tests/test_rope_scaling_engine_gpu.py's SCORE_TOL.

What the engine accepts at these sizes: all four load with an F16 cache; kv_cache = q8_0 is refused at load (head size 128 only); the context shift
takes head sizes 64 / 80 / 128, so hd80 shifts and hd256 is refused with the kernel's shape status and an untouched cache; a rope_freqs.weight table
loads at 256 (the walk reads it for both of a thread's pairs).

Run on the MI355X box:  python -m pytest tests/test_engine_head_sizes_gpu.py -m gpu -x -q"""
import dataclasses

import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import kv_ops as KO
from oracle import oracle as O
from rope_ref import mixed_factors, patch_oracle, plain_table, scaled_table
from score_ref import logprob_ref
from test_batch_decode_regimes_gpu import rows_close

pytestmark = pytest.mark.gpu
TOL = 1e-3          # tests/test_engine_narrow_widths_gpu.py
SCORE_TOL = 2e-3    # tests/test_rope_scaling_engine_gpu.py
CTX = 1024
STEPS = 4
SEED = 20261020
THETA = 500000.0
LENGTHS = (1, 3, 7, 40, 70)          # 70: above one 64-row key tile


def shape_of(name, hidden, inter, heads, kv_heads):
    return G.LlamaShape(name, hidden, inter, 2, heads, kv_heads, 512, ctx=CTX, bos=256, eos=257)


SHAPES = {"hd256": shape_of("hd256", 512, 1024, 2, 1), "hd256mha": shape_of("hd256mha", 512, 1024, 2, 2),
          "hd80": shape_of("hd80", 320, 640, 4, 2), "hd96": shape_of("hd96", 384, 768, 4, 1)}
NAMES = sorted(SHAPES)
HD = {n: s.hidden // s.heads for n, s in SHAPES.items()}

_files, _oracle, _seeded = {}, {}, {}


def prompt_of(n):
    r = np.random.Generator(np.random.Philox(key=[SEED, n]))
    return [256] + [int(t) for t in r.integers(0, 256, n - 1)]


def model_file(name, tmp_path_factory, ctx=CTX, **kw):
    """the model's GGUF, written once per (model, context, extra tensors); the weights depend on the seed alone"""
    key = (name, ctx, tuple(sorted(kw)))
    if key not in _files:
        path = str(tmp_path_factory.mktemp(name) / (name + "_q8_0.gguf"))
        G.make_synthetic_llama(path, dataclasses.replace(SHAPES[name], ctx=ctx), "Q8_0", seed=SEED, **kw)
        _files[key] = path
    return _files[key]


def oracle_run(path, key, n_prompt):
    """the oracle's logits of a prompt and of STEPS greedy steps behind it: (fed tokens, logits [1 + STEPS][V]); once per (model, length), read only"""
    k = (key, n_prompt)
    if k not in _oracle:
        m = O.OracleModel(path, CTX)
        lg = [m.forward(prompt_of(n_prompt), 0)]
        fed = []
        for i in range(STEPS):
            fed.append(m.argmax(lg[-1]))
            lg.append(m.forward([fed[-1]], n_prompt + i))
        out = np.stack(lg)
        out.setflags(write=False)
        _oracle[k] = (fed, out)
    return _oracle[k]


def seeded_rows(tag, s, layer, side, n, per):
    """rows [0, n) of side 0 (K) / 1 (V) of sequence s's cache in layer `layer`: [n][per] halves of 0.5 N(0, 1), one Philox key each, drawn once"""
    key = (tag, s, layer, side, n, per)
    if key not in _seeded:
        r = np.random.Generator(np.random.Philox(key=[SEED, ((sum(tag.encode()) * 16 + s) * 8 + layer) * 2 + side]))
        rows = (0.5 * r.standard_normal((n, per), dtype=np.float32)).astype(np.float16).view(np.uint16)
        rows.setflags(write=False)
        _seeded[key] = rows
    return _seeded[key]


def oracle_seeded(tag, path, shape, starts, steps):
    """Per sequence s: rows [0, starts[s]) seeded, then `steps` one-token forwards on a seeded token stream (test_batch_decode_regimes_gpu.py's
    construction with rows of this module): toks, logits [steps][V], k / v [layers][steps][per] = the rows the steps wrote.  Once per tag, read only."""
    if tag not in _oracle:
        per = shape.kv_heads * (shape.hidden // shape.heads)
        seqs = []
        for s, start in enumerate(starts):
            r = np.random.Generator(np.random.Philox(key=[SEED, 100 * sum(tag.encode()) + s]))
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


def engine_for(path, ctx=CTX, **opts):
    eng = E.Engine()
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.load(path, ctx)
    return eng


def check_rows(got, want, what):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    print("%s: max |dlogit| = %.3g (bar %.0e)" % (what, err, TOL))
    assert err <= TOL, (what, err)
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * TOL
    assert np.array_equal(got.argmax(1)[clear], want.argmax(1)[clear]), what


def greedy_steps(eng, path, key, n_prompt, what):
    """the prompt's logits are checked by the caller; here: 4 teacher-forced steps as fused eager, fused hipGraph (the same bits) and one-token forwards"""
    fed, want = oracle_run(path, key, n_prompt)
    rows = {}
    for mode in ("eager", "graph", "launchers"):      # (each mode rewrites the same cache rows with the same tokens)
        rows[mode] = np.stack([eng.forward([t], n_prompt + i) if mode == "launchers" else eng.decode_fused(t, n_prompt + i, graph=mode == "graph")
                               for i, t in enumerate(fed)])
    assert np.array_equal(rows["eager"].view(np.uint32), rows["graph"].view(np.uint32)), what
    check_rows(rows["graph"], want[1:], what + ", fused steps")
    check_rows(rows["launchers"], want[1:], what + ", one-token forwards")


# ------------------------------------------------------------------------------- prompts, greedy steps, score
@pytest.mark.parametrize("name", NAMES)
def test_prompts_and_greedy_steps_match_the_oracle(name, tmp_path_factory):
    """Prompts of 1, 3, 7, 40 and 70 tokens and a chunked one (40 + 30), four greedy steps behind each: fused + hipGraph = fused eager bit for bit, both
    and the one-token forward within TOL of the oracle."""
    path = model_file(name, tmp_path_factory)
    eng = engine_for(path)
    for n in LENGTHS:
        _, want = oracle_run(path, name, n)
        check_rows(eng.forward(prompt_of(n), 0)[None, :], want[:1], "%s prompt of %d" % (name, n))
        greedy_steps(eng, path, name, n, "%s behind %d tokens" % (name, n))
    _, want = oracle_run(path, name, 70)
    eng.forward(prompt_of(70)[:40], 0)
    check_rows(eng.forward(prompt_of(70)[40:], 40)[None, :], want[:1], "%s chunked 40 + 30" % name)
    greedy_steps(eng, path, name, 70, "%s behind 40 + 30 tokens" % name)
    eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_score_matches_the_oracles_rows(name, tmp_path_factory):
    """score() on the 40-token prompt against log-softmax of the oracle's logits at every position"""
    path = model_file(name, tmp_path_factory)
    toks = prompt_of(40)
    m = O.OracleModel(path, CTX)
    trace = {}
    m.forward(toks, 0, trace=trace)
    normed = O.rmsnorm(trace["layer_out"][-1], m.f.f32("output_norm.weight"), m.eps)
    rows = np.stack([m._gemv(m.out_name, normed[t], m.vocab, m.hidden) for t in range(40)])
    want, _ = logprob_ref(rows, toks[1:] + [-1])
    eng = engine_for(path)
    lp = eng.score(toks)
    eng.close()
    err = float(np.abs(lp - want).max())
    print(name, "score: max |dlogprob| = %.3g" % err)
    assert np.isfinite(lp).all() and err <= SCORE_TOL, err


# ------------------------------------------------------------------------------- head size 256 across the regime borders
CTX16K = 16448


@pytest.mark.parametrize("name", ["hd256", "hd256mha"])
def test_head_dim_256_decodes_across_both_regime_borders(name, tmp_path_factory):
    """Context 16448, cache rows seeded in engine and oracle alike (test_batch_decode_regimes_gpu.py's construction): four fused steps from position
    542 (single pass, from 544 the walk with 8 splits) and four from 16382 (from 16384: 16 splits), teacher-forced, every row within TOL."""
    path = model_file(name, tmp_path_factory, ctx=CTX16K)
    shape = dataclasses.replace(SHAPES[name], ctx=CTX16K)
    per = shape.kv_heads * HD[name]
    starts = [542, 16382]
    seqs = oracle_seeded("hs/" + name, path, shape, starts, STEPS)
    eng = engine_for(path, CTX16K)
    for s, seq in enumerate(seqs):
        for layer in range(shape.layers):
            eng.kv_write(layer, 0, seeded_rows("hs/" + name, s, layer, 0, starts[s], per), seeded_rows("hs/" + name, s, layer, 1, starts[s], per))
        got = np.stack([eng.decode_fused(t, starts[s] + i, graph=True) for i, t in enumerate(seq["toks"])])
        check_rows(got, seq["logits"], "%s from position %d" % (name, starts[s]))
        for layer in range(shape.layers):          # the rows the steps wrote
            k, v = eng.kv_read(layer, starts[s], STEPS, per)
            assert rows_close(k, seq["k"][layer]) and rows_close(v, seq["v"][layer]), (name, s, layer)
    eng.close()


@pytest.mark.parametrize("name", ["hd256", "hd256mha"])
def test_head_dim_256_batched_step_of_three_sequences(name, tmp_path_factory):
    """sequences = 3 at positions {0, 543, 600} (the batch's largest position picks 8 splits for all rows, the row at 0 included): one decode_batch
    step against the three oracles, and against each sequence stepped alone on an engine of its own (decode_fused: single pass / 8 splits) within TOL."""
    path = model_file(name, tmp_path_factory)
    shape = SHAPES[name]
    per = shape.kv_heads * HD[name]
    starts = [0, 543, 600]
    tag = "hs3/" + name
    seqs = oracle_seeded(tag, path, shape, starts, 1)
    eng = engine_for(path, sequences=3)
    for s in (1, 2):
        for layer in range(shape.layers):
            eng.kv_write_slot(s, layer, 0, seeded_rows(tag, s, layer, 0, starts[s], per), seeded_rows(tag, s, layer, 1, starts[s], per))
    got, nxt = eng.decode_batch([0, 1, 2], [q["toks"][0] for q in seqs], starts)
    eng.close()
    want = np.stack([q["logits"][0] for q in seqs])
    check_rows(got, want, name + " batched step")
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * TOL
    assert np.array_equal(np.array(nxt)[clear], want.argmax(1)[clear])
    solo = engine_for(path)
    for s, q in enumerate(seqs):
        for layer in range(shape.layers):
            if starts[s]:
                solo.kv_write(layer, 0, seeded_rows(tag, s, layer, 0, starts[s], per), seeded_rows(tag, s, layer, 1, starts[s], per))
        alone = solo.decode_fused(q["toks"][0], starts[s], graph=True)
        d = float(np.abs(got[s] - alone).max())
        print(name, "row", s, "batched - alone: max |dlogit| = %.3g" % d)
        assert d <= TOL, (name, s, d)
    solo.close()


# ------------------------------------------------------------------------------- what these head sizes do not take
@pytest.mark.parametrize("name", NAMES)
def test_the_8_bit_cache_is_refused_at_load(name, tmp_path_factory):
    eng = E.Engine()
    eng.set_option("kv_cache", "q8_0")
    with pytest.raises(_lib.NtkError) as e:
        eng.load(model_file(name, tmp_path_factory), CTX)
    assert e.value.status == -2 and "kv_cache=q8_0 needs head_dim 128" in str(e.value) and "head_dim %d" % HD[name] in str(e.value)
    eng.close()


def test_context_shift_is_refused_at_256_and_leaves_the_cache_alone(tmp_path_factory):
    """Engine.kv_shift on hd256: NTK_E_SHAPE from ntk_kv_shift (head sizes 64 / 80 / 128), every layer's cache bit-unchanged, and the next decode step
    still the oracle's"""
    path = model_file("hd256", tmp_path_factory)
    fed, want = oracle_run(path, "hd256", 40)
    eng = engine_for(path)
    eng.forward(prompt_of(40), 0)
    before = [eng.kv_read(l, 0, CTX, 256) for l in range(2)]
    with pytest.raises(_lib.NtkError) as e:
        eng.kv_shift(0, 0, 8, 40)
    assert e.value.status == -2 and "kv_shift" in str(e.value)
    for l in range(2):
        k, v = eng.kv_read(l, 0, CTX, 256)
        assert np.array_equal(k, before[l][0]) and np.array_equal(v, before[l][1]), l
    check_rows(eng.decode_fused(fed[0], 40, graph=True)[None, :], want[1:2], "hd256 step behind the refused shift")
    eng.close()


def test_context_shift_at_head_dim_80(tmp_path_factory):
    """hd80 shifts: rows [8, 40) of every layer move to [0, 32), K re-rotated -- against kv_ops.shift_f16_ref at test_kv_shift_f16_against_the_checker's
    bar, V rows bit for bit, everything outside the destination rows unchanged; the step behind the shift equals the step on a cache written from the
    checker."""
    path = model_file("hd80", tmp_path_factory)
    hd, row = 80, 160
    a = engine_for(path)
    a.forward(prompt_of(40), 0)
    k0 = np.stack([a.kv_read(l, 0, CTX, row)[0] for l in range(2)])
    v0 = np.stack([a.kv_read(l, 0, CTX, row)[1] for l in range(2)])
    assert a.kv_shift(0, 0, 8, 40) == 32
    k1 = np.stack([a.kv_read(l, 0, CTX, row)[0] for l in range(2)])
    v1 = np.stack([a.kv_read(l, 0, CTX, row)[1] for l in range(2)])
    want_k, want_v = KO.shift_f16_ref(k0, v0, 8, 0, 32, hd, inv_freq=plain_table(hd, THETA))
    assert np.array_equal(v1, want_v)
    assert np.array_equal(k1[:, 32:], k0[:, 32:])
    err = np.abs(k1[:, :32].view(np.float16).astype(np.float64) - want_k[:, :32].view(np.float16).astype(np.float64))
    bar = 2.0 ** -10 * KO.pair_max(k0[:, 8:40].view(np.float16), hd) + 2.0 ** -24
    print("hd80 shift: worst err / bar = %.3f" % float((err / bar).max()))
    assert (err <= bar).all()
    c = engine_for(path)
    for l in range(2):
        c.kv_write(l, 0, want_k[l, :32], want_v[l, :32])
    la, lc = a.decode_fused(77, 32, graph=True), c.decode_fused(77, 32, graph=True)
    assert np.isfinite(la).all() and float(np.abs(la - lc).max()) <= TOL
    a.close(); c.close()


# ------------------------------------------------------------------------------- a frequency table at 256
def test_a_rope_freqs_table_at_head_dim_256(tmp_path_factory):
    """hd256 with a rope_freqs.weight tensor over all 128 pairs: the load takes it, prompt passes and fused steps match the table-aware oracle
    (tests/test_rope_scaling_engine_gpu.py's construction), and the factors matter (the plain oracle is 10 TOL away)."""
    factors = mixed_factors(256, 15)
    path = model_file("hd256", tmp_path_factory, rope_freqs=factors)
    tab = scaled_table(256, THETA, factors)
    toks = prompt_of(70)
    plain = O.OracleModel(path, CTX).forward(toks[:40], 0)
    with pytest.MonkeyPatch.context() as mp:
        patch_oracle(mp, tab)
        m = O.OracleModel(path, CTX)
        want = {n: O.OracleModel(path, CTX).forward(toks[:n], 0) for n in (3, 70)}
        lg = [m.forward(toks[:40], 0)]
        fed = []
        for i in range(STEPS):
            fed.append(m.argmax(lg[-1]))
            lg.append(m.forward([fed[-1]], 40 + i))
    assert float(np.abs(lg[0] - plain).max()) >= 10 * TOL          # the guard
    eng = engine_for(path)
    assert eng.rope_factors == 128
    for n in (3, 70):          # the per-pair rotation; the rows form across a key tile
        check_rows(eng.forward(toks[:n], 0)[None, :], want[n][None, :], "hd256 + table, prompt of %d" % n)
    check_rows(eng.forward(toks[:40], 0)[None, :], lg[0][None, :], "hd256 + table, prompt of 40")
    for graph in (False, True):
        got = np.stack([eng.decode_fused(t, 40 + i, graph=graph) for i, t in enumerate(fed)])
        check_rows(got, np.stack(lg[1:]), "hd256 + table, fused steps, graph %d" % graph)
    eng.close()
