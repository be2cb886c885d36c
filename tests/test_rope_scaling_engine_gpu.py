"""RoPE frequency scaling through the engine on the GPU: synthetic models whose GGUF carries rope_freqs.weight (and, one variant, linear scaling) against
an oracle that rotates with the same table -- OracleModel.forward calls the module-level oracle.rope, which is replaced by tests/rope_ref.py's rope_ref
bound to the model's table and scale (rope_ref is made a reference by tests/test_rope_scaling_cpu.py).

Models (written by make_synthetic_llama into a temporary directory, context 128):
  t64      the tiny shape of the golden files (hidden 256, 2 layers, 4 / 2 heads, head_dim 64), Q8_0, a seeded factor table over all pairs
  t64lin   the same with linear scaling of factor 4 on top (freq_scale 0.25)
  t128     hidden 256, 2 layers, 2 / 1 heads, head_dim 128, Q4_K_M, a seeded factor table
  t128q8   the same shape with Q8_0 weights (the weight format of tests/test_kv_q8_gpu.py's models): the 8-bit KV cache's logit bars are held on it
Bars are the project's: logits within 1e-3 of the oracle for these shallow models, score within 2e-3.

THE GUARD (test_engine_matches_the_table_aware_oracle_in_every_prompt_form): on every model the table-aware oracle's logits differ from the plain
oracle's by at least ten times the bar at every tested position but position 0 (where nothing rotates): an engine that ignored the file's factors --
the engine before this feature -- matches the plain oracle and fails every test below.  Factor seeds were chosen on the CPU, with the oracle alone.

kv_cache=q8_0 (test 4 of the issue): tests/test_kv_q8_gpu.py holds no logits bar between a q8_0 and an F16 engine; its engine bars are the cache contents
after a prompt pass (V blocks bit-exact, K quants within one step and scales within 2^-10 of the numpy quantiser of the reference rotation, > 99 % of
the quants equal) and fused against unfused steps at 1e-3 at positions 540 and 3068.  test_q8_kv_cache_on_a_scaled_model asserts the cache bars, and
holds the logits -- q8_0 against F16, fused against unfused, prompt passes and 8 decode steps -- to 3 x what the same engines show on the identical file
under rope_scaling=none; the reasoning, and why the absolute 1e-3 is not used at 40 positions (the unscaled engine misses it there), are in that test.

Run on the MI355X box:  python -m pytest tests/test_rope_scaling_engine_gpu.py -m gpu -x -q"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from ntransformer_amd import _lib, kv_q8
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import kv_ops as KO
from oracle import oracle as O
from rope_ref import mixed_factors, patch_oracle, plain_table, rope_ref, scaled_table
from score_ref import logprob_ref

pytestmark = pytest.mark.gpu
TOL, SCORE_TOL, CTX, THETA = 1e-3, 2e-3, 128, 500000.0
T64 = G.LlamaShape("tiny", 256, 512, 2, 4, 2, 512, ctx=256, bos=256, eos=257)
T128 = G.LlamaShape("tiny128", 256, 512, 2, 2, 1, 512, ctx=256, bos=256, eos=257)
MODELS = {"t64": (T64, "Q8_0", 64, 11, None), "t64lin": (T64, "Q8_0", 64, 12, 4.0), "t128": (T128, "Q4_K_M", 128, 13, None),
          "t128q8": (T128, "Q8_0", 128, 14, None)}
LENGTHS = (1, 3, 4, 37, 70)
N_STEPS = 8


def prompt_tokens(n=70, seed=31):
    r = np.random.Generator(np.random.Philox(key=[20261020, seed]))
    return [256] + [int(t) for t in r.integers(0, 256, n - 1)]


def factors_of(name):
    shape, mix, hd, seed, linear = MODELS[name]
    return mixed_factors(hd, seed)


_files, _refs = {}, {}


def model_file(name, tmp_path_factory, **kw):
    """the model's GGUF (written once per session); kw: another rope_freqs / rope_scaling, under its own key"""
    key = (name, json.dumps({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in kw.items()}, sort_keys=True))
    if key not in _files:
        shape, mix, hd, seed, linear = MODELS[name]
        args = dict(rope_freqs=factors_of(name), rope_scaling={"type": "linear", "factor": linear} if linear else None)
        args.update(kw)
        path = str(tmp_path_factory.mktemp(name) / "model.gguf")
        G.make_synthetic_llama(path, shape, mix, seed=20261020, **args)
        _files[key] = path
    return _files[key]


def table_of(name):
    shape, mix, hd, seed, linear = MODELS[name]
    return scaled_table(hd, THETA, factors_of(name)), (np.float32(1.0) / np.float32(linear) if linear else 1.0)


def oracle_ref(name, tmp_path_factory):
    """The table-aware oracle on the model, once per session, read only: logits behind prompts of LENGTHS tokens, N_STEPS teacher-forced decode steps
    behind the 37-token prompt, the logits at every position of that prompt (score), the chunked 37 + 33 pass -- and the PLAIN oracle's prompt logits."""
    if name not in _refs:
        path = model_file(name, tmp_path_factory)
        tab, fscale = table_of(name)
        toks = prompt_tokens()
        ref = dict(path=path, tokens=toks, tab=tab, fscale=fscale)
        ref["plain"] = {T: O.OracleModel(path, CTX).forward(toks[:T], 0) for T in LENGTHS}
        with pytest.MonkeyPatch.context() as mp:
            patch_oracle(mp, tab, fscale)
            ref["prompt"] = {T: O.OracleModel(path, CTX).forward(toks[:T], 0) for T in LENGTHS}
            m = O.OracleModel(path, CTX)
            trace = {}
            lg = m.forward(toks[:37], 0, trace=trace)
            normed = O.rmsnorm(trace["layer_out"][-1], m.f.f32("output_norm.weight"), m.eps)
            ref["all37"] = np.stack([m._gemv(m.out_name, normed[t], m.vocab, m.hidden) for t in range(37)])
            ref["k37"], ref["v37"] = [a.copy() for a in m.k_cache], [a.copy() for a in m.v_cache]
            fed, steps = [int(np.argmax(lg))], []
            for i in range(N_STEPS):
                steps.append(m.forward([fed[-1]], 37 + i))
                fed.append(int(np.argmax(steps[-1])))
            ref["fed"], ref["steps"] = fed[:N_STEPS], steps
            m2 = O.OracleModel(path, CTX)
            m2.forward(toks[:37], 0)
            ref["chunked"] = m2.forward(toks[37:70], 37)
        _refs[name] = ref
    return _refs[name]


def engine_for(path, ctx=CTX, **opts):
    e = E.Engine()
    for k, v in opts.items():
        e.set_option(k, v)
    e.load(path, ctx)
    return e


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ------------------------------------------------------------------------------------------------ 1, 2: the guard and the prompt forms
@pytest.mark.parametrize("name", sorted(MODELS))
def test_engine_matches_the_table_aware_oracle_in_every_prompt_form(name, tmp_path_factory):
    """Prompt passes of 1 and 3 tokens (the per-pair rotation), 4 and 37 (the rows form with the fused store), 70 (beyond the 64-token border of
    prefill_fused_split) and a chunked prefill 37 + 33."""
    ref = oracle_ref(name, tmp_path_factory)
    for T in LENGTHS[1:]:
        gap = dist(ref["prompt"][T], ref["plain"][T])
        print(name, "T", T, "table-aware oracle - plain oracle: max |dlogit| =", gap)
        assert gap >= 10 * TOL, (name, T, gap)                       # THE GUARD: the factors matter at every tested length
    assert dist(ref["chunked"], ref["prompt"][70]) <= 1e-4          # (the oracle itself: chunked = whole)
    e = engine_for(ref["path"])
    info = e.rope_info()
    shape, mix, hd, seed, linear = MODELS[name]
    assert info["rope_factors"] == hd // 2 and info["rope_scaling_type"] == ("linear" if linear else "none") and info["rope_theta"] == THETA
    assert info["rope_freq_scale"] == (0.25 if linear else 1.0) and e.rope_factors == hd // 2
    for T in LENGTHS:
        got = e.forward(ref["tokens"][:T], 0)
        err = dist(got, ref["prompt"][T])
        print(name, "T", T, "engine - table-aware oracle: max |dlogit| =", err)
        assert np.isfinite(got).all() and err <= TOL, (name, T, err)
    e.forward(ref["tokens"][:37], 0)
    err = dist(e.forward(ref["tokens"][37:70], 37), ref["chunked"])
    print(name, "chunked 37 + 33: max |dlogit| =", err)
    assert err <= TOL
    lp = e.score(ref["tokens"][:37])
    want, _ = logprob_ref(ref["all37"], ref["tokens"][1:37] + [-1])
    assert np.abs(lp - want).max() <= SCORE_TOL, float(np.abs(lp - want).max())
    e.close()


# ------------------------------------------------------------------------------------------------ 3: decode steps
@pytest.mark.parametrize("mode", ["fused_graph", "fused_eager", "unfused"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_eight_decode_steps_behind_a_prompt(name, mode, tmp_path_factory):
    """fused + graph, graph = 0, and fused = 0 (the 1:1 launch sequence: a one-token forward), against one-token forwards of the table-aware oracle"""
    ref = oracle_ref(name, tmp_path_factory)
    e = engine_for(ref["path"])
    e.forward(ref["tokens"][:37], 0)
    for i, tok in enumerate(ref["fed"]):
        got = e.forward([tok], 37 + i) if mode == "unfused" else e.decode_fused(tok, 37 + i, graph=(mode == "fused_graph"))
        err = dist(got, ref["steps"][i])
        assert np.isfinite(got).all() and err <= TOL, (name, mode, i, err)
    if mode == "fused_graph":       # ... and the generate loop under the options: greedy tokens of fused + graph equal those of fused = 0 unless a near tie flips
        a = e.generate_tokens(ref["tokens"][:37], N_STEPS, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
        want = [int(np.argmax(ref["prompt"][37]))] + [int(np.argmax(s)) for s in ref["steps"][:N_STEPS - 1]]
        margins = [float(np.sort(s)[-1] - np.sort(s)[-2]) for s in [ref["prompt"][37]] + ref["steps"][:N_STEPS - 1]]
        if min(margins) > 2 * TOL:
            assert a == want
    e.close()


# ------------------------------------------------------------------------------------------------ 4: the 8-bit KV cache
Q8_VS_F16_FACTOR = 3.0


@pytest.mark.parametrize("name", ["t128q8", "t128"])
def test_q8_kv_cache_on_a_scaled_model(name, tmp_path_factory):
    """The 8-bit KV cache under a factor table, on both hd-128 models (t128q8: Q8_0 weights, the weight format of tests/test_kv_q8_gpu.py's own models).
    Cache contents at that file's bars.  Logits, two distances, each over the 37-token pass, the 3-token pass and 8 decode steps behind them:
      q8_0 engine - F16 engine            (the fused decode path and the prompt path of a scaled q8_0 engine, held to the scaled F16 engine, which the
                                           other tests hold to the oracle)
      q8_0 fused step - q8_0 unfused step (8 steps)
    each within Q8_VS_F16_FACTOR = 3 x the LARGEST value the same engines show on the identical file loaded with rope_scaling=none, over the same
    passes and steps.  Why that bar: both distances are rounding noise of the cached K and V carried into the logits (the 8-bit quantisation; the half
    rounding of the prompt path's one-layer F16 image).  A rotation preserves the norm of every pair, so the scaled and the unscaled model quantise values
    of the same magnitudes, block by block, and the two sets of distances are draws from one distribution -- maxima over 512 logits, whose largest over
    ten passes varies by tens of per cent between two such sets, not by multiples.  A q8_0 path that rotated otherwise than the F16 path (another table,
    q and k apart, one launch without the table) would be off by the guard's distance, 0.2 and more, far beyond 3 x the noise.
    NOT used: test_kv_q8_gpu.py's absolute 1e-3 for fused against unfused steps.  That bar was set at positions 540 and 3068 over seeded caches; 40 rows
    average the image's rounding less, and the engine misses it here WITHOUT scaling: measured on the MI355X, t128q8, 8 steps, rope_scaling=none:
    1.23e-3 7.9e-4 6.7e-4 6.8e-4 6.6e-4 7.8e-4 9.5e-4 8.0e-4; with the file's factors: 7.0e-4 7.6e-4 5.7e-4 6.8e-4 1.03e-3 5.3e-4 6.6e-4 6.3e-4 (t128,
    Q4_K_M, logits up to 8: 1.8e-3 .. 4.0e-3 without, 1.8e-3 .. 2.9e-3 with).  q8_0 - F16, largest of the ten: t128q8 0.026 without, 0.025 with; t128
    0.25 without, 0.26 with."""
    ref = oracle_ref(name, tmp_path_factory)
    tab, fscale = ref["tab"], ref["fscale"]
    nh, nkv, hd, per = 2, 1, 128, 128
    q = engine_for(ref["path"], kv_cache="q8_0")
    f = engine_for(ref["path"])
    scaled, fused_unfused = [], []
    q.kv_inputs_capture(0)
    for start, T in ((0, 37), (37, 3)):          # the fused RoPE + 8-bit store launch; ntk_rope_tab + ntk_kv_store_q8
        toks = ref["tokens"][start:start + T]
        lq, lf = q.forward(toks, start), f.forward(toks, start)
        scaled.append(dist(lq, lf))
        assert np.isfinite(lq).all()
        k_in, v_in = q.kv_inputs_read(T, per)
        got_k, got_v = q.kv_read_q8(0, start, T, per)
        assert np.array_equal(got_v, kv_q8.to_blocks(*kv_q8.quantize_q8_0(v_in)))
        rk = np.stack([rope_ref(np.zeros(nh * hd, np.float32), k_in[t], [start + t], nh, nkv, hd, tab, fscale)[1] for t in range(T)])
        wd, wq = kv_q8.quantize_q8_0(rk)
        gd, gq = kv_q8.from_blocks(got_k)
        assert np.abs(gq.astype(np.int32) - wq.astype(np.int32)).max() <= 1
        assert (np.abs(gd.astype(np.float64) - wd.astype(np.float64)) <= 2.0 ** -10 * wd.astype(np.float64)).all()
        assert float((gq == wq).mean()) > 0.99
        plain = np.stack([O.rope(np.zeros(nh * hd, np.float32), k_in[t], [start + t], nh, nkv, hd, THETA)[1] for t in range(T)])
        assert float((kv_q8.quantize_q8_0(plain)[1] == gq).mean()) < 0.9          # (not the unscaled rotation's quants)
    # decode: the 1:1 step (ntk_rope_tab + ntk_kv_store_q8) and the fused step (ntk_attention_decode_q8 given the table) rotate and store the SAME row --
    # layer 0's k of a token depends on nothing but the token -- so the two cache rows agree at the cache bars above; eager = graph bit for bit
    for i, tok in enumerate(ref["fed"]):
        plain = q.forward([tok], 40 + i)
        row_k, row_v = q.kv_read_q8(0, 40 + i, 1, per)
        k_in, _ = q.kv_inputs_read(1, per)
        eager = q.decode_fused(tok, 40 + i, False)
        graph = q.decode_fused(tok, 40 + i, True)
        assert np.isfinite(eager).all() and np.isfinite(plain).all() and np.array_equal(eager, graph)
        got_k, got_v = q.kv_read_q8(0, 40 + i, 1, per)
        (d1, q1), (d2, q2) = kv_q8.from_blocks(row_k), kv_q8.from_blocks(got_k)
        assert np.abs(q1.astype(np.int32) - q2.astype(np.int32)).max() <= 1 and float((q1 == q2).mean()) > 0.99
        assert (np.abs(d1.astype(np.float64) - d2.astype(np.float64)) <= 2.0 ** -10 * d1.astype(np.float64)).all()
        assert np.abs(kv_q8.from_blocks(row_v)[1].astype(np.int32) - kv_q8.from_blocks(got_v)[1].astype(np.int32)).max() <= 1
        wq = kv_q8.quantize_q8_0(rope_ref(np.zeros(nh * hd, np.float32), k_in[0], [40 + i], nh, nkv, hd, tab, fscale)[1][None, :])[1]
        assert np.abs(q2.astype(np.int32) - wq.astype(np.int32)).max() <= 1
        fused_unfused.append(dist(eager, plain))
        scaled.append(dist(eager, f.decode_fused(tok, 40 + i, True)))
    q.close(); f.close()
    # the same passes and steps on the identical file with rope_scaling=none
    qn, fn = engine_for(ref["path"], kv_cache="q8_0", rope_scaling="none"), engine_for(ref["path"], rope_scaling="none")
    unscaled = [dist(qn.forward(ref["tokens"][s:s + T], s), fn.forward(ref["tokens"][s:s + T], s)) for s, T in ((0, 37), (37, 3))]
    fused_unfused_none = []
    for i, tok in enumerate(ref["fed"]):
        plain = qn.forward([tok], 40 + i)
        fused = qn.decode_fused(tok, 40 + i, True)
        fused_unfused_none.append(dist(fused, plain))
        unscaled.append(dist(fused, fn.decode_fused(tok, 40 + i, True)))
    qn.close(); fn.close()
    fmt = lambda xs: " ".join("%.3g" % x for x in xs)
    print(name, "q8_0 fused - unfused, 8 steps, with the file's factors:", fmt(fused_unfused))
    print(name, "q8_0 fused - unfused, 8 steps, with rope_scaling=none:  ", fmt(fused_unfused_none), "-> bar %.3g" % (Q8_VS_F16_FACTOR * max(fused_unfused_none)))
    print(name, "q8_0 - f16 with the file's factors (37-token pass, 3-token pass, 8 steps):", fmt(scaled))
    print(name, "q8_0 - f16 with rope_scaling=none  (the same):", fmt(unscaled), "-> bar %.3g" % (Q8_VS_F16_FACTOR * max(unscaled)))
    assert max(fused_unfused) <= Q8_VS_F16_FACTOR * max(fused_unfused_none), (fused_unfused, fused_unfused_none)
    assert max(scaled) <= Q8_VS_F16_FACTOR * max(unscaled), (scaled, unscaled)


# ------------------------------------------------------------------------------------------------ 5: sequence slots, the packed pass, shared weights
@pytest.mark.parametrize("name", ["t64", "t128"])
def test_sequence_slots_packed_pass_and_shared_weights(name, tmp_path_factory):
    ref = oracle_ref(name, tmp_path_factory)
    shape, mix, hd, seed, linear = MODELS[name]
    row = shape.kv_heads * hd
    toks = ref["tokens"]
    prompts = [toks[:37], toks[:5], [256] + toks[40:56], toks[:1]]
    solo = engine_for(ref["path"])
    e = engine_for(ref["path"], sequences=4)
    steps = []
    for s, p in enumerate(prompts):
        want = solo.forward(p, 0)
        got = e.seq_forward(s, p, 0)
        assert dist(got, want) <= TOL, (name, s)
        steps.append(solo.decode_fused(7 + s, len(p), graph=True))
    assert dist(e.seq_forward(0, prompts[0], 0), ref["prompt"][37]) <= TOL
    lg, _ = e.decode_batch([0, 1, 2, 3], [7, 8, 9, 10], [len(p) for p in prompts])
    for s in range(4):
        assert dist(lg[s], steps[s]) <= TOL, (name, s, dist(lg[s], steps[s]))
    # forward_batch: a segment alone in a pass = seq_forward's cache rows, bit for bit
    a = engine_for(ref["path"], sequences=4)
    for slot, p in ((2, prompts[0]), (1, prompts[1]), (3, prompts[1][:3])):
        got, _ = a.forward_batch([slot], [p], [0])
        want = e.seq_forward(slot, p, 0)
        assert dist(got[0], want) <= TOL
        for layer in range(shape.layers):
            (ka, va), (kb, vb) = a.kv_read_slot(slot, layer, 0, len(p), row), e.kv_read_slot(slot, layer, 0, len(p), row)
            assert np.array_equal(ka, kb) and np.array_equal(va, vb), (name, slot, layer)
    got, _ = a.forward_batch([0, 1, 2], [prompts[0], prompts[1], prompts[2]], [0, 0, 0])      # a 3-segment pass
    for s in range(3):
        assert dist(got[s], solo.forward(prompts[s], 0)) <= TOL, (name, s)
    assert dist(got[0], ref["prompt"][37]) <= TOL
    a.close(); e.close()
    # a sharing sequence rotates as its source does: the solo bits
    want = solo.forward(prompts[0], 0)
    want_step = solo.decode_fused(7, 37, graph=True)
    b = E.Engine()
    b.set_option("rope_scaling", "none")          # (its own rope options do not apply: the source's table and scale do)
    b.load_shared(solo, CTX)
    assert b.rope_factors == hd // 2
    assert np.array_equal(b.forward(prompts[0], 0), want) and np.array_equal(b.decode_fused(7, 37, graph=True), want_step)
    b.close(); solo.close()


# ------------------------------------------------------------------------------------------------ 6: the context shift
def test_kv_shift_on_a_scaled_model(tmp_path_factory):
    """The construction of tests/test_kv_ops_engine_gpu.py on the scaled t128 model (linear scaling 4 on top of the factors, written here): shifted keys are
    the keys the model caches at the new positions; the step behind the shift against a cache written from the checker given the model's table and scale."""
    path = model_file("t128", tmp_path_factory, rope_scaling={"type": "linear", "factor": 4.0})
    tab, fscale, hd, row = scaled_table(128, THETA, factors_of("t128")), 0.25, 128, 128
    toks = prompt_tokens(48, seed=32)
    r = np.random.Generator(np.random.Philox(key=[20261020, 33]))
    a, b = engine_for(path), engine_for(path)
    a.forward(toks[:40], 0)
    k0 = np.stack([a.kv_read(l, 0, CTX, row)[0] for l in range(2)])
    v0 = np.stack([a.kv_read(l, 0, CTX, row)[1] for l in range(2)])
    assert a.kv_shift(0, 0, 8, 40) == 32
    ka, va = a.kv_read(0, 0, 32, row)
    b.kv_inputs_capture(0)
    b.forward(toks[8:40] + [int(t) for t in r.integers(0, 256, 8)], 0)
    kb, vb = b.kv_read(0, 0, 32, row)
    k_in, _ = b.kv_inputs_read(32, row)
    assert np.array_equal(va, vb)
    err = np.abs(ka.view(np.float16).astype(np.float64) - kb.view(np.float16).astype(np.float64))
    bar = 2.0 ** -9 * KO.pair_max(k_in, hd) + 2.0 ** -24
    print("shift vs the scaled model's RoPE: worst err / bar = %.3f" % float((err / bar).max()))
    assert (err <= bar).all()
    # the unscaled rotation would not do: the plain checker lands elsewhere
    plain_k, _ = KO.shift_f16_ref(k0, v0, 8, 0, 32, hd, inv_freq=plain_table(hd, THETA))
    assert not (np.abs(plain_k[0, :32].view(np.float16).astype(np.float64) - kb.view(np.float16).astype(np.float64)) <= bar).all()
    # the step behind the shift
    want_k, want_v = KO.shift_f16_ref(k0, v0, 8, 0, 32, hd, inv_freq=tab, freq_scale=fscale)
    c = engine_for(path)
    for l in range(2):
        c.kv_write(l, 0, want_k[l, :32], want_v[l, :32])
    la, lc = a.decode_fused(77, 32, graph=True), c.decode_fused(77, 32, graph=True)
    assert np.isfinite(la).all() and dist(la, lc) <= TOL
    a.close(); b.close(); c.close()


# ------------------------------------------------------------------------------------------------ 7: tensor parallelism, two processes
def test_two_tensor_parallel_ranks_match_the_table_aware_oracle(tmp_path_factory, tmp_path):
    from test_tp_gpu import RANK_SCRIPT
    ref = oracle_ref("t64", tmp_path_factory)
    d = str(tmp_path)
    json.dump({"prompt": ref["tokens"][:37], "fed": ref["fed"][:4], "run_id": "rope"}, open(os.path.join(d, "job.json"), "w"))
    script = os.path.join(d, "rank.py")
    open(script, "w").write(RANK_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, script, ROOT, str(k), "2", ref["path"], str(CTX), d], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for k in range(2)]
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        outs.append(o.decode(errors="replace"))
    for k, p in enumerate(procs):
        assert p.returncode == 0, outs[k][-2000:]
    want = np.stack([ref["prompt"][37]] + ref["steps"][:4])
    lgs = [np.load(os.path.join(d, "logits_%d.npy" % k)) for k in range(2)]
    for k in range(2):
        assert json.load(open(os.path.join(d, "done_%d.json" % k)))["tp_error"] == 0
        assert dist(lgs[k], want) <= TOL, ("vs the table-aware oracle", k, dist(lgs[k], want))
    assert np.array_equal(lgs[0], lgs[1])


# ------------------------------------------------------------------------------------------------ 8: options
def run_tokens(e, toks):
    return [e.forward(toks[:37], 0), e.forward(toks[37:40], 37), e.decode_fused(5, 40, graph=True), e.decode_fused(6, 41, graph=False)]


def same_bits(xs, ys):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(xs, ys))


def test_rope_options_equal_files_written_with_those_values(tmp_path_factory):
    toks = prompt_tokens()
    l3 = G.llama3_rope_factors(64, THETA, 8.0, 1.0, 4.0, 64)
    assert (l3 == 1.0).any() and (l3 == 8.0).any() and ((l3 > 1.0) & (l3 < 8.0)).any()
    plain_path = model_file("t64", tmp_path_factory, rope_freqs=None, rope_scaling=None)
    # a synthetic-style load with rope_scaling=llama3:8,1,4,64 = a file that carries llama3_rope_factors(..., orig_ctx=64)
    a = engine_for(model_file("t64", tmp_path_factory, rope_freqs=l3, rope_scaling=None))
    b = engine_for(plain_path, rope_scaling="llama3:8,1,4,64")
    want = run_tokens(a, toks)
    assert same_bits(run_tokens(b, toks), want)
    assert b.rope_info() == dict(a.rope_info(), rope_scaling_type="llama3", rope_orig_ctx=64) and b.rope_factors == 32
    a.close(); b.close()
    # ... and the seeded generator's model (no file at all) takes the option too
    s = E.Engine()
    s.set_option("rope_scaling", "llama3:8,1,4,64")
    s.load_synthetic(E.synth_spec("tiny", "Q8_0"), CTX)
    s0 = E.Engine()
    s0.load_synthetic(E.synth_spec("tiny", "Q8_0"), CTX)
    assert s.rope_factors == 32 and s0.rope_factors == 0
    assert dist(s.forward(toks[:37], 0), s0.forward(toks[:37], 0)) >= 10 * TOL
    s.close(); s0.close()
    # rope_scaling=none on a scaled file = the same file written without scaling
    p0 = engine_for(plain_path)
    plain = run_tokens(p0, toks)
    assert p0.rope_info() == {"rope_theta": THETA, "rope_freq_scale": 1.0, "rope_factors": 0, "rope_orig_ctx": 0, "rope_scaling_type": "none"}
    p0.close()
    assert not same_bits(plain, want)
    n = engine_for(model_file("t64lin", tmp_path_factory), rope_scaling="none")
    assert same_bits(run_tokens(n, toks), plain) and n.rope_factors == 0 and n.rope_freq_scale == 1.0
    n.close()
    # rope_freq_base / rope_freq_scale / linear:<f> = files written with those values
    shape = G.LlamaShape("tiny", 256, 512, 2, 4, 2, 512, ctx=256, theta=10000.0, bos=256, eos=257)
    path = str(tmp_path_factory.mktemp("theta") / "model.gguf")
    G.make_synthetic_llama(path, shape, "Q8_0", seed=20261020, rope_scaling={"type": "linear", "factor": 4.0})
    f = engine_for(path)
    want = run_tokens(f, toks)
    assert f.rope_info()["rope_theta"] == 10000.0 and f.rope_freq_scale == 0.25
    f.close()
    for opts in (dict(rope_freq_base=10000.0, rope_freq_scale=0.25), dict(rope_freq_base="1e4", rope_scaling="linear:4")):
        o = engine_for(plain_path, **opts)
        assert same_bits(run_tokens(o, toks), want), opts
        o.close()
    assert not same_bits(plain, want)
    # linear:<f> sets the linear scale alone: the file's divisors stay (t64 + linear:4 = t64lin's rotation when both carry the same divisors)
    lin_file = engine_for(model_file("t64", tmp_path_factory, rope_scaling={"type": "linear", "factor": 4.0}))
    lin_opt = engine_for(model_file("t64", tmp_path_factory), rope_scaling="linear:4")
    assert lin_opt.rope_factors == 32 and lin_opt.rope_freq_scale == 0.25 and lin_opt.rope_scaling_type == "linear"
    assert same_bits(run_tokens(lin_opt, toks), run_tokens(lin_file, toks))
    lin_file.close(); lin_opt.close()


def test_rope_options_are_refused_after_a_load(tmp_path_factory):
    """(the option grammar itself: tests/test_rope_scaling_cpu.py; this half needs a loaded engine)"""
    e = engine_for(model_file("t64", tmp_path_factory))
    before = e.forward(prompt_tokens()[:5], 0)
    for key, val in (("rope_scaling", "none"), ("rope_freq_base", "10000"), ("rope_freq_scale", "0.5")):
        with pytest.raises(_lib.NtkError) as ei:
            e.set_option(key, val)
        assert ei.value.status == -2 and key in str(ei.value) and "before" in str(ei.value)
    assert np.array_equal(e.forward(prompt_tokens()[:5], 0), before)
    e.close()


# ------------------------------------------------------------------------------------------------ 9: refusals, yarn, the CLI
def test_a_refused_load_leaves_nothing_resident_and_the_engine_usable(tmp_path_factory):
    def free():
        fr, tot = C.c_size_t(), C.c_size_t()
        _lib.lib().ntk_device_mem_info(C.byref(fr), C.byref(tot))
        return fr.value
    good = model_file("t64", tmp_path_factory)
    e = engine_for(good)
    e.close()
    base = free()
    bad = {"short": (np.ones(31, np.float32), -2), "f16": (np.ones(32, np.float16), -1), "zero": (np.r_[np.ones(31, np.float32), np.float32(0)], -2),
           "nan": (np.r_[np.float32(np.nan), np.ones(31, np.float32)], -2)}
    e = E.Engine()
    for what, (freqs, status) in bad.items():
        with pytest.raises(_lib.NtkError) as ei:
            e.load(model_file("t64", tmp_path_factory, rope_freqs=freqs, rope_scaling={"original_context_length": len(what)}), CTX)
        assert ei.value.status == status and "rope_freqs.weight" in str(ei.value), what
        assert free() >= base - (1 << 20), (what, base - free())          # nothing stays resident
    e.load(good, CTX)                                                  # the same engine object loads a good file afterwards
    assert e.rope_factors == 32 and np.isfinite(e.forward(prompt_tokens()[:5], 0)).all()
    e.close()


YARN_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from ntransformer_amd import engine as E
e = E.Engine()
e.load(sys.argv[2], 128)
np.save(sys.argv[3], e.forward([int(t) for t in sys.argv[4].split(",")], 0))
print("INFO", e.rope_scaling_type, e.rope_freq_scale, e.rope_factors, e.rope_orig_ctx)
e.close()
"""


def test_a_yarn_file_loads_unscaled_and_says_so(tmp_path_factory, tmp_path):
    """(a child process: the engine writes the line to the C stderr)"""
    toks = prompt_tokens()[:20]
    yarn = model_file("t64", tmp_path_factory, rope_freqs=None, rope_scaling={"type": "yarn", "factor": 4.0, "original_context_length": 32})
    script = str(tmp_path / "yarn.py")
    open(script, "w").write(YARN_SCRIPT)
    out = str(tmp_path / "logits.npy")
    r = subprocess.run([sys.executable, script, ROOT, yarn, out, ",".join(map(str, toks))], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    lines = [l for l in r.stderr.splitlines() if "yarn" in l and "not applied" in l]
    assert len(lines) == 1, r.stderr[-2000:]
    assert "INFO yarn 1.0 0 32" in r.stdout
    p = engine_for(model_file("t64", tmp_path_factory, rope_freqs=None, rope_scaling=None))
    assert np.array_equal(np.load(out), p.forward(toks, 0))            # as the same file without the keys
    p.close()


def test_cli_rope_scaling_flag_reaches_the_engine():
    """`ntransformer --synthetic tiny:Q8_0 --rope-scaling llama3:8,1,4,64`: the greedy tokens the Python engine generates under the same option"""
    exe = os.path.join(os.path.dirname(E.__file__), "ntransformer")
    assert os.path.exists(exe), "CLI not built"
    base = [exe, "--synthetic", "tiny:Q8_0", "-p", "hi there", "-c", "128", "-n", "24", "-t", "0", "--repeat-penalty", "1.0"]
    texts = {}
    for flags in ((), ("--rope-scaling", "llama3:8,1,4,64"), ("--rope-scaling", "llama3:8,1,4,64", "--rope-freq-scale", "0.5", "--rope-freq-base", "10000")):
        r = subprocess.run(base + list(flags), capture_output=True, timeout=300)
        assert r.returncode == 0, (r.stderr + r.stdout).decode("utf-8", "replace")[-2000:]
        texts[flags] = r.stdout
    spec = E.SynthSpec(256, 512, 2, 4, 2, 512, 256, 1e-5, 500000.0, 256, 257, b"Q8_0", 20260925)
    for flags, opts in (((), {}), (("--rope-scaling", "llama3:8,1,4,64"), {"rope_scaling": "llama3:8,1,4,64"})):
        e = E.Engine()
        for k, v in opts.items():
            e.set_option(k, v)
        e.load_synthetic(spec, 128)
        ids = e.generate_tokens(e.tokenize("hi there"), 24, temperature=0.0, repeat_penalty=1.0)
        buf = C.create_string_buffer(4096)
        arr = (C.c_int * len(ids))(*ids)
        n = e.L.nt_engine_detokenize(e.h, arr, len(ids), buf, 4096)
        text = buf.raw[:n].replace(b"\0", b"")          # (the CLI prints token by token with fputs: a NUL byte token prints nothing)
        assert len(ids) == 24 and text and text in texts[flags], (flags, ids, text, texts[flags][-500:])
        e.close()
    assert texts[()] != texts[("--rope-scaling", "llama3:8,1,4,64")]
    r = subprocess.run(base + ["--rope-scaling", "llama3:8,1"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--rope-scaling" in r.stderr
