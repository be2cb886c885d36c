"""Qwen3 models through the engine on the GPU: synthetic two-layer models with per-head Q / K RMSNorm vectors (blk.N.attn_q_norm.weight /
attn_k_norm.weight) and a head size of their own (<arch>.attention.key_length) against an oracle that knows both -- tests/qwen3_ref.py subclasses
OracleModel, oracle/ is untouched.

Models (tests/qwen3_ref.py; context 1024, theta 1e6, eps 1e-6, norm weights 1 + 0.5 u):
  q3n64     hidden 256, 4 / 2 heads, head_dim 64 = hidden / heads, norms, Q8_0
  q3w128    hidden 256, 4 / 2 heads, head_dim 128: heads x head_dim = 512 > hidden, norms, Q4_K_M
  q3g128    hidden 1024, 8 / 2 heads, head_dim 128, norms, 4 query heads per KV head, BF16 (the oracle reads its F32 twin)
  nemo128   hidden 512, 2 / 1 heads, head_dim 128: heads x head_dim = 256 < hidden, architecture `llama`, key_length and NO norms, Q8_0
Bars are the project's: logits within 1e-3 of the oracle, score within 2e-3.

THE GUARD is tests/test_qwen3_cpu.py (it needs no GPU): on every model and tested prompt length the reference is at least ten bars away from the oracle
without the norms, from the one with the q and k vectors swapped, from the one that keeps hidden / heads, and -- for the bias + norm model -- from the one
that normalises ahead of the bias.  The engine before this feature refused every one of these files but nemo128 by tensor name, and computed nemo128 with
256-wide heads.  test_engine_matches_... repeats the guard on the reference it uses.

kv_cache=q8_0 is held the way tests/test_engine_qwen2_gpu.py holds it (its q8_distances and factor are imported): cache contents at the bars of
tests/test_kv_q8_gpu.py on the captured -- normalised -- K rows, and the logits of the q8_0 engine against the F16 engine and fused against unfused within
3 x what the same engines show on the norm-free twin of the file.

Run on the MI355X box:  python -m pytest tests/test_engine_qwen3_gpu.py -m gpu -x -q"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from ntransformer_amd import engine as E
from ntransformer_amd import kv_ops as KO
from oracle import oracle as O
from qwen3_ref import (BIAS_SCALE, CTX, GUARD_LENGTHS, LENGTHS, MODELS, N_STEPS, SCORE_TOL, TOL, Qwen3Oracle, dist, model_file, oracle_file,
                       oracle_passes, oracle_ref, prompt_tokens)
from rope_ref import plain_table
from score_ref import logprob_ref
from test_engine_qwen2_gpu import Q8_VS_TWIN_FACTOR, q8_distances

pytestmark = pytest.mark.gpu
THETA = 1e6


def engine_for(path, ctx=CTX, **opts):
    e = E.Engine()
    for k, v in opts.items():
        e.set_option(k, v)
    e.load(path, ctx)
    return e


def norm_layers(name):
    return 2 if MODELS[name][3] else 0


# ------------------------------------------------------------------------------------------------ prompt forms, score, the count of normalising layers
@pytest.mark.parametrize("name", sorted(MODELS))
def test_engine_matches_the_norm_aware_oracle_in_every_prompt_form(name, tmp_path_factory):
    """Prompt passes of 1 and 3 tokens (per-token GEMVs / the streaming GEMM), 4 and 37 (the fused store), 70 (beyond the 64-token border of
    prefill_fused_split), a chunked prefill 37 + 33, and score over 37 positions."""
    ref = oracle_ref(name, tmp_path_factory)
    for wrong in ("none", "swapped", "coupled"):          # (the guard, on the reference this test uses)
        for T in GUARD_LENGTHS if wrong in ref else ():
            assert dist(ref["prompt"][T], ref[wrong][T]) >= 10 * TOL
    e = engine_for(ref["path"])
    assert e.qk_norm == norm_layers(name) and e.qkv_bias == 0 and e.n_layers == 2
    for T in LENGTHS:
        got = e.forward(ref["tokens"][:T], 0)
        err = dist(got, ref["prompt"][T])
        print(name, "T", T, "engine - norm-aware oracle: max |dlogit| =", err)
        assert np.isfinite(got).all() and err <= TOL, (name, T, err)
    e.forward(ref["tokens"][:37], 0)
    err = dist(e.forward(ref["tokens"][37:70], 37), ref["chunked"])
    print(name, "chunked 37 + 33: max |dlogit| =", err)
    assert err <= TOL
    lp = e.score(ref["tokens"][:37])
    want, _ = logprob_ref(ref["all37"], ref["tokens"][1:37] + [-1])
    print(name, "score over 37 positions: max |dlogprob| =", float(np.abs(lp - want).max()))
    assert np.abs(lp - want).max() <= SCORE_TOL
    e.close()


# ------------------------------------------------------------------------------------------------ decode steps
@pytest.mark.parametrize("mode", ["fused_graph", "fused_eager", "unfused"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_eight_decode_steps_behind_a_prompt(name, mode, tmp_path_factory):
    """fused + graph (the norm launch is a node of the captured token), graph = 0, and fused = 0 (a one-token forward), against the norm-aware oracle"""
    ref = oracle_ref(name, tmp_path_factory)
    e = engine_for(ref["path"])
    e.forward(ref["tokens"][:37], 0)
    for i, tok in enumerate(ref["fed"]):
        got = e.forward([tok], 37 + i) if mode == "unfused" else e.decode_fused(tok, 37 + i, graph=(mode == "fused_graph"))
        err = dist(got, ref["steps"][i])
        assert np.isfinite(got).all() and err <= TOL, (name, mode, i, err)
    if mode == "fused_graph":       # ... and the generate loop: its greedy tokens are the oracle's unless a near tie flips
        a = e.generate_tokens(ref["tokens"][:37], N_STEPS, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
        want = [int(np.argmax(ref["prompt"][37]))] + [int(np.argmax(s)) for s in ref["steps"][:N_STEPS - 1]]
        margins = [float(np.sort(s)[-1] - np.sort(s)[-2]) for s in [ref["prompt"][37]] + ref["steps"][:N_STEPS - 1]]
        if min(margins) > 2 * TOL:
            assert a == want
    e.close()


def test_a_step_behind_560_tokens_sees_normalised_keys_in_the_split_regime(tmp_path_factory):
    """q3w128, position 560 (>= 544: the split-KV decode attention over 560 cached rows of 128-wide heads, every K of them normalised)"""
    path = model_file("q3w128", tmp_path_factory)
    r = np.random.Generator(np.random.Philox(key=[20261022, 43]))
    toks = [256] + [int(t) for t in r.integers(0, 256, 559)]
    _, want_plain = oracle_passes(path, [(toks, 0), ([77], 560)], norms="none")
    _, want = oracle_passes(path, [(toks, 0), ([77], 560)])
    assert dist(want, want_plain) >= 10 * TOL
    e = engine_for(path)
    e.forward(toks, 0)
    for graph in (True, False):
        got = e.decode_fused(77, 560, graph=graph)
        err = dist(got, want)
        print("step at position 560, graph", graph, ": max |dlogit| =", err)
        assert np.isfinite(got).all() and err <= TOL
    e.close()


# ------------------------------------------------------------------------------------------------ sequence slots, the packed pass, shared weights
@pytest.mark.parametrize("name", ["q3n64", "q3w128", "nemo128"])
def test_sequence_slots_packed_pass_and_shared_weights(name, tmp_path_factory):
    ref = oracle_ref(name, tmp_path_factory)
    toks, fed = ref["tokens"], ref["fed"]
    e = engine_for(ref["path"], sequences=4)
    assert e.qk_norm == norm_layers(name)
    # the packed pass: three prompts in one pass over the weights ...
    got, _ = e.forward_batch([0, 1, 2], [toks[:37], toks[:4], toks[:3]], [0, 0, 0])
    for s, T in enumerate((37, 4, 3)):
        assert dist(got[s], ref["prompt"][T]) <= TOL, (name, "packed", s, dist(got[s], ref["prompt"][T]))
    # ... and mixed segments: a decode row behind slot 0's prompt beside a 70-token prompt chunk in slot 3
    got, _ = e.forward_batch([0, 3], [[fed[0]], toks[:70]], [37, 0])
    assert dist(got[0], ref["steps"][0]) <= TOL and dist(got[1], ref["prompt"][70]) <= TOL, (name, dist(got[0], ref["steps"][0]), dist(got[1], ref["prompt"][70]))
    # a batched decode step over three slots: slot 0 at position 38, slots 1 and 2 behind their short prompts
    want1 = oracle_passes(ref["path"], [(toks[:4], 0), ([9], 4)])[1]
    want2 = oracle_passes(ref["path"], [(toks[:3], 0), ([10], 3)])[1]
    lg, nxt = e.decode_batch([0, 1, 2], [fed[1], 9, 10], [38, 4, 3])
    for s, want in enumerate((ref["steps"][1], want1, want2)):
        assert np.isfinite(lg[s]).all() and dist(lg[s], want) <= TOL, (name, "decode_batch", s, dist(lg[s], want))
    # seq_forward on another slot
    assert dist(e.seq_forward(3, toks[:37], 0), ref["prompt"][37]) <= TOL
    e.close()
    # a sharing sequence normalises with its source's vectors: the solo bits
    solo = engine_for(ref["path"])
    want = solo.forward(toks[:37], 0)
    want_step = solo.decode_fused(fed[0], 37, graph=True)
    b = E.Engine()
    b.load_shared(solo, CTX)
    assert b.qk_norm == norm_layers(name)
    assert np.array_equal(b.forward(toks[:37], 0), want) and np.array_equal(b.decode_fused(fed[0], 37, graph=True), want_step)
    assert dist(want_step, ref["steps"][0]) <= TOL
    b.close(); solo.close()


# ------------------------------------------------------------------------------------------------ the context shift
def test_a_context_shift_followed_by_a_step(tmp_path_factory):
    """The construction of tests/test_kv_ops_engine_gpu.py on q3w128: the cached keys were normalised before they were cached, and a shift re-rotates them as
    they are -- shifted keys are the keys the model caches at the new positions (layer 0, where a key depends on nothing but its token); the step behind the
    shift against a cache written from the checker."""
    path = model_file("q3w128", tmp_path_factory)
    hd, row = 128, 256
    tab = plain_table(hd, THETA)
    toks = prompt_tokens(48, seed=42)
    r = np.random.Generator(np.random.Philox(key=[20261022, 44]))
    a, b = engine_for(path, ctx=128), engine_for(path, ctx=128)
    a.forward(toks[:40], 0)
    k0 = np.stack([a.kv_read(l, 0, 128, row)[0] for l in range(2)])
    v0 = np.stack([a.kv_read(l, 0, 128, row)[1] for l in range(2)])
    assert a.kv_shift(0, 0, 8, 40) == 32
    ka, va = a.kv_read(0, 0, 32, row)
    b.kv_inputs_capture(0)
    b.forward(toks[8:40] + [int(t) for t in r.integers(0, 256, 8)], 0)
    kb, vb = b.kv_read(0, 0, 32, row)
    k_in, _ = b.kv_inputs_read(32, row)
    assert np.array_equal(va, vb)
    err = np.abs(ka.view(np.float16).astype(np.float64) - kb.view(np.float16).astype(np.float64))
    bar = 2.0 ** -9 * KO.pair_max(k_in, hd) + 2.0 ** -24
    print("shift vs the model's own keys: worst err / bar = %.3f" % float((err / bar).max()))
    assert (err <= bar).all()
    want_k, want_v = KO.shift_f16_ref(k0, v0, 8, 0, 32, hd, inv_freq=tab)
    c = engine_for(path, ctx=128)
    for l in range(2):
        c.kv_write(l, 0, want_k[l, :32], want_v[l, :32])
    la, lc = a.decode_fused(77, 32, graph=True), c.decode_fused(77, 32, graph=True)
    assert np.isfinite(la).all() and dist(la, lc) <= TOL
    a.close(); b.close(); c.close()


# ------------------------------------------------------------------------------------------------ the 8-bit KV cache
@pytest.mark.parametrize("name", ["q3w128", "q3g128"])
def test_q8_kv_cache_on_a_normalising_model(name, tmp_path_factory):
    """(see the module docstring; the F16 engine is held to the oracle by the tests above)"""
    ref = oracle_ref(name, tmp_path_factory)
    shape, mix, arch, _ = MODELS[name]
    hd = shape.hd
    # the captured rows are the normalised ones: layer 0's K of a token is rmsnorm per head of W_k . norm(embedding) -- the oracle's
    m = Qwen3Oracle(oracle_file(ref["path"]), CTX)
    x0 = O.rmsnorm(m.embed(ref["tokens"][:3]), m.f.f32("blk.0.attn_norm.weight"), m.eps)
    k_want = np.stack([m._gemv("blk.0.attn_k.weight", x0[t], shape.kv_heads * hd, shape.hidden) for t in range(3)])
    raw = Qwen3Oracle(oracle_file(ref["path"]), CTX, norms="none")
    k_raw = np.stack([raw._gemv("blk.0.attn_k.weight", x0[t], shape.kv_heads * hd, shape.hidden) for t in range(3)])
    e = engine_for(ref["path"])
    e.kv_inputs_capture(0)
    e.forward(ref["tokens"][:3], 0)
    k_in, _ = e.kv_inputs_read(3, shape.kv_heads * hd)
    e.close()
    assert dist(k_in, k_want) <= TOL and dist(k_in, k_raw) >= 100 * TOL
    normed = q8_distances(ref["path"], ref["tokens"], ref["fed"], shape.heads, shape.kv_heads, hd, True)
    twin = q8_distances(model_file(name, tmp_path_factory, qk_norm=None), ref["tokens"], ref["fed"], shape.heads, shape.kv_heads, hd, False)
    fmt = lambda xs: " ".join("%.3g" % x for x in xs)
    print(name, "q8_0 - f16 with the norms (37-token pass, 3-token pass, 8 steps):", fmt(normed[0]))
    print(name, "q8_0 - f16 on the norm-free twin (the same):", fmt(twin[0]), "-> bar %.3g" % (Q8_VS_TWIN_FACTOR * max(twin[0])))
    print(name, "q8_0 fused - unfused, 8 steps, with the norms:", fmt(normed[1]))
    print(name, "q8_0 fused - unfused, 8 steps, on the twin:    ", fmt(twin[1]), "-> bar %.3g" % (Q8_VS_TWIN_FACTOR * max(twin[1])))
    assert max(normed[0]) <= Q8_VS_TWIN_FACTOR * max(twin[0]), (normed[0], twin[0])
    assert max(normed[1]) <= Q8_VS_TWIN_FACTOR * max(twin[1]), (normed[1], twin[1])


# ------------------------------------------------------------------------------------------------ tensor parallelism, two processes
def test_two_tensor_parallel_ranks_match_the_norm_aware_oracle(tmp_path_factory, tmp_path):
    """q3w128: each rank owns two of the four 128-wide query heads and one KV head, and holds both norm vectors whole"""
    from test_tp_gpu import RANK_SCRIPT
    ref = oracle_ref("q3w128", tmp_path_factory)
    d = str(tmp_path)
    json.dump({"prompt": ref["tokens"][:37], "fed": ref["fed"][:4], "run_id": "qwen3"}, open(os.path.join(d, "job.json"), "w"))
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
        assert dist(lgs[k], want) <= TOL, ("vs the norm-aware oracle", k, dist(lgs[k], want))
    assert np.array_equal(lgs[0], lgs[1])


# ------------------------------------------------------------------------------------------------ the seeded generator's Qwen3 flavours, the CLI
def tiny_spec(mix, eps=1e-6, theta=1e6):
    return E.SynthSpec(256, 512, 2, 4, 2, 512, 256, eps, theta, 256, 257, mix, 20260925)


@pytest.mark.parametrize("flavour,layers_normed,hd,tied", [("qwen3-hd128:", 2, 128, False), ("qwen3:", 2, 64, False), ("hd128:", 0, 128, False),
                                                          ("qwen3-hd128-tied:", 2, 128, True), ("hd128-tied:", 0, 128, True)])
def test_load_synthetic_runs_the_qwen3_flavours(flavour, layers_normed, hd, tied, tmp_path):
    """nt_engine_load_synthetic with the flavour in front of the mix (what `--synthetic qwen3-4b:Q8_0` runs, at the tiny shape): the norm vectors reach the
    layers, the heads have the flavour's size, and the logits are the bits of an engine that loaded the file nt_synth_write_gguf writes for the same spec.
    The untied flavours are also held to the norm-aware oracle over that file at the 1e-3 bar.  The tied flavours are not: their LM head is token_embd.weight,
    whose rows the generator scales to RMS 1 where output.weight has RMS 0.125, so their logits -- and every absolute rounding error in them -- are many times
    the size the absolute bar was set for (measured: |logit| up to 182 against 6.5 on the untied twin; qwen3-hd128-tied is 1.33e-3 from the oracle on the
    prompt, 7e-6 of its largest logit, hd128-tied 2.7e-4); they are held to 1 % of the largest logit, and the figures are printed."""
    spec = tiny_spec((flavour + "Q8_0").encode())
    path = str(tmp_path / "synth.gguf")
    E.synth_write_gguf(path, spec, 2)
    d = E.gguf_describe(path)
    names = [t["name"] for t in d["tensors"]]
    assert ("output.weight" not in names) == tied and d["qk_norm_tensors"] == 2 * layers_normed and d["head_dim"] == hd
    toks = prompt_tokens(37)
    want, want_step = oracle_passes(path, [(toks, 0), ([7], 37)])
    if layers_normed:
        assert dist(want, oracle_passes(path, [(toks, 0)], norms="none")[0]) >= 10 * TOL
    s = E.Engine()
    s.load_synthetic(spec, 128)
    f = engine_for(path, ctx=128)
    assert s.qk_norm == layers_normed == f.qk_norm
    assert s.weight_bytes() == f.weight_bytes() == sum(t["nbytes"] for t in d["tensors"])          # (tied: no second copy of the embedding is uploaded)
    got, got_f = s.forward(toks, 0), f.forward(toks, 0)
    step, step_f = s.decode_fused(7, 37, graph=True), f.decode_fused(7, 37, graph=True)
    print(flavour, "max |logit| %.3g; engine - oracle: prompt %.3g, step %.3g" % (float(np.abs(want).max()), dist(got, want), dist(step, want_step)))
    assert np.isfinite(got).all() and np.isfinite(step).all()
    assert np.array_equal(got, got_f) and np.array_equal(step, step_f)
    if not tied:
        assert dist(got, want) <= TOL and dist(step, want_step) <= TOL, (dist(got, want), dist(step, want_step))
    else:          # the same computation, so far from the wrong ones that no rounding could bridge it
        assert dist(got, want) <= 0.01 * float(np.abs(want).max())
    s.close(); f.close()


def test_cli_runs_a_qwen3_flavour():
    """`ntransformer --synthetic tiny:qwen3-hd128:Q8_0`: the greedy tokens the Python engine generates from the same seeded spec, and not those of the
    norm-free twin `tiny:hd128:Q8_0`"""
    exe = os.path.join(os.path.dirname(E.__file__), "ntransformer")
    assert os.path.exists(exe), "CLI not built"
    texts = {}
    for kind, mix in (("normed", "qwen3-hd128:Q8_0"), ("twin", "hd128:Q8_0")):
        r = subprocess.run([exe, "--synthetic", "tiny:" + mix, "-p", "hi there", "-c", "128", "-n", "24", "-t", "0", "--repeat-penalty", "1.0"],
                           capture_output=True, timeout=300)
        assert r.returncode == 0, (r.stderr + r.stdout).decode("utf-8", "replace")[-2000:]
        e = E.Engine()
        e.load_synthetic(tiny_spec(mix.encode(), 1e-5, 500000.0), 128)          # (the CLI's tiny shape keeps the Llama eps and theta)
        assert e.qk_norm == (2 if kind == "normed" else 0)
        ids = e.generate_tokens(e.tokenize("hi there"), 24, temperature=0.0, repeat_penalty=1.0)
        buf = C.create_string_buffer(4096)
        arr = (C.c_int * len(ids))(*ids)
        n = e.L.nt_engine_detokenize(e.h, arr, len(ids), buf, 4096)
        text = buf.raw[:n].replace(b"\0", b"")          # (the CLI prints token by token with fputs: a NUL byte token prints nothing)
        assert len(ids) == 24 and text and text in r.stdout, (kind, ids, text, r.stdout[-500:])
        texts[kind] = text
        e.close()
    assert texts["normed"] != texts["twin"]


# ------------------------------------------------------------------------------------------------ biases AND norms, a Llama model
def test_a_model_with_biases_and_norms_adds_the_bias_first(tmp_path_factory):
    """q3n64 written with the three Qwen2 bias vectors beside the norm pair: the bias is added ahead of the norm (llama.cpp's order) in every pass"""
    path = model_file("q3n64", tmp_path_factory, qkv_bias=BIAS_SCALE)
    toks = prompt_tokens()
    want, want_step = oracle_passes(path, [(toks[:37], 0), ([7], 37)])
    assert dist(want, oracle_passes(path, [(toks[:37], 0)], bias_first=False)[0]) >= 10 * TOL
    e = engine_for(path)
    assert e.qkv_bias == 2 and e.qk_norm == 2
    assert dist(e.forward(toks[:37], 0), want) <= TOL
    assert dist(e.decode_fused(7, 37, graph=True), want_step) <= TOL
    assert dist(e.decode_fused(7, 37, graph=False), want_step) <= TOL
    assert dist(e.forward([7], 37), want_step) <= TOL
    e.close()


def test_a_llama_model_normalises_nothing_and_matches_the_plain_oracle():
    """an existing golden model: nt_engine_qk_norm = 0, and its logits are the PLAIN oracle's, prompt and decode (its launches are what they were)"""
    path = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    toks = prompt_tokens(37)
    m = O.OracleModel(path, 256)
    want = m.forward(toks, 0)
    want_step = m.forward([7], 37)
    e = engine_for(path, ctx=256)
    assert e.qk_norm == 0 and e.qkv_bias == 0
    assert dist(e.forward(toks, 0), want) <= TOL
    assert dist(e.decode_fused(7, 37, graph=True), want_step) <= TOL
    e.close()
    u = E.Engine()
    assert u.qk_norm == -1          # unloaded
    u.close()
