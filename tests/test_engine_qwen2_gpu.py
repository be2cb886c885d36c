"""Qwen2 models through the engine on the GPU: synthetic two-layer models whose GGUF is written under the `qwen2` architecture with seeded Q | K | V
projection biases (blk.N.attn_{q,k,v}.bias) against an oracle that adds them -- tests/qkv_bias_ref.py wraps OracleModel._gemv, oracle/ is untouched.

Models (tests/qkv_bias_ref.py; context 1024, theta 1e6, eps 1e-6):
  qt64    hidden 256, 4 / 2 heads, head_dim 64, Q8_0
  qt128   hidden 256, 2 / 1 heads, head_dim 128, Q4_K_M
  q7      hidden 1792, inter 512, vocab 512, 14 / 2 heads, head_dim 128, Q8_0: 7 query heads per KV head
Bars are the project's: logits within 1e-3 of the bias-aware oracle, score within 2e-3.

THE GUARD is tests/test_qkv_bias_cpu.py::test_the_biases_move_the_logits_by_ten_bars_on_every_test_model (it needs no GPU): the bias-aware oracle is 1 .. 4
in the logits -- a thousand bars -- away from the plain oracle at every tested prompt length, so an engine that ignores the bias tensors (the engine before
this feature loaded these files without complaint) fails every test here.  test_engine_matches_... repeats the assertion on the reference it uses.

kv_cache=q8_0 is held the way tests/test_rope_scaling_engine_gpu.py holds it: the cache contents at the bars of tests/test_kv_q8_gpu.py (V blocks bit-exact,
K quants within one step and scales within 2^-10 of the numpy quantiser of the oracle's rotation of the captured, biased K), and the logits -- q8_0 engine
against F16 engine, fused against unfused steps -- within 3 x what the same engines show on the bias-free twin of the file (the same seed written without
the three bias vectors): both distances are rounding noise of cached rows of the same magnitudes.

Run on the MI355X box:  python -m pytest tests/test_engine_qwen2_gpu.py -m gpu -x -q"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from ntransformer_amd import kv_q8
from ntransformer_amd import engine as E
from ntransformer_amd import kv_ops as KO
from oracle import oracle as O
from qkv_bias_ref import BIAS_SCALE, CTX, GUARD_LENGTHS, LENGTHS, MODELS, N_STEPS, SCORE_TOL, TOL, dist, model_file, oracle_ref, patch_oracle, prompt_tokens
from rope_ref import plain_table
from score_ref import logprob_ref

pytestmark = pytest.mark.gpu
THETA = 1e6


def engine_for(path, ctx=CTX, **opts):
    e = E.Engine()
    for k, v in opts.items():
        e.set_option(k, v)
    e.load(path, ctx)
    return e


def biased_oracle(path, passes):
    """the bias-aware oracle through a list of (tokens, start_pos) passes on one model object: the logits of each"""
    with pytest.MonkeyPatch.context() as mp:
        patch_oracle(mp)
        m = O.OracleModel(path, CTX)
        return [m.forward(list(t), s) for t, s in passes]


# ------------------------------------------------------------------------------------------------ prompt forms, score, the count of biased layers
@pytest.mark.parametrize("name", sorted(MODELS))
def test_engine_matches_the_bias_aware_oracle_in_every_prompt_form(name, tmp_path_factory):
    """Prompt passes of 1 and 3 tokens (per-token GEMVs / the streaming GEMM), 4 and 37 (the fused store), 70 (beyond the 64-token border of
    prefill_fused_split), a chunked prefill 37 + 33, and score over 37 positions."""
    ref = oracle_ref(name, tmp_path_factory)
    for T in GUARD_LENGTHS:
        assert dist(ref["prompt"][T], ref["plain"][T]) >= 10 * TOL          # (the guard, on the reference this test uses)
    e = engine_for(ref["path"])
    assert e.qkv_bias == 2 and e.n_layers == 2
    for T in LENGTHS:
        got = e.forward(ref["tokens"][:T], 0)
        err = dist(got, ref["prompt"][T])
        print(name, "T", T, "engine - bias-aware oracle: max |dlogit| =", err)
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
    """fused + graph (the bias launch is a node of the captured token), graph = 0, and fused = 0 (a one-token forward), against the bias-aware oracle"""
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


def test_a_step_behind_560_tokens_sees_biased_keys_in_the_split_regime(tmp_path_factory):
    """qt128, position 560 (>= 544: the split-KV decode attention over 560 cached rows, every one of them a biased K and V)"""
    path = model_file("qt128", tmp_path_factory)
    r = np.random.Generator(np.random.Philox(key=[20261021, 43]))
    toks = [256] + [int(t) for t in r.integers(0, 256, 559)]
    plain = O.OracleModel(path, CTX)
    plain.forward(toks, 0)
    want_plain = plain.forward([77], 560)
    _, want = biased_oracle(path, [(toks, 0), ([77], 560)])
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
@pytest.mark.parametrize("name", ["qt64", "q7"])
def test_sequence_slots_packed_pass_and_shared_weights(name, tmp_path_factory):
    ref = oracle_ref(name, tmp_path_factory)
    toks, fed = ref["tokens"], ref["fed"]
    e = engine_for(ref["path"], sequences=4)
    assert e.qkv_bias == 2
    # the packed pass: three prompts in one pass over the weights ...
    got, _ = e.forward_batch([0, 1, 2], [toks[:37], toks[:4], toks[:3]], [0, 0, 0])
    for s, T in enumerate((37, 4, 3)):
        assert dist(got[s], ref["prompt"][T]) <= TOL, (name, "packed", s, dist(got[s], ref["prompt"][T]))
    # ... and mixed segments: a decode row behind slot 0's prompt beside a 70-token prompt chunk in slot 3
    got, _ = e.forward_batch([0, 3], [[fed[0]], toks[:70]], [37, 0])
    assert dist(got[0], ref["steps"][0]) <= TOL and dist(got[1], ref["prompt"][70]) <= TOL, (name, dist(got[0], ref["steps"][0]), dist(got[1], ref["prompt"][70]))
    # a batched decode step over three slots: slot 0 at position 38, slots 1 and 2 behind their short prompts
    want1 = biased_oracle(ref["path"], [(toks[:4], 0), ([9], 4)])[1]
    want2 = biased_oracle(ref["path"], [(toks[:3], 0), ([10], 3)])[1]
    lg, nxt = e.decode_batch([0, 1, 2], [fed[1], 9, 10], [38, 4, 3])
    for s, want in enumerate((ref["steps"][1], want1, want2)):
        assert np.isfinite(lg[s]).all() and dist(lg[s], want) <= TOL, (name, "decode_batch", s, dist(lg[s], want))
    # seq_forward on another slot
    assert dist(e.seq_forward(3, toks[:37], 0), ref["prompt"][37]) <= TOL
    e.close()
    # a sharing sequence adds its source's biases: the solo bits
    solo = engine_for(ref["path"])
    want = solo.forward(toks[:37], 0)
    want_step = solo.decode_fused(fed[0], 37, graph=True)
    b = E.Engine()
    b.load_shared(solo, CTX)
    assert b.qkv_bias == 2
    assert np.array_equal(b.forward(toks[:37], 0), want) and np.array_equal(b.decode_fused(fed[0], 37, graph=True), want_step)
    assert dist(want_step, ref["steps"][0]) <= TOL
    b.close(); solo.close()


# ------------------------------------------------------------------------------------------------ the context shift
def test_a_context_shift_followed_by_a_step(tmp_path_factory):
    """The construction of tests/test_kv_ops_engine_gpu.py on qt128: the cached keys carry the bias, and a shift re-rotates them as they are -- shifted keys are
    the keys the model caches at the new positions (layer 0, where a key depends on nothing but its token); the step behind the shift against a cache written
    from the checker."""
    path = model_file("qt128", tmp_path_factory)
    hd, row = 128, 128
    tab = plain_table(hd, THETA)
    toks = prompt_tokens(48, seed=42)
    r = np.random.Generator(np.random.Philox(key=[20261021, 44]))
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
Q8_VS_TWIN_FACTOR = 3.0


def q8_distances(path, toks, fed, nh, nkv, hd, check_cache):
    """q8_0 engine against F16 engine over a 37-token pass, a 3-token pass and 8 decode steps, and the q8_0 engine's fused against its unfused steps"""
    per = nkv * hd
    q, f = engine_for(path, kv_cache="q8_0"), engine_for(path)
    vs_f16, fused_unfused = [], []
    q.kv_inputs_capture(0)
    for start, T in ((0, 37), (37, 3)):          # the fused RoPE + 8-bit store launch; ntk_rope + ntk_kv_store_q8
        lq, lf = q.forward(toks[start:start + T], start), f.forward(toks[start:start + T], start)
        assert np.isfinite(lq).all()
        vs_f16.append(dist(lq, lf))
        if check_cache:                          # the bars of tests/test_kv_q8_gpu.py::test_engine_cache_contents_after_a_prompt_pass, on the captured (biased) rows
            k_in, v_in = q.kv_inputs_read(T, per)
            got_k, got_v = q.kv_read_q8(0, start, T, per)
            assert np.array_equal(got_v, kv_q8.to_blocks(*kv_q8.quantize_q8_0(v_in)))
            rk = np.stack([O.rope(np.zeros(nh * hd, np.float32), k_in[t], [start + t], nh, nkv, hd, THETA)[1] for t in range(T)])
            wd, wq = kv_q8.quantize_q8_0(rk)
            gd, gq = kv_q8.from_blocks(got_k)
            assert np.abs(gq.astype(np.int32) - wq.astype(np.int32)).max() <= 1
            assert (np.abs(gd.astype(np.float64) - wd.astype(np.float64)) <= 2.0 ** -10 * wd.astype(np.float64)).all()
            assert float((gq == wq).mean()) > 0.99
    for i, tok in enumerate(fed):
        plain = q.forward([tok], 40 + i)
        eager = q.decode_fused(tok, 40 + i, False)
        graph = q.decode_fused(tok, 40 + i, True)
        assert np.isfinite(eager).all() and np.isfinite(plain).all() and np.array_equal(eager, graph)
        fused_unfused.append(dist(eager, plain))
        vs_f16.append(dist(eager, f.decode_fused(tok, 40 + i, True)))
    q.close(); f.close()
    return vs_f16, fused_unfused


@pytest.mark.parametrize("name", ["qt128", "q7"])
def test_q8_kv_cache_on_a_biased_model(name, tmp_path_factory):
    """(see the module docstring; the F16 engine is held to the oracle by the tests above)"""
    ref = oracle_ref(name, tmp_path_factory)
    shape, mix = MODELS[name]
    hd = shape.hidden // shape.heads
    # the captured rows are the biased ones: layer 0's V of a token is W_v . norm(embedding) + b_v -- the oracle's
    with pytest.MonkeyPatch.context() as mp:
        patch_oracle(mp)
        m = O.OracleModel(ref["path"], CTX)
        x0 = O.rmsnorm(m.embed(ref["tokens"][:3]), m.f.f32("blk.0.attn_norm.weight"), m.eps)
        v_want = np.stack([m._gemv("blk.0.attn_v.weight", x0[t], shape.kv_heads * hd, shape.hidden) for t in range(3)])
        bias_v = np.array(m.f.f32("blk.0.attn_v.bias"))
    e = engine_for(ref["path"])
    e.kv_inputs_capture(0)
    e.forward(ref["tokens"][:3], 0)
    _, v_in = e.kv_inputs_read(3, shape.kv_heads * hd)
    e.close()
    assert dist(v_in, v_want) <= TOL and dist(v_in, v_want - bias_v[None, :]) >= 0.5 * float(np.abs(bias_v).max())
    biased = q8_distances(ref["path"], ref["tokens"], ref["fed"], shape.heads, shape.kv_heads, hd, True)
    twin = q8_distances(model_file(name, tmp_path_factory, qkv_bias=None), ref["tokens"], ref["fed"], shape.heads, shape.kv_heads, hd, False)
    fmt = lambda xs: " ".join("%.3g" % x for x in xs)
    print(name, "q8_0 - f16 with the biases (37-token pass, 3-token pass, 8 steps):", fmt(biased[0]))
    print(name, "q8_0 - f16 on the bias-free twin (the same):", fmt(twin[0]), "-> bar %.3g" % (Q8_VS_TWIN_FACTOR * max(twin[0])))
    print(name, "q8_0 fused - unfused, 8 steps, with the biases:", fmt(biased[1]))
    print(name, "q8_0 fused - unfused, 8 steps, on the twin:    ", fmt(twin[1]), "-> bar %.3g" % (Q8_VS_TWIN_FACTOR * max(twin[1])))
    assert max(biased[0]) <= Q8_VS_TWIN_FACTOR * max(twin[0]), (biased[0], twin[0])
    assert max(biased[1]) <= Q8_VS_TWIN_FACTOR * max(twin[1]), (biased[1], twin[1])


# ------------------------------------------------------------------------------------------------ tensor parallelism, two processes
def test_two_tensor_parallel_ranks_match_the_bias_aware_oracle(tmp_path_factory, tmp_path):
    """each rank owns whole heads and the matching slice of every bias"""
    from test_tp_gpu import RANK_SCRIPT
    ref = oracle_ref("qt64", tmp_path_factory)
    d = str(tmp_path)
    json.dump({"prompt": ref["tokens"][:37], "fed": ref["fed"][:4], "run_id": "qwen2"}, open(os.path.join(d, "job.json"), "w"))
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
        assert dist(lgs[k], want) <= TOL, ("vs the bias-aware oracle", k, dist(lgs[k], want))
    assert np.array_equal(lgs[0], lgs[1])


# ------------------------------------------------------------------------------------------------ the CLI, a Llama model, a partial set of biases
def test_cli_runs_the_file(tmp_path_factory):
    """`ntransformer -m <qwen2 file>`: the greedy tokens the Python engine generates from the same file, and not those of its bias-free twin"""
    exe = os.path.join(os.path.dirname(E.__file__), "ntransformer")
    assert os.path.exists(exe), "CLI not built"
    texts = {}
    for kind, path in (("biased", model_file("qt64", tmp_path_factory)), ("twin", model_file("qt64", tmp_path_factory, qkv_bias=None))):
        r = subprocess.run([exe, "-m", path, "-p", "hi there", "-c", "128", "-n", "24", "-t", "0", "--repeat-penalty", "1.0"], capture_output=True, timeout=300)
        assert r.returncode == 0, (r.stderr + r.stdout).decode("utf-8", "replace")[-2000:]
        e = engine_for(path, ctx=128)
        ids = e.generate_tokens(e.tokenize("hi there"), 24, temperature=0.0, repeat_penalty=1.0)
        buf = C.create_string_buffer(4096)
        arr = (C.c_int * len(ids))(*ids)
        n = e.L.nt_engine_detokenize(e.h, arr, len(ids), buf, 4096)
        text = buf.raw[:n].replace(b"\0", b"")          # (the CLI prints token by token with fputs: a NUL byte token prints nothing)
        assert len(ids) == 24 and text and text in r.stdout, (kind, ids, text, r.stdout[-500:])
        texts[kind] = text
        e.close()
    assert texts["biased"] != texts["twin"]


def test_a_llama_model_has_no_biased_layer_and_matches_the_plain_oracle():
    """an existing golden model: nt_engine_qkv_bias = 0, and its logits are the PLAIN oracle's, prompt and decode (its launches are what they were)"""
    path = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    toks = prompt_tokens(37)
    m = O.OracleModel(path, 256)
    want = m.forward(toks, 0)
    want_step = m.forward([7], 37)
    e = engine_for(path, ctx=256)
    assert e.qkv_bias == 0
    assert dist(e.forward(toks, 0), want) <= TOL
    assert dist(e.decode_fused(7, 37, graph=True), want_step) <= TOL
    e.close()


def test_a_llama_file_with_only_a_key_bias(tmp_path_factory):
    """the biases are optional and independent, under any architecture: a `llama` file that carries attn_k.bias alone"""
    path = model_file("qt64", tmp_path_factory, arch="llama", qkv_bias={"k": BIAS_SCALE})
    toks = prompt_tokens()
    plain = O.OracleModel(path, CTX).forward(toks[:37], 0)
    want, want_step = biased_oracle(path, [(toks[:37], 0), ([7], 37)])
    assert dist(want, plain) >= 10 * TOL
    e = engine_for(path)
    assert e.qkv_bias == 2
    assert dist(e.forward(toks[:37], 0), want) <= TOL
    assert dist(e.decode_fused(7, 37, graph=True), want_step) <= TOL
    assert dist(e.forward([7], 37), want_step) <= TOL
    e.close()


# ------------------------------------------------------------------------------------------------ the seeded generator's Qwen2 flavour, loaded without a file
@pytest.mark.parametrize("flavour,layers_biased,tied", [("qwen2-tied:", 2, True), ("qwen2:", 2, False), ("tied:", 0, True)])
def test_load_synthetic_runs_the_qwen2_flavours(flavour, layers_biased, tied, tmp_path):
    """nt_engine_load_synthetic with the flavour in front of the mix (what `--synthetic qwen2.5-7b:Q8_0` runs, at the tiny shape): the bias vectors reach the
    layers, a tied flavour computes its logits from token_embd.weight, and the logits are the bias-aware oracle's over the file nt_synth_write_gguf writes
    for the same spec -- and the bits of an engine that loaded that file."""
    spec = E.SynthSpec(256, 512, 2, 4, 2, 512, 256, 1e-6, 1e6, 256, 257, (flavour + "Q8_0").encode(), 20260925)
    path = str(tmp_path / "synth.gguf")
    E.synth_write_gguf(path, spec, 2)
    d = E.gguf_describe(path)
    names = [t["name"] for t in d["tensors"]]
    assert ("output.weight" not in names) == tied and d["qkv_bias_tensors"] == 3 * layers_biased
    toks = prompt_tokens(37)
    want, want_step = biased_oracle(path, [(toks, 0), ([7], 37)])
    if layers_biased:
        assert dist(want, O.OracleModel(path, 128).forward(toks, 0)) >= 10 * TOL
    s = E.Engine()
    s.load_synthetic(spec, 128)
    f = engine_for(path, ctx=128)
    assert s.qkv_bias == layers_biased == f.qkv_bias
    assert s.weight_bytes() == f.weight_bytes() == sum(t["nbytes"] for t in d["tensors"])          # (tied: no second copy of the embedding is uploaded)
    got, got_f = s.forward(toks, 0), f.forward(toks, 0)
    assert np.isfinite(got).all() and dist(got, want) <= TOL, dist(got, want)
    assert np.array_equal(got, got_f)
    step, step_f = s.decode_fused(7, 37, graph=True), f.decode_fused(7, 37, graph=True)
    assert dist(step, want_step) <= TOL and np.array_equal(step, step_f)
    s.close(); f.close()
