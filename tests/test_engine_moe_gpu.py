"""Mixture-of-experts models through the engine on the GPU: synthetic two-layer models whose FFN is the routed expert quartet (blk.N.ffn_gate_inp.weight +
ffn_{gate,up,down}_exps.weight) against an oracle that routes -- tests/moe_ref.py subclasses tests/qwen3_ref.Qwen3Oracle, oracle/ is untouched.

Models (tests/moe_ref.py; context 1024): moe8q8 (qwen3moe, heads of 64, norms, E 8 / K 2, I_e 96, Q8_0), moe4k (qwen3moe, heads of 128 through key_length,
norms, E 4 / K 2, I_e 768, Q4_K_M with Q6_K ffn_down_exps: 630-byte rows), mixtral4 (llama, E 4 / K 2, I_e = feed_forward_length, Q8_0), half (layer 0
dense, layer 1 routed).  Bars are the project's: logits within 1e-3 of the oracle, score within 2e-3.

THE GUARD is tests/test_moe_cpu.py (no GPU): every wrong oracle (unrenormalised or uniform weights, the K smallest logits, gate and up swapped, the down
expert reversed) is at least ten bars from the reference, and at every routed row of the passes run here the K-th and (K + 1)-th router logit lie at least
16 GEMV bars apart, so no rounding difference between two summation orders can move a token to another expert.  The engine before this feature refused
every one of these files ("Tensor not found: blk.N.ffn_gate.weight").

Run on the MI355X box:  python -m pytest tests/test_engine_moe_gpu.py -m gpu -x -q"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from moe_ref import CTX, GUARD_LENGTHS, LENGTHS, MODELS, N_STEPS, SCORE_TOL, TOL, WRONG, dist, model_file, oracle_passes, oracle_ref, prompt_tokens
from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from oracle import oracle as O
from score_ref import logprob_ref
from test_engine_qwen2_gpu import Q8_VS_TWIN_FACTOR, q8_distances

pytestmark = pytest.mark.gpu


def engine_for(path, ctx=CTX, **opts):
    e = E.Engine()
    for k, v in opts.items():
        e.set_option(k, v)
    e.load(path, ctx)
    return e


def routed_layers(name):
    return len(MODELS[name][7]) if MODELS[name][7] is not None else 2


# ------------------------------------------------------------------------------------------------ prompt forms, score, the public surface
@pytest.mark.parametrize("name", sorted(MODELS))
def test_engine_matches_the_routing_oracle_in_every_prompt_form(name, tmp_path_factory):
    """Prompt passes of 1 / 3 / 4 / 37 / 70 tokens, a chunked prefill 37 + 33, score over 37 positions; Engine.moe() and the describe fields"""
    ref = oracle_ref(name, tmp_path_factory)
    assert ref["gap"] >= 1.0          # (the guard's condition, on the reference this test uses)
    for wrong in WRONG:
        for T in GUARD_LENGTHS:
            assert dist(ref["prompt"][T], ref[wrong][T]) >= 10 * TOL
    shape, mix, arch, norms, n_exp, n_used, ie, layers, _ = MODELS[name]
    d = E.gguf_describe(ref["path"])
    assert (d["expert_count"], d["expert_used_count"], d["expert_feed_forward_length"], d["moe_layers"]) == (n_exp, n_used, ie or shape.inter, routed_layers(name))
    e = engine_for(ref["path"])
    assert e.moe() == routed_layers(name) and e.moe_experts() == (n_exp, n_used) and e.n_layers == 2 and e.qk_norm == (2 if norms else 0)
    for T in LENGTHS:
        got = e.forward(ref["tokens"][:T], 0)
        err = dist(got, ref["prompt"][T])
        print(name, "T", T, "engine - routing oracle: max |dlogit| =", err)
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
    """fused + graph (norm, route, gate | up, down are nodes of the captured token; the experts are chosen on the device), graph = 0, and fused = 0"""
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


# ------------------------------------------------------------------------------------------------ sequence slots, the packed pass, shared weights
@pytest.mark.parametrize("name", sorted(MODELS))
def test_sequence_slots_packed_pass_and_shared_weights(name, tmp_path_factory):
    ref = oracle_ref(name, tmp_path_factory)
    toks, fed = ref["tokens"], ref["fed"]
    e = engine_for(ref["path"], sequences=4)
    assert e.moe() == routed_layers(name)
    got, _ = e.forward_batch([0, 1, 2], [toks[:37], toks[:4], toks[:3]], [0, 0, 0])          # three prompts in one pass over the weights ...
    for s, T in enumerate((37, 4, 3)):
        assert dist(got[s], ref["prompt"][T]) <= TOL, (name, "packed", s, dist(got[s], ref["prompt"][T]))
    got, _ = e.forward_batch([0, 3], [[fed[0]], toks[:70]], [37, 0])                         # ... and mixed segments: a decode row beside a 70-token chunk
    assert dist(got[0], ref["steps"][0]) <= TOL and dist(got[1], ref["prompt"][70]) <= TOL, (name, dist(got[0], ref["steps"][0]), dist(got[1], ref["prompt"][70]))
    lg, nxt = e.decode_batch([0, 1, 2], [fed[1], 9, 10], [38, 4, 3])                         # a batched step over three slots, against each sequence alone
    for s, want in enumerate((ref["steps"][1], ref["slots"][0], ref["slots"][1])):
        assert np.isfinite(lg[s]).all() and dist(lg[s], want) <= TOL, (name, "decode_batch", s, dist(lg[s], want))
    assert dist(e.seq_forward(3, toks[:37], 0), ref["prompt"][37]) <= TOL
    e.close()
    solo = engine_for(ref["path"])          # a sharing sequence reads its source's expert tensors: the solo bits
    want = solo.forward(toks[:37], 0)
    want_step = solo.decode_fused(fed[0], 37, graph=True)
    b = E.Engine()
    b.load_shared(solo, CTX)
    assert b.moe() == routed_layers(name)
    assert np.array_equal(b.forward(toks[:37], 0), want) and np.array_equal(b.decode_fused(fed[0], 37, graph=True), want_step)
    assert dist(want_step, ref["steps"][0]) <= TOL
    b.close(); solo.close()


@pytest.mark.parametrize("level", [0, 1])
def test_expert_tensors_stay_raw_at_every_repack_level(level, tmp_path_factory):
    """moe4k (K-quant attention matrices, which repack) at repack 0 and 1 beside the default: the same oracle, the same bar"""
    ref = oracle_ref("moe4k", tmp_path_factory)
    e = engine_for(ref["path"], repack=level)
    assert dist(e.forward(ref["tokens"][:37], 0), ref["prompt"][37]) <= TOL
    assert dist(e.decode_fused(ref["fed"][0], 37, graph=True), ref["steps"][0]) <= TOL
    e.close()


# ------------------------------------------------------------------------------------------------ the 8-bit KV cache
def test_q8_kv_cache_on_a_routed_model(tmp_path_factory):
    """moe4k (heads of 128): the q8_0 engine against the F16 engine of the same model, and fused against unfused, within the factor the Qwen3 test
    uses (tests/test_engine_qwen2_gpu.py: 3 x) of what the same engines show on the DENSE twin of the file (the same attention tensors, a dense FFN)"""
    ref = oracle_ref("moe4k", tmp_path_factory)
    shape = MODELS["moe4k"][0]
    routed = q8_distances(ref["path"], ref["tokens"], ref["fed"], shape.heads, shape.kv_heads, shape.hd, False)
    twin = q8_distances(model_file("moe4k", tmp_path_factory, experts=None, overrides=None), ref["tokens"], ref["fed"], shape.heads, shape.kv_heads, shape.hd, False)
    fmt = lambda xs: " ".join("%.3g" % x for x in xs)
    print("moe4k q8_0 - f16 (37-token pass, 3-token pass, 8 steps):", fmt(routed[0]))
    print("moe4k q8_0 - f16 on the dense twin (the same):", fmt(twin[0]), "-> bar %.3g" % (Q8_VS_TWIN_FACTOR * max(twin[0])))
    print("moe4k q8_0 fused - unfused, 8 steps:", fmt(routed[1]))
    print("moe4k q8_0 fused - unfused on the twin:", fmt(twin[1]), "-> bar %.3g" % (Q8_VS_TWIN_FACTOR * max(twin[1])))
    assert max(routed[0]) <= Q8_VS_TWIN_FACTOR * max(twin[0]), (routed[0], twin[0])
    assert max(routed[1]) <= Q8_VS_TWIN_FACTOR * max(twin[1]), (routed[1], twin[1])


# ------------------------------------------------------------------------------------------------ refusals, the CLI, the generator, a Llama model
def test_tensor_parallelism_over_a_routed_model_is_refused(tmp_path_factory):
    path = model_file("moe8q8", tmp_path_factory)
    e = E.Engine()
    e.tp_configure(0, 2)
    with pytest.raises(_lib.NtkError) as ei:
        e.load(path, 128)
    assert ei.value.status == -2 and "ffn_gate_inp.weight" in str(ei.value) and "tensor parallelism" in str(ei.value)
    e.close()


def test_cli_runs_a_routed_file(tmp_path_factory):
    """`ntransformer -m <moe file>`: the configuration names the experts, and the greedy text is the Python engine's on the same file"""
    exe = os.path.join(os.path.dirname(E.__file__), "ntransformer")
    assert os.path.exists(exe), "CLI not built"
    path = model_file("moe8q8", tmp_path_factory)
    r = subprocess.run([exe, "-m", path, "-p", "hi there", "-c", "128", "-n", "16", "-t", "0", "--repeat-penalty", "1.0"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stderr + r.stdout).decode("utf-8", "replace")[-2000:]
    assert b"Experts: 8, used per token: 2, expert FFN width: 96" in r.stderr
    e = engine_for(path, ctx=128)
    ids = e.generate_tokens(e.tokenize("hi there"), 16, temperature=0.0, repeat_penalty=1.0)
    buf = C.create_string_buffer(4096)
    arr = (C.c_int * len(ids))(*ids)
    n = e.L.nt_engine_detokenize(e.h, arr, len(ids), buf, 4096)
    text = buf.raw[:n].replace(b"\0", b"")
    assert len(ids) == 16 and text and text in r.stdout, (ids, text, r.stdout[-500:])
    e.close()


def tiny_spec(mix, seed):
    return E.SynthSpec(256, 512, 2, 4, 2, 512, 256, 1e-6, 1e6, 256, 257, mix, seed)


@pytest.mark.parametrize("flavour,seed,arch,hd,ie", [("qwen3-moe8x2-i96:", 20260925, "qwen3moe", 64, 96), ("qwen3-hd128-moe4x2:", 20260925, "qwen3moe", 128, 512),
                                                     ("moe4x2-i256:", 20260926, "llama", 64, 256)])
def test_load_synthetic_runs_the_moe_flavours(flavour, seed, arch, hd, ie, tmp_path):
    """nt_engine_load_synthetic with a moe<E>x<K>[-i<I_e>] flavour (what `--synthetic qwen3-30b-a3b:Q8_0` runs, at the tiny shape): the logits are the bits
    of an engine that loaded the file nt_synth_write_gguf writes for the same spec, and within 1e-3 of the routing oracle over that file.  The spec's seed
    was searched on the CPU for the routing-gap condition of tests/test_moe_cpu.py (moe4x2-i256 misses it at 20260925: 0.89 bars), asserted here."""
    spec = tiny_spec((flavour + "Q8_0").encode(), seed)
    path = str(tmp_path / "synth.gguf")
    E.synth_write_gguf(path, spec, 2)
    d = E.gguf_describe(path)
    assert d["architecture"] == arch and d["moe_layers"] == 2 and d["head_dim"] == hd and d["expert_feed_forward_length"] == ie
    toks = prompt_tokens(37)
    from moe_ref import MoEOracle
    m = MoEOracle(path, 128)
    want, want_step = m.forward(toks, 0), m.forward([7], 37)
    s = E.Engine()
    s.load_synthetic(spec, 128)
    f = engine_for(path, ctx=128)
    assert s.moe() == 2 == f.moe() and s.moe_experts() == f.moe_experts() == (d["expert_count"], d["expert_used_count"])
    assert s.weight_bytes() == f.weight_bytes() == sum(t["nbytes"] for t in d["tensors"])
    got, got_f = s.forward(toks, 0), f.forward(toks, 0)
    step, step_f = s.decode_fused(7, 37, graph=True), f.decode_fused(7, 37, graph=True)
    print(flavour, "gap ratio %.3g; engine - oracle: prompt %.3g, step %.3g" % (m.min_gap_ratio(), dist(got, want), dist(step, want_step)))
    assert np.isfinite(got).all() and np.isfinite(step).all()
    assert np.array_equal(got, got_f) and np.array_equal(step, step_f)
    assert m.min_gap_ratio() >= 1.0
    assert dist(got, want) <= TOL and dist(step, want_step) <= TOL, (dist(got, want), dist(step, want_step))
    s.close(); f.close()


def test_a_llama_model_routes_nothing_and_matches_the_plain_oracle():
    """an existing golden model: nt_engine_moe = 0, and its logits are the PLAIN oracle's, prompt and decode (its launches are what they were)"""
    path = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    toks = prompt_tokens(37)
    m = O.OracleModel(path, 256)
    want = m.forward(toks, 0)
    want_step = m.forward([7], 37)
    e = engine_for(path, ctx=256)
    assert e.moe() == 0 and e.moe_experts() == (0, 0)
    d = E.gguf_describe(path)
    assert (d["expert_count"], d["expert_used_count"], d["expert_feed_forward_length"], d["moe_layers"]) == (0, 0, 0, 0)
    assert dist(e.forward(toks, 0), want) <= TOL
    assert dist(e.decode_fused(7, 37, graph=True), want_step) <= TOL
    e.close()
    u = E.Engine()
    assert u.moe() == -1          # unloaded
    u.close()
