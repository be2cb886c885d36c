"""Mixture-of-experts models through the engine with the prompt pass's expert FFN on the grouped matrix-core GEMM (csrc/moe_gemm.hip; options moe_gemm,
moe_gemm_min_rows): the four models of tests/moe_ref.py with moe_gemm_min_rows = 2, so that every pass of two rows or more takes the GEMM form, against
MoEOracle at the bars of tests/test_engine_moe_gpu.py (logits 1e-3, score 2e-3; the guard of tests/test_moe_cpu.py holds for the same passes).

Prompts of 3 / 4 / 37 / 70 tokens and the chunked 37 + 33, score over 37, the packed pass with the mixed segments of the existing engine test, decode_batch
over three slots, seq_forward, kv_cache = q8_0 on moe4k at the existing factor bar, eight fused decode steps behind a GEMM-form prompt.

Option switching: moe_gemm 1 -> 0 -> 1 on a 37-token prompt gives other bits in between and the first bits back; with moe_gemm = 0 every pass, and a
one-row pass at any setting, hashes to tests/golden/moe_pass_bits.json, recorded from the build BEFORE this feature (tools/record_moe_bits.py,
tests/moe_bits.py); a golden Llama model has the same bits under both settings; moe8q8's expert width of 96 RUNS the GEMM (its bits differ from option 0).

Run on the MI355X box:  python -m pytest tests/test_engine_moe_gemm_gpu.py -m gpu -x -q -s"""
import json
import os

import numpy as np
import pytest

import moe_bits as B
import test_engine_qwen2_gpu as Q2
from conftest import GOLDEN
from moe_ref import CTX, MODELS, N_STEPS, SCORE_TOL, TOL, dist, model_file, oracle_ref, prompt_tokens
from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from score_ref import logprob_ref

pytestmark = pytest.mark.gpu
GEMM_LENGTHS = (3, 4, 37, 70)


def engine_for(path, ctx=CTX, **opts):
    e = E.Engine()
    for k, v in opts.items():
        e.set_option(k, v)
    e.load(path, ctx)
    return e


@pytest.mark.parametrize("name", sorted(MODELS))
def test_prompt_forms_on_the_gemm_against_the_routing_oracle(name, tmp_path_factory):
    ref = oracle_ref(name, tmp_path_factory)
    assert ref["gap"] >= 1.0
    e = engine_for(ref["path"], moe_gemm_min_rows=2)
    off = engine_for(ref["path"], moe_gemm=0)
    for T in GEMM_LENGTHS:
        got = e.forward(ref["tokens"][:T], 0)
        err = dist(got, ref["prompt"][T])
        print(name, "T", T, "GEMM form - routing oracle: max |dlogit| =", err)
        assert np.isfinite(got).all() and err <= TOL, (name, T, err)
        assert not np.array_equal(got, off.forward(ref["tokens"][:T], 0)), (name, T, "the GEMM form did not run")          # (moe8q8: a width of 96 runs it)
    e.forward(ref["tokens"][:37], 0)
    err = dist(e.forward(ref["tokens"][37:70], 37), ref["chunked"])
    print(name, "chunked 37 + 33: max |dlogit| =", err)
    assert err <= TOL
    lp = e.score(ref["tokens"][:37])
    want, _ = logprob_ref(ref["all37"], ref["tokens"][1:37] + [-1])
    print(name, "score over 37 positions: max |dlogprob| =", float(np.abs(lp - want).max()))
    assert np.abs(lp - want).max() <= SCORE_TOL
    e.close(); off.close()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_eight_fused_decode_steps_behind_a_gemm_form_prompt(name, tmp_path_factory):
    ref = oracle_ref(name, tmp_path_factory)
    e = engine_for(ref["path"], moe_gemm_min_rows=2)
    e.forward(ref["tokens"][:37], 0)
    for i, tok in enumerate(ref["fed"]):
        got = e.decode_fused(tok, 37 + i, graph=True)
        err = dist(got, ref["steps"][i])
        assert np.isfinite(got).all() and err <= TOL, (name, i, err)
    assert len(ref["fed"]) == N_STEPS
    e.close()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_packed_pass_batched_step_and_seq_forward(name, tmp_path_factory):
    ref = oracle_ref(name, tmp_path_factory)
    toks, fed = ref["tokens"], ref["fed"]
    e = engine_for(ref["path"], sequences=4, moe_gemm_min_rows=2)
    got, _ = e.forward_batch([0, 1, 2], [toks[:37], toks[:4], toks[:3]], [0, 0, 0])
    for s, T in enumerate((37, 4, 3)):
        assert dist(got[s], ref["prompt"][T]) <= TOL, (name, "packed", s, dist(got[s], ref["prompt"][T]))
    got, _ = e.forward_batch([0, 3], [[fed[0]], toks[:70]], [37, 0])          # mixed segments: a decode row beside a 70-token chunk
    assert dist(got[0], ref["steps"][0]) <= TOL and dist(got[1], ref["prompt"][70]) <= TOL, (name, dist(got[0], ref["steps"][0]), dist(got[1], ref["prompt"][70]))
    lg, _ = e.decode_batch([0, 1, 2], [fed[1], 9, 10], [38, 4, 3])          # three rows: the GEMM form at min_rows = 2
    for s, want in enumerate((ref["steps"][1], ref["slots"][0], ref["slots"][1])):
        assert np.isfinite(lg[s]).all() and dist(lg[s], want) <= TOL, (name, "decode_batch", s, dist(lg[s], want))
    assert dist(e.seq_forward(3, toks[:37], 0), ref["prompt"][37]) <= TOL
    e.close()


def test_q8_kv_cache_on_a_routed_model_with_the_gemm(tmp_path_factory, monkeypatch):
    """tests/test_engine_moe_gpu.py's q8_0 test with every engine at moe_gemm_min_rows = 2 (the 37- and the 3-token pass on the GEMM): the same factor bar"""
    ref = oracle_ref("moe4k", tmp_path_factory)
    shape = MODELS["moe4k"][0]
    plain = Q2.engine_for
    monkeypatch.setattr(Q2, "engine_for", lambda path, *a, **kw: plain(path, *a, **dict(kw, moe_gemm_min_rows=2)))
    routed = Q2.q8_distances(ref["path"], ref["tokens"], ref["fed"], shape.heads, shape.kv_heads, shape.hd, False)
    twin = Q2.q8_distances(model_file("moe4k", tmp_path_factory, experts=None, overrides=None), ref["tokens"], ref["fed"], shape.heads, shape.kv_heads, shape.hd, False)
    print("moe4k GEMM form q8_0 - f16:", " ".join("%.3g" % x for x in routed[0]), "-> bar %.3g" % (Q2.Q8_VS_TWIN_FACTOR * max(twin[0])))
    assert max(routed[0]) <= Q2.Q8_VS_TWIN_FACTOR * max(twin[0]), (routed[0], twin[0])
    assert max(routed[1]) <= Q2.Q8_VS_TWIN_FACTOR * max(twin[1]), (routed[1], twin[1])


# ------------------------------------------------------------------------------------------------ the options
@pytest.mark.parametrize("name", sorted(MODELS))
def test_switching_the_option_and_the_parents_bits(name, tmp_path_factory):
    with open(B.GOLDEN_FILE) as f:
        gold = json.load(f)["cases"]
    path = B.model_path(name, tmp_path_factory)
    toks = prompt_tokens()
    e = engine_for(path, moe_gemm_min_rows=2)
    first = e.forward(toks[:37], 0)
    e.set_option("moe_gemm", 0)
    between = e.forward(toks[:37], 0)
    e.set_option("moe_gemm", 1)
    back = e.forward(toks[:37], 0)
    assert not np.array_equal(first, between) and np.array_equal(first, back)
    assert dist(first, between) <= 2 * TOL
    assert B.digest(between) == gold["%s/p37" % name]          # option 0: the build before the feature, bit for bit
    assert B.digest(e.forward(toks[:1], 0)) == gold["%s/p1" % name]          # one row, GEMM on, threshold 2: the GEMV launches
    e.set_option("moe_gemm_min_rows", 1)          # (1 is accepted; a one-row pass still never takes the GEMM)
    assert B.digest(e.forward(toks[:1], 0)) == gold["%s/p1" % name]
    # the decode steps behind a prompt run with option 0, the option back on for the steps: the parent's bits
    e.set_option("moe_gemm", 0)
    e.forward(toks[:37], 0)
    e.set_option("moe_gemm", 1)
    steps = np.stack([e.decode_fused(tok, 37 + i, graph=True) for i, tok in enumerate(B.FED)])
    assert B.digest(steps) == gold["%s/steps" % name]
    e.close()
    off = engine_for(path, moe_gemm=0)          # every pass of the recording with option 0
    for k, v in B.run_passes(off).items():
        assert B.digest(v) == gold["%s/%s" % (name, k)], (name, k)
    off.close()
    dflt = engine_for(path)          # the default settings: the one-row pass is the parent's
    assert B.digest(dflt.forward(toks[:1], 0)) == gold["%s/p1" % name]
    dflt.close()


def test_a_llama_model_has_the_same_bits_under_both_settings():
    path = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    toks = prompt_tokens(37)
    got = []
    for opts in (dict(), dict(moe_gemm=0), dict(moe_gemm=1, moe_gemm_min_rows=2)):
        e = engine_for(path, ctx=256, **opts)
        assert e.moe() == 0
        got.append((e.forward(toks, 0), e.decode_fused(7, 37, graph=True)))
        e.close()
    for p, s in got[1:]:
        assert np.array_equal(p, got[0][0]) and np.array_equal(s, got[0][1])


def test_bad_option_values_are_refused(tmp_path_factory):
    e = engine_for(B.model_path("moe8q8", tmp_path_factory))
    toks = prompt_tokens()
    want = e.forward(toks[:37], 0)
    for key, v in (("moe_gemm", "2"), ("moe_gemm", "yes"), ("moe_gemm_min_rows", "0"), ("moe_gemm_min_rows", "1025"), ("moe_gemm_min_rows", "x")):
        with pytest.raises(_lib.NtkError) as ei:
            e.set_option(key, v)
        assert ei.value.status == -2 and key in str(ei.value)
    assert np.array_equal(e.forward(toks[:37], 0), want)          # a refusal changes nothing
    e.close()
