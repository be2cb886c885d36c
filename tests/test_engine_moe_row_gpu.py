"""One-row passes of mixture-of-experts models on the row form of the routed FFN (csrc/moe_row.hip; option moe_row, default 1), over the four models of
tests/moe_ref.py: Engine.moe_row() counts the routed layers (0 with the option off); a 1-token prompt, the eight fed fused graph steps of tests/moe_bits.py and
the same steps eager give the same logits with the option 1, then 0, then 1, and the digests of tests/golden/moe_pass_bits.json; steps fed the oracle's tokens
lie within 1e-3 of the routing oracle.  A Llama golden model reports 0 and keeps its bits; bad option values are refused."""
import json
import os

import numpy as np
import pytest

import moe_bits as B
from conftest import GOLDEN
from moe_ref import MODELS, TOL, dist, oracle_ref, prompt_tokens
from ntransformer_amd import _lib
from test_engine_moe_gemm_gpu import engine_for

pytestmark = pytest.mark.gpu


def one_row_passes(e, toks):
    """(a 1-token prompt, eight fused graph steps behind a 37-token prompt, the same steps eager)"""
    p1 = e.forward(toks[:1], 0)
    steps = []
    for graph in (True, False):
        e.forward(toks[:37], 0)
        steps.append(np.stack([e.decode_fused(tok, 37 + i, graph=graph) for i, tok in enumerate(B.FED)]))
    return p1, steps[0], steps[1]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_one_row_passes_keep_their_bits_under_the_option(name, tmp_path_factory):
    with open(B.GOLDEN_FILE) as f:
        gold = json.load(f)["cases"]
    ref = oracle_ref(name, tmp_path_factory)
    toks = ref["tokens"]
    routed = 2 if MODELS[name][7] is None else len(MODELS[name][7])
    e = engine_for(ref["path"], moe_gemm=0)          # (the 37-token prompt of the recording ran on the expert GEMV)
    assert e.moe() == routed and e.moe_row() == routed
    runs = []
    for on in (1, 0, 1):
        e.set_option("moe_row", on)
        assert e.moe_row() == (routed if on else 0)
        runs.append(one_row_passes(e, toks))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert B.digest(runs[0][0]) == gold["%s/p1" % name] and B.digest(runs[0][1]) == gold["%s/steps" % name]
    e.forward(toks[:37], 0)
    for i, tok in enumerate(ref["fed"]):
        err = dist(e.decode_fused(tok, 37 + i, graph=True), ref["steps"][i])
        assert err <= TOL, (name, i, err)
    e.close()


def test_a_llama_model_reports_zero_and_keeps_its_bits():
    path = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    toks = prompt_tokens(37)
    got = []
    for on in (1, 0):
        e = engine_for(path, ctx=256, moe_row=on)
        assert e.moe() == 0 and e.moe_row() == 0
        got.append((e.forward(toks, 0), e.decode_fused(7, 37, graph=True)))
        e.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def test_bad_option_values_are_refused(tmp_path_factory):
    e = engine_for(B.model_path("moe8q8", tmp_path_factory))
    for v in ("2", "yes", "-1", ""):
        with pytest.raises(_lib.NtkError) as ei:
            e.set_option("moe_row", v)
        assert ei.value.status == -2 and "moe_row" in str(ei.value)
    assert e.moe_row() == 2          # a refusal changes nothing
    e.close()
