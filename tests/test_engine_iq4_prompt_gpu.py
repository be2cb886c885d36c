"""GPU tests of the engine's prompt pass on models with IQ4 matrices at prompt lengths that take the FP16 matrix-core GEMM's chunk form, with one and with two
64-token chunks (40 and 100 tokens): the two-layer IQ4_XS-mix model (Q | K | V = IQ4_XS | IQ4_XS | Q5_K, Q6_K LM head) and the plain IQ4_NL one of
tests/test_engine_iq4_gpu.py, from the decode repack (repack = 2: one resident copy, no unpack of the IQ4_XS matrices) and from the GGUF bytes (repack = 0),
against the oracle on their F32 twins at the project's bar, 1e-3, on the logits of forward and the log-probabilities of score.  The last test pins the PATH:
with option f16_prefill = 0 the projections run on the F32 matrix cores, with 1 on the FP16 ones -- both within the bar, and not the same bits.  (The plain
IQ4_NL model is the one that pins it: without an FP16 decoder for the type both settings take the same kernels.  The IQ4_XS mix has a Q5_K attn_v, which
changes its path with the option whatever the IQ4_XS matrices do.)
Run on the MI355X box:  python -m pytest tests/test_engine_iq4_prompt_gpu.py -m gpu -x -q -s"""
import numpy as np
import pytest

from ntransformer_amd import engine as E, gguf as G, ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL, CTX, SEED = 1e-3, 128, 20261126
MODELS = {"IQ4_XS": G.GGML_IQ4_XS, "IQ4_NL": G.GGML_IQ4_NL}
LENGTHS = (40, 100)   # the shorter prompt is the head of the longer one: one walk of the oracle serves both
PROMPT = [256] + [int(t) for t in np.random.Generator(np.random.Philox(key=[SEED, 4])).integers(0, 256, max(LENGTHS) - 1)]

@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> (model file, the oracle's logits on the F32 twin behind every prefix of PROMPT [100, V])"""
    ops.init(0)
    d, out = tmp_path_factory.mktemp("iq4_prompt"), {}
    for name, gt in MODELS.items():
        path, twin = str(d / (name + ".gguf")), str(d / (name + "_f32.gguf"))
        assert gt in G.make_synthetic_llama(path, G.TINY, name, seed=SEED).values()
        G.write_f32_twin(path, twin, widen=(G.GGML_IQ4_XS, G.GGML_IQ4_NL, G.GGML_Q4_K, G.GGML_Q5_K, G.GGML_Q6_K))
        m = O.OracleModel(twin, CTX)
        out[name] = (path, np.stack([m.forward([t], i) for i, t in enumerate(PROMPT)]).astype(np.float64))
    return out

def worst(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())

@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("repack", [2, 0])
@pytest.mark.parametrize("n", LENGTHS)
def test_prompt_and_score_meet_the_twin(name, repack, n, reference):
    path, rows = reference[name]
    eng = E.Engine()
    eng.set_option("repack", repack)
    eng.load(path, CTX)
    assert (eng.repacked_bytes() > 0) == (repack != 0 and name != "IQ4_NL")
    e_fwd = worst(eng.forward(PROMPT[:n], 0), rows[n - 1])
    l = rows[:n]
    lse = np.log(np.exp(l - l.max(axis=1, keepdims=True)).sum(axis=1)) + l.max(axis=1)
    e_score = worst(eng.score(PROMPT[:n]), [l[i, PROMPT[i + 1]] - lse[i] for i in range(n - 1)] + [0.0])
    eng.close()
    print("%s repack=%s, %d tokens: forward %.3g, score %.3g (bar %g)" % (name, repack, n, e_fwd, e_score, TOL))
    assert e_fwd <= TOL and e_score <= TOL   # (a NaN fails it)

@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_f16_prefill_option_changes_the_bits_of_a_prompt(name, reference, n=LENGTHS[0]):
    path, rows = reference[name]
    eng, got = E.Engine(), []
    eng.load(path, CTX)
    for on in (0, 1):   # (the option may change at any time)
        eng.set_option("f16_prefill", on)
        got.append(np.array(eng.forward(PROMPT[:n], 0), np.float32))
    eng.close()
    errs = [worst(g, rows[n - 1]) for g in got]
    print("%s, %d tokens: f16_prefill = 0 / 1: %.3g / %.3g from the twin (bar %g), %d logits differ" % (name, n, errs[0], errs[1], TOL, int((got[0] != got[1]).sum())))
    assert all(e <= TOL for e in errs)
    assert not np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
