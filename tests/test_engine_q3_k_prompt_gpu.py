"""GPU tests of the engine's prompt pass on models with Q3_K matrices at prompt lengths that take the FP16 matrix-core GEMM's chunk form, with one and with
two 64-token chunks (40 and 100 tokens; tests/test_engine_q3_k_gpu.py's 5 and 9 tokens take the K-slice form): the two-layer Q3_K_M model (Q | K | V = Q3_K | Q3_K | Q5_K, heads of 128) and the plain
Q3_K one with heads of 64, from the decode repack (repack = 2: one resident copy, no unpack) and from the GGUF bytes (repack = 0), against the oracle on
their F32 twins at the project's bar, 1e-3, on the logits of forward and the log-probabilities of score.  They pin the pass's result, not its path: the F32
fallback meets the same bar, and that the FP16 form is the one taken is read off a kernel trace (profiles/q3_k_prompt.txt).
Run on the MI355X box:  python -m pytest tests/test_engine_q3_k_prompt_gpu.py -m gpu -x -q -s"""
import numpy as np
import pytest

from ntransformer_amd import engine as E, gguf as G, ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL, CTX, SEED = 1e-3, 128, 20261126
HD128 = G.LlamaShape("q3hd128", 512, 1024, 2, 4, 2, 512, ctx=CTX, bos=256, eos=257)
MODELS = {"Q3_K_M": (HD128, "Q3_K_M"), "Q3_K-hd64": (G.TINY, "Q3_K")}
LENGTHS = (40, 100)   # the shorter prompt is the head of the longer one: one walk of the oracle serves both
PROMPT = [256] + [int(t) for t in np.random.Generator(np.random.Philox(key=[SEED, 3])).integers(0, 256, max(LENGTHS) - 1)]

@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> (model file, the oracle's logits on the F32 twin behind every prefix of PROMPT [100, V])"""
    ops.init(0)
    d, out = tmp_path_factory.mktemp("q3k_prompt"), {}
    for name, (shape, mix) in MODELS.items():
        path, twin = str(d / (name + ".gguf")), str(d / (name + "_f32.gguf"))
        assert G.GGML_Q3_K in G.make_synthetic_llama(path, shape, mix, seed=SEED).values()
        G.write_f32_twin(path, twin, widen=(G.GGML_Q3_K, G.GGML_Q4_K, G.GGML_Q5_K, G.GGML_Q6_K))
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
    assert (eng.repacked_bytes() > 0) == (repack != 0)
    e_fwd = worst(eng.forward(PROMPT[:n], 0), rows[n - 1])
    l = rows[:n]
    lse = np.log(np.exp(l - l.max(axis=1, keepdims=True)).sum(axis=1)) + l.max(axis=1)
    e_score = worst(eng.score(PROMPT[:n]), [l[i, PROMPT[i + 1]] - lse[i] for i in range(n - 1)] + [0.0])
    eng.close()
    print("%s repack=%s, %d tokens: forward %.3g, score %.3g (bar %g)" % (name, repack, n, e_fwd, e_score, TOL))
    assert e_fwd <= TOL and e_score <= TOL   # (a NaN fails it)
