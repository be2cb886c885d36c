"""GPU tests of the engine on models with Q2_K matrices: a two-layer Q2_K_MIX model (Q | K | V = Q2_K | Q2_K | Q4_K at four query heads per KV head, Q3_K
attn_output and ffn_down, Q2_K gate | up and embedding, Q6_K LM head; heads of 128) and a plain Q2_K one with heads of 64, against the oracle on their F32
twins (gguf.write_f32_twin: the same weights as floats, no quantiser in the reference).  The same body runs a Q4_K_M file as the control: the twin comparison
itself holds at the project's bar, 1e-3 (tests/test_engine_gpu.py), on every logit and on the log-probabilities of score.
Run on the MI355X box:  python -m pytest tests/test_engine_q2_k_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL, CTX, SEED = 1e-3, 128, 20261127
HD128 = G.LlamaShape("q2hd128", 512, 1024, 2, 4, 1, 512, ctx=CTX, bos=256, eos=257)
MODELS = {"Q2_K_MIX": (HD128, "Q2_K_MIX"), "Q2_K-hd64": (G.TINY, "Q2_K"), "Q4_K_M-control": (HD128, "Q4_K_M")}
PROMPTS = [[256] + [int(t) for t in np.random.Generator(np.random.Philox(key=[SEED, k])).integers(0, 256, n - 1)] for k, n in ((1, 5), (2, 9))]
NEXT = [7, 100]


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> (model file, oracle logits on the F32 twin: behind every prefix of PROMPTS[0] [5, V], behind both prompts [2, V], behind NEXT [2, V])"""
    ops.init(0)
    d, out = tmp_path_factory.mktemp("q2k"), {}
    for name, (shape, mix) in MODELS.items():
        path, twin = str(d / (name + ".gguf")), str(d / (name + "_f32.gguf"))
        types = G.make_synthetic_llama(path, shape, mix, seed=SEED)
        assert (G.GGML_Q2_K in types.values()) == (name != "Q4_K_M-control")
        if name == "Q2_K_MIX": assert types["blk.0.attn_v.weight"] == G.GGML_Q4_K
        G.write_f32_twin(path, twin, widen=(G.GGML_Q2_K, G.GGML_Q3_K, G.GGML_Q4_K, G.GGML_Q5_K, G.GGML_Q6_K))
        m = O.OracleModel(twin, CTX)
        rows, ends, steps = np.stack([m.forward([t], i) for i, t in enumerate(PROMPTS[0])]), [], []
        for p, t in zip(PROMPTS, NEXT):
            m = O.OracleModel(twin, CTX)
            ends.append(m.forward(p, 0))
            steps.append(m.forward([t], len(p)))
        out[name] = (path, rows, np.stack(ends), np.stack(steps))
    return out


def worst(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("repack", [2, 0])   # the default (one resident copy, raw readers behind an unpack) and the raw GGUF blocks everywhere
def test_prompt_captured_step_and_score_meet_the_twin(name, repack, reference):
    path, rows, ends, steps = reference[name]
    eng = E.Engine()
    eng.set_option("repack", repack)
    eng.load(path, CTX)
    assert (eng.repacked_bytes() > 0) == (repack != 0)
    errs = [worst(eng.forward(PROMPTS[0], 0), ends[0])] + [worst(eng.decode_fused(NEXT[0], 5, graph=True), steps[0]) for _ in range(3)]   # capture, two replays
    l = rows.astype(np.float64)
    lse = np.log(np.exp(l - l.max(axis=1, keepdims=True)).sum(axis=1)) + l.max(axis=1)
    e_score = worst(eng.score(PROMPTS[0]), [l[i, PROMPTS[0][i + 1]] - lse[i] for i in range(4)] + [0.0])
    eng.close()
    print("%s repack=%s: prompt, captured step x 3 %s, score %.3g" % (name, repack, ["%.3g" % e for e in errs], e_score))
    assert all(e <= TOL for e in errs + [e_score])   # (a NaN fails it)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_batched_step_of_two_rows_meets_the_twin(name, reference):
    path, _, ends, steps = reference[name]
    eng = E.Engine()
    eng.set_option("sequences", 2)
    eng.load(path, CTX)
    e_prompt = [worst(eng.seq_forward(s, p, 0), ends[s]) for s, p in enumerate(PROMPTS)]
    got, _ = eng.decode_batch([0, 1], NEXT, [len(p) for p in PROMPTS])
    eng.close()
    print("%s: slot prompts %s, decode_batch of two rows %.3g" % (name, e_prompt, worst(got, steps)))
    assert all(e <= TOL for e in e_prompt + [worst(got, steps)])


def test_the_one_to_one_sequence_refuses_a_q2_k_model_at_load(reference):
    eng = E.Engine()
    eng.set_option("fused", 0)
    with pytest.raises(_lib.NtkError, match=r"blk\.0\.attn_q\.weight with option fused = 0"):
        eng.load(reference["Q2_K-hd64"][0], CTX)
    eng.load(reference["Q4_K_M-control"][0], CTX)   # (the option alone refuses nothing)
    eng.close()
