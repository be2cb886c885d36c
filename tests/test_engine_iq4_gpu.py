"""GPU tests of the engine on models with IQ4 matrices: a two-layer file of the IQ4_XS mix (Q | K | V = IQ4_XS | IQ4_XS | Q5_K, IQ4_XS embedding, Q6_K LM
head: the matrix-core decode GEMV over the repack, its raw readers behind an unpack) and a plain IQ4_NL one (the raw fused GEMV in decode), against the
oracle on their F32 twins (gguf.write_f32_twin: the same weights as floats, no quantiser in the reference).  The same body runs a Q4_K_M file as the
control: the twin comparison itself holds at the project's bar, 1e-3 on every logit; the log-probabilities of score at 2e-3.
Run on the MI355X box:  python -m pytest tests/test_engine_iq4_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL, CTX, SEED = 1e-3, 128, 20261126
MODELS = {"IQ4_XS": "IQ4_XS", "IQ4_NL": "IQ4_NL", "Q4_K_M-control": "Q4_K_M"}
PROMPTS = [[256] + [int(t) for t in np.random.Generator(np.random.Philox(key=[SEED, k])).integers(0, 256, n - 1)] for k, n in ((1, 3), (2, 37))]
FED = [7, 100, 3, 255, 0, 41, 200, 9]   # the tokens of the eight decode steps behind PROMPTS[1]


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> (model file, oracle logits on the F32 twin: behind every prefix of PROMPTS[0] [3, V], behind both prompts [2, V], behind FED after
    PROMPTS[1] [8, V], behind FED[0] after PROMPTS[0] [V])"""
    ops.init(0)
    d, out = tmp_path_factory.mktemp("iq4"), {}
    for name, mix in MODELS.items():
        path, twin = str(d / (name + ".gguf")), str(d / (name + "_f32.gguf"))
        types = G.make_synthetic_llama(path, G.TINY, mix, seed=SEED)
        assert (G.NAME_TO_GGML.get(mix) in types.values()) == (name != "Q4_K_M-control")
        G.write_f32_twin(path, twin, widen=(G.GGML_IQ4_XS, G.GGML_IQ4_NL, G.GGML_Q4_K, G.GGML_Q5_K, G.GGML_Q6_K))
        m = O.OracleModel(twin, CTX)
        rows = np.stack([m.forward([t], i) for i, t in enumerate(PROMPTS[0])])
        m = O.OracleModel(twin, CTX)
        ends = [m.forward(PROMPTS[0], 0)]
        short = m.forward([FED[0]], 3)
        m = O.OracleModel(twin, CTX)
        ends.append(m.forward(PROMPTS[1], 0))
        steps = np.stack([m.forward([t], 37 + i) for i, t in enumerate(FED)])
        out[name] = (path, rows, np.stack(ends), steps, short)
    return out


def worst(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# (name, repack, captured): the default (one resident copy, raw readers behind an unpack) with captured and with eager steps; the raw GGUF blocks everywhere
@pytest.mark.parametrize("name,repack,graph", [(n, 2, g) for n in sorted(MODELS) for g in (True, False)] + [("IQ4_XS", 0, True)])
def test_prompts_eight_decode_steps_and_score_meet_the_twin(name, repack, graph, reference):
    path, rows, ends, steps, _ = reference[name]
    eng = E.Engine()
    eng.set_option("repack", repack)
    eng.load(path, CTX)
    assert (eng.repacked_bytes() > 0) == (repack != 0 and name != "IQ4_NL")
    l = rows.astype(np.float64)
    lse = np.log(np.exp(l - l.max(axis=1, keepdims=True)).sum(axis=1)) + l.max(axis=1)
    e_score = worst(eng.score(PROMPTS[0]), [l[i, PROMPTS[0][i + 1]] - lse[i] for i in range(2)] + [0.0])
    errs = [worst(eng.forward(PROMPTS[0], 0), ends[0]), worst(eng.forward(PROMPTS[1], 0), ends[1])]
    errs += [worst(eng.decode_fused(t, 37 + i, graph=graph), steps[i]) for i, t in enumerate(FED)]
    eng.close()
    print("%s repack=%s graph=%s: prompts of 3 and 37, eight steps %s, score %.3g" % (name, repack, graph, ["%.3g" % e for e in errs], e_score))
    assert all(e <= TOL for e in errs) and e_score <= 2e-3   # (a NaN fails it)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_batched_step_of_two_rows_meets_the_twin(name, reference):
    path, _, ends, steps, short = reference[name]
    eng = E.Engine()
    eng.set_option("sequences", 2)
    eng.load(path, CTX)
    e_prompt = [worst(eng.seq_forward(s, p, 0), ends[s]) for s, p in enumerate(PROMPTS)]
    got, _ = eng.decode_batch([0, 1], [FED[0], FED[0]], [len(p) for p in PROMPTS])
    eng.close()
    e_step = worst(got, [short, steps[0]])
    print("%s: slot prompts %s, decode_batch of two rows %.3g" % (name, e_prompt, e_step))
    assert all(e <= TOL for e in e_prompt + [e_step])


def test_an_iq4_xs_expert_tensor_is_refused_at_load_by_name(tmp_path):
    path = str(tmp_path / "iq4_experts.gguf")
    G.make_synthetic_llama(path, G.MOE_8Q8, "Q8_0", seed=SEED, arch="qwen3moe", qk_norm=0.5, experts=8, experts_used=2, expert_inter=256, overrides={"ffn_up_exps": "IQ4_XS"})
    eng = E.Engine()
    with pytest.raises(_lib.NtkError) as ei:
        eng.load(path, CTX)
    assert ei.value.status == -1 and "ffn_up_exps.weight" in str(ei.value) and eng.moe() == -1, str(ei.value)
    eng.close()
