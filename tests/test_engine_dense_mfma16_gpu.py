"""The prompt pass of F16 / BF16 models on the 16-bit matrix cores (ntk_gemm_dense16 behind the engine; option `dense_mfma16`, default 1) against the oracle.

Models as in tests/test_engine_unquantised_gpu.py: gguf.TINY (hidden 256, 4 heads of 64, 2 KV heads, 2 layers, vocabulary 512); the oracle reads BF16 models
through their F32 twin (gguf.write_f32_twin: the same values, exactly).  Bars: that file's TOL = 1e-3 on logits, 2 TOL on log-probabilities.  Every batched
prompt projection of these models -- Q | K | V and gate | up as one launch each, Wo and down with the residual, the LM head over more than one row -- goes
through the new kernel from 32 tokens on (below, the engine keeps the F32-MFMA form, which is as fast there: csrc/gemm_dense16_plan.h); `dense_mfma16` = 0 is
the F32-MFMA form of the same tree at every length.

Run on the MI355X box:  python -m pytest tests/test_engine_dense_mfma16_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import _lib, ops
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-3
CTX = 128
SEED = 20261021


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[SEED, seed]))


def tokens(seed, n):
    return [G.TINY.bos] + [int(t) for t in rng(seed).integers(0, 256, n - 1)]


PROMPT = tokens(1, 70)
FED = [int(t) for t in rng(2).integers(0, 256, 8)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{mix: (engine file, oracle file)}"""
    d = tmp_path_factory.mktemp("dense_mfma16")
    bf, twin, f16 = str(d / "tiny_bf16.gguf"), str(d / "tiny_bf16_as_f32.gguf"), str(d / "tiny_f16.gguf")
    G.make_synthetic_llama(bf, G.TINY, "BF16", seed=SEED)
    G.write_f32_twin(bf, twin)
    G.make_synthetic_llama(f16, G.TINY, "F16", seed=SEED)
    return {"BF16": (bf, twin), "F16": (f16, f16)}


@pytest.fixture(scope="module")
def oracle_rows(files):
    """{mix: logits behind every prefix of PROMPT [70, vocab], and behind 8 teacher-forced tokens after the first 37 [8, vocab]}: computed once, read-only"""
    out = {}
    for mix, (_, ofile) in files.items():
        m = O.OracleModel(ofile, CTX)
        rows = np.stack([m.forward([t], i) for i, t in enumerate(PROMPT)])
        m = O.OracleModel(ofile, CTX)
        m.forward(PROMPT[:37], 0)
        dec = np.stack([m.forward([t], 37 + i) for i, t in enumerate(FED)])
        rows.setflags(write=False)
        dec.setflags(write=False)
        out[mix] = (rows, dec)
    return out


def load(path, ctx=CTX, **options):
    eng = E.Engine()
    before = ("kv_cache", "sequences", "batch_kv_q8")
    for k, v in options.items():
        if k in before:
            eng.set_option(k, v)
    eng.load(path, ctx)
    for k, v in options.items():
        if k not in before:
            eng.set_option(k, v)
    return eng


def worst(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("mix", ["BF16", "F16"])
def test_prompt_passes_meet_the_oracle(mix, files, oracle_rows):
    """2, 3, 17 tokens (lengths the engine keeps on the F32-MFMA form), 37 and 70 (the new kernel: a ragged chunk; two chunks), 20 + 17 chunked, and 8 decode
    steps behind a 37-token prompt"""
    rows, dec = oracle_rows[mix]
    eng = load(files[mix][0])
    eng.set_option("dense_mfma16", 1)                                     # (the option exists: on the parent commit this raises)
    for n in (2, 3, 17, 37, 70):
        got = eng.forward(PROMPT[:n], 0)
        e = worst(got, rows[n - 1])
        print("%s prompt of %d tokens: max |d logit| = %.3g" % (mix, n, e))
        assert np.isfinite(got).all() and e <= TOL
    eng.forward(PROMPT[:20], 0)
    got = eng.forward(PROMPT[20:37], 20)
    e = worst(got, rows[36])
    print("%s prompt 20 + 17 tokens: max |d logit| = %.3g" % (mix, e))
    assert e <= TOL
    for i, t in enumerate(FED):                                           # the KV rows the prompt pass stored feed the decode steps
        got = eng.decode_fused(t, 37 + i, True)
        e = worst(got, dec[i])
        assert np.isfinite(got).all() and e <= TOL, (i, e)
    print("%s 8 decode steps behind the 37-token prompt: last max |d logit| = %.3g" % (mix, e))
    eng.close()


@pytest.mark.parametrize("mix", ["BF16", "F16"])
def test_score_meets_the_oracle_at_every_position(mix, files, oracle_rows):
    rows, _ = oracle_rows[mix]
    toks = PROMPT[:37]
    eng = load(files[mix][0], dense_mfma16=1)
    eng.set_option("score_rows", 16)                                      # the LM head 16 rows at a time (the F32-MFMA form) behind layers on the new kernel
    got = eng.score(toks)
    eng.set_option("score_rows", 64)                                      # ... and all 37 rows in one launch of the new kernel
    whole = eng.score(toks)
    l = rows[:37].astype(np.float64)
    lse = np.log(np.exp(l - l.max(axis=1, keepdims=True)).sum(axis=1)) + l.max(axis=1)
    want = np.array([l[i, toks[i + 1]] - lse[i] for i in range(36)] + [0.0])
    e = worst(got, want)
    print("%s score: max |d logprob| = %.3g" % (mix, e))
    assert got[-1] == 0.0 and e <= 2 * TOL
    assert whole[-1] == 0.0 and worst(whole, want) <= 2 * TOL
    eng.close()


def test_sequence_slots_batched_step_and_packed_prompt(files):
    path, twin = files["BF16"]
    prompts = [tokens(10 + k, n) for k, n in enumerate((5, 9, 40))]       # (40, and the packed pass's 49 rows: lengths the engine routes to the new kernel)
    nxt = [7, 100, 255]
    want_prompt, want_step = [], []
    for p, t in zip(prompts, nxt):
        m = O.OracleModel(twin, CTX)
        want_prompt.append(m.forward(p, 0))
        want_step.append(m.forward([t], len(p)))
    eng = load(path, sequences=3, dense_mfma16=1)
    for s, p in enumerate(prompts):
        assert worst(eng.seq_forward(s, p, 0), want_prompt[s]) <= TOL
    got, _ = eng.decode_batch([0, 1, 2], nxt, [len(p) for p in prompts])
    e = worst(got, np.stack(want_step))
    print("BF16 decode_batch of three slots: max |d logit| = %.3g" % e)
    assert np.isfinite(got).all() and e <= TOL
    got, _ = eng.forward_batch([2, 0], [prompts[2], prompts[1]], [0, 0])   # two segments in one pass over the weights
    e = worst(got, np.stack([want_prompt[2], want_prompt[1]]))
    print("BF16 forward_batch of two segments: max |d logit| = %.3g" % e)
    assert np.isfinite(got).all() and e <= TOL
    eng.close()


def test_q8_0_kv_cache_under_a_bf16_model():
    """heads of 128 (the 8-bit cache takes no other): the prompt pass on the 16-bit matrix cores against the F32-MFMA form on the same cache format, and the
    fused step behind each against its unfused step (tests/test_kv_q8_gpu.py's bar)"""
    spec = E.SynthSpec(256, 512, 2, 2, 1, 512, 4096, 1e-5, 500000.0, 256, 257, b"BF16", 20261017)
    toks = [256] + [int(t) for t in rng(30).integers(0, 256, 39)]
    per = []
    for on in (1, 0):
        e = E.Engine()
        e.set_option("synth_threads", 16)
        e.set_option("kv_cache", "q8_0")
        e.set_option("dense_mfma16", on)
        e.load_synthetic(spec, 256)
        prompt_logits = e.forward(toks, 0)
        step = e.decode_fused(5, 40, True)
        plain = e.forward([5], 40)
        assert np.isfinite(prompt_logits).all() and worst(step, plain) <= TOL
        per.append(np.stack([prompt_logits, step]))
        e.close()
    err = worst(per[0], per[1])
    print("BF16, kv_cache=q8_0, dense_mfma16 1 vs 0: %.3g" % err)
    assert err <= TOL


# ------------------------------------------------------------------------------------------------ the option
@pytest.mark.parametrize("mix", ["BF16", "F16"])
def test_option_off_and_on(mix, files, oracle_rows):
    """one engine, dense_mfma16 flipped 1 -> 0 -> 1 between runs: both settings meet the oracle and each other, back on gives the first run's bits, and the
    two settings differ in at least one bit -- the new path is taken"""
    rows, _ = oracle_rows[mix]
    eng = load(files[mix][0])
    runs = {}
    for on in (1, 0, 1):
        eng.set_option("dense_mfma16", on)
        got = np.stack([eng.forward(PROMPT[:17], 0), eng.forward(PROMPT[:37], 0), eng.forward(PROMPT, 0)])
        if on in runs:
            assert np.array_equal(got, runs[on])
        runs[on] = got
        e = worst(got, np.stack([rows[16], rows[36], rows[69]]))
        assert np.isfinite(got).all() and e <= TOL, (on, e)
    e = worst(runs[0], runs[1])
    print("%s dense_mfma16 0 vs 1: max |d logit| = %.3g" % (mix, e))
    assert e <= TOL
    assert not np.array_equal(runs[0], runs[1]), "the option changed nothing: both runs took the same launches"
    with pytest.raises(_lib.NtkError):
        eng.set_option("dense_mfma16", "2")
    eng.close()


# ------------------------------------------------------------------------------------------------ planes of two kinds in one model
def test_q8_0_model_with_bf16_ffn_down_and_f16_attn_output(tmp_path):
    """Q8_0 matrices read FP16 planes (their producers' fused split included), the F16 Wo reads FP16 planes too, the BF16 down projection planes of its own
    kind in the same two workspaces: the bookkeeping must never hand one kind to the other"""
    path, twin = str(tmp_path / "q8_mixed.gguf"), str(tmp_path / "q8_mixed_f32.gguf")
    G.make_synthetic_llama(path, G.TINY, "Q8_0", seed=SEED, overrides={"ffn_down": "BF16", "attn_output": "F16"})
    G.write_f32_twin(path, twin)
    want = {}
    for n in (17, 37, 70):                                                # (37: the producers' fused split -- up to 64 tokens -- in front of the 16-bit GEMM, which the engine takes from 32)
        want[n] = O.OracleModel(twin, CTX).forward(PROMPT[:n], 0)
    for options in ({}, {"prefill_fused_split": 0}, {"prefill_row_max": 0}):
        eng = load(path, **options)
        for n in (17, 37, 70):
            got = eng.forward(PROMPT[:n], 0)
            e = worst(got, want[n])
            print("Q8_0 + BF16 ffn_down + F16 attn_output %s, %d tokens: max |d logit| = %.3g" % (options, n, e))
            assert np.isfinite(got).all() and e <= TOL, (options, n, e)
        eng.close()


def test_a_quantised_model_does_not_see_the_option(tmp_path):
    path = str(tmp_path / "tiny_q8.gguf")
    G.make_synthetic_llama(path, G.TINY, "Q8_0", seed=SEED)
    eng = load(path)
    runs = []
    for on in (1, 0, 1):
        eng.set_option("dense_mfma16", on)
        runs.append(np.stack([eng.forward(PROMPT[:17], 0), eng.forward(PROMPT, 0)]))
    assert np.isfinite(runs[0]).all()
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)) and np.array_equal(runs[0].view(np.uint32), runs[2].view(np.uint32))
    eng.close()
