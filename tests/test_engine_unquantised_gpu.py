"""Unquantised models (BF16, F16) through the engine on the GPU: every entry point of a two-layer model against the oracle, the `dense_fused` option (the
fused 16-bit decode GEMV and the batched prompt GEMM against the 1:1 launcher sequence), the CLI and tensor parallelism.

The oracle has no BF16: it reads a twin file holding the SAME values as F32 (gguf.write_f32_twin; bfloat16 -> float is exact), so the reference has no
quantiser in it.  The model is gguf.TINY (hidden 256, 4 heads of 64, 2 KV heads, 2 layers, vocabulary 512); the 8-bit KV cache takes heads of 128 only, so
that case and the context shift run the tiny head-128 model of tests/test_kv_q8_gpu.py with BF16 weights.

Bars: 1e-3 on logits (the project's), 2e-3 on log-probabilities (tests/test_score_gpu.py: log-sum-exp is 1-Lipschitz in the max norm).

Run on the MI355X box:  python -m pytest tests/test_engine_unquantised_gpu.py -m gpu -x -q"""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from ntransformer_amd import _lib, ops
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-3
CTX = 128
SEED = 20261020


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[SEED, seed]))


def tokens(seed, n):
    return [G.TINY.bos] + [int(t) for t in rng(seed).integers(0, 256, n - 1)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{mix: (engine file, oracle file)}: the BF16 model with its F32 twin, the F16 model (the oracle reads F16 itself)"""
    d = tmp_path_factory.mktemp("unquantised")
    bf, twin, f16 = str(d / "tiny_bf16.gguf"), str(d / "tiny_bf16_as_f32.gguf"), str(d / "tiny_f16.gguf")
    G.make_synthetic_llama(bf, G.TINY, "BF16", seed=SEED)
    G.write_f32_twin(bf, twin)
    G.make_synthetic_llama(f16, G.TINY, "F16", seed=SEED)
    return {"BF16": (bf, twin), "F16": (f16, f16)}


PROMPT = tokens(1, 70)
FED = [int(t) for t in rng(2).integers(0, 256, 8)]


@pytest.fixture(scope="module")
def oracle_rows(files):
    """{mix: logits behind every prefix of PROMPT [70, vocab] and behind 8 teacher-forced tokens after the first 37 [8, vocab]}: computed once, read-only"""
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
    """prompts of 1, 3, 37 and 70 tokens (one row; fewer than a 16-token pass; three passes with a ragged one; five), and 37 tokens in two chunks"""
    rows, _ = oracle_rows[mix]
    eng = load(files[mix][0])
    for n in (1, 3, 37, 70):
        got = eng.forward(PROMPT[:n], 0)
        e = worst(got, rows[n - 1])
        print("%s prompt of %d tokens: max |d logit| = %.3g" % (mix, n, e))
        assert np.isfinite(got).all() and e <= TOL
    eng.forward(PROMPT[:20], 0)
    got = eng.forward(PROMPT[20:37], 20)
    e = worst(got, rows[36])
    print("%s prompt 20 + 17 tokens: max |d logit| = %.3g" % (mix, e))
    assert e <= TOL
    eng.close()


@pytest.mark.parametrize("mix", ["BF16", "F16"])
@pytest.mark.parametrize("how", ["graph", "eager", "unfused"])
def test_decode_steps_meet_the_oracle(mix, how, files, oracle_rows):
    _, dec = oracle_rows[mix]
    eng = load(files[mix][0], **({"fused": 0} if how == "unfused" else {}))
    eng.forward(PROMPT[:37], 0)
    for i, t in enumerate(FED):
        got = eng.forward([t], 37 + i) if how == "unfused" else eng.decode_fused(t, 37 + i, how == "graph")
        e = worst(got, dec[i])
        assert np.isfinite(got).all() and e <= TOL, (how, i, e)
    print("%s decode (%s): last step max |d logit| = %.3g" % (mix, how, e))
    eng.close()


def test_score_meets_the_oracle_at_every_position(files, oracle_rows):
    rows, _ = oracle_rows["BF16"]
    toks = PROMPT[:37]
    eng = load(files["BF16"][0])
    eng.set_option("score_rows", 16)
    got = eng.score(toks)
    l = rows[:37].astype(np.float64)
    lse = np.log(np.exp(l - l.max(axis=1, keepdims=True)).sum(axis=1)) + l.max(axis=1)
    want = np.array([l[i, toks[i + 1]] - lse[i] for i in range(36)] + [0.0])
    e = worst(got, want)
    print("BF16 score: max |d logprob| = %.3g" % e)
    assert got[-1] == 0.0 and e <= 2 * TOL
    eng.close()


def test_batched_step_and_packed_prompt_meet_the_oracle(files):
    path, twin = files["BF16"]
    prompts = [tokens(10 + k, n) for k, n in enumerate((5, 9, 21))]
    nxt = [7, 100, 255]
    want_prompt, want_step = [], []
    for p, t in zip(prompts, nxt):
        m = O.OracleModel(twin, CTX)
        want_prompt.append(m.forward(p, 0))
        want_step.append(m.forward([t], len(p)))
    eng = load(path, sequences=3)
    for s, p in enumerate(prompts):
        got = eng.seq_forward(s, p, 0)
        assert worst(got, want_prompt[s]) <= TOL
    got, _ = eng.decode_batch([0, 1, 2], nxt, [len(p) for p in prompts])
    e = worst(got, np.stack(want_step))
    print("BF16 decode_batch of three slots: max |d logit| = %.3g" % e)
    assert np.isfinite(got).all() and e <= TOL
    # the packed prompt pass: two segments (slot 2 and slot 0) in one pass over the weights
    got, _ = eng.forward_batch([2, 0], [prompts[2], prompts[1]], [0, 0])
    e = worst(got, np.stack([want_prompt[2], want_prompt[1]]))
    print("BF16 forward_batch of two segments: max |d logit| = %.3g" % e)
    assert np.isfinite(got).all() and e <= TOL
    # ... and the sampled batched step: greedy rows return the arg-max of the same logits
    params = [E.GenParams(1, 0.0, 40, 0.9, 1.0, 64, 42, 0)] * 3
    for s, p in enumerate(prompts):
        eng.seq_forward(s, p, 0)
    lg, toks = eng.decode_batch_sample([0, 1, 2], nxt, [len(p) for p in prompts], params, [[], [], []], [0.0, 0.0, 0.0])
    assert worst(lg, np.stack(want_step)) <= TOL
    for s in range(3):
        top2 = np.sort(want_step[s])[-2:]
        assert toks[s] == int(np.argmax(want_step[s])) or top2[1] - top2[0] <= 2 * TOL
    eng.close()


def test_bf16_ffn_down_in_a_q8_0_model(tmp_path):
    path, twin = str(tmp_path / "q8_bf16_down.gguf"), str(tmp_path / "q8_f32_down.gguf")
    G.make_synthetic_llama(path, G.TINY, "Q8_0", seed=SEED, overrides={"ffn_down": "BF16"})
    G.write_f32_twin(path, twin)
    m = O.OracleModel(twin, CTX)
    want = [m.forward(PROMPT[:37], 0)] + [m.forward([t], 37 + i) for i, t in enumerate(FED[:4])]
    eng = load(path)
    got = [eng.forward(PROMPT[:37], 0)] + [eng.decode_fused(t, 37 + i, True) for i, t in enumerate(FED[:4])]
    e = worst(np.stack(got), np.stack(want))
    print("Q8_0 with BF16 ffn_down: max |d logit| = %.3g" % e)
    assert e <= TOL
    eng.close()


# ------------------------------------------------------------------------------------------------ dense_fused = 0 against 1
@pytest.mark.parametrize("mix", ["BF16", "F16"])
def test_dense_fused_off_and_on_agree(mix, files, oracle_rows):
    """The A/B switch: 0 restores the 1:1 launcher sequence of both passes.  Same inputs, one engine, the option flipped between the runs (any time: the
    captured graphs are dropped); both settings also stand against the oracle."""
    rows, dec = oracle_rows[mix]
    eng = load(files[mix][0])
    runs = {}
    for on in (1, 0, 1):
        eng.set_option("dense_fused", on)
        lg = [eng.forward(PROMPT[:37], 0)]
        lg += [eng.decode_fused(t, 37 + i, True) for i, t in enumerate(FED[:4])]
        lg.append(eng.forward(PROMPT, 0))
        got = np.stack(lg)
        if on in runs:
            assert np.array_equal(got, runs[on])                         # back on: the same bits as before the flip
        runs[on] = got
        e = worst(got, np.concatenate([rows[36:37], dec[:4], rows[69:70]]))
        assert e <= TOL, (on, e)
    e = worst(runs[0], runs[1])
    print("%s dense_fused 0 vs 1: max |d logit| = %.3g" % (mix, e))
    assert e <= TOL
    assert not np.array_equal(runs[0], runs[1]), "the option changed nothing: both runs took the same launches"
    with pytest.raises(_lib.NtkError):
        eng.set_option("dense_fused", "2")
    eng.close()


# ------------------------------------------------------------------------------------------------ 8-bit KV cache, context shift (heads of 128)
def tiny128_bf16():
    return E.SynthSpec(256, 512, 2, 2, 1, 512, 4096, 1e-5, 500000.0, 256, 257, b"BF16", 20261017)


def synth_engine(ctx, **options):
    e = E.Engine()
    e.set_option("synth_threads", 16)
    for k, v in options.items():
        e.set_option(k, v)
    e.load_synthetic(tiny128_bf16(), ctx)
    return e


def test_q8_0_kv_cache_under_a_bf16_model():
    """tests/test_kv_q8_gpu.py's bar for the 8-bit cache: the fused step (eager = graph, bit for bit) within 1e-3 of the fused = 0 step on the same cache;
    and the same with dense_fused = 0"""
    toks = [256] + [int(t) for t in rng(30).integers(0, 256, 39)]
    fed = [int(t) for t in rng(31).integers(0, 256, 4)]
    per_setting = []
    for on in (1, 0):
        e = synth_engine(256, kv_cache="q8_0", dense_fused=on)
        e.forward(toks, 0)
        eager = [e.decode_fused(t, 40 + i, False) for i, t in enumerate(fed)]
        graph = [e.decode_fused(t, 40 + i, True) for i, t in enumerate(fed)]
        plain = [e.forward([t], 40 + i) for i, t in enumerate(fed)]
        for a, b in zip(eager, graph):
            assert np.isfinite(a).all() and np.array_equal(a, b)
        err = worst(np.stack(eager), np.stack(plain))
        print("BF16, kv_cache=q8_0, dense_fused=%d: |fused - unfused| = %.3g" % (on, err))
        assert err <= TOL
        per_setting.append(np.stack(eager))
        e.close()
    assert worst(per_setting[0], per_setting[1]) <= TOL


def test_context_shift_under_a_bf16_model():
    """one shift (keep 1, discard 8 of 40) and the step behind it: the fused 16-bit launches against the 1:1 sequence on the same operations"""
    toks = [256] + [int(t) for t in rng(32).integers(0, 256, 39)]
    got = []
    for on in (1, 0):
        e = synth_engine(64, dense_fused=on)
        e.forward(toks, 0)
        assert e.kv_shift(0, 1, 8, 40) == 32
        got.append(np.stack([e.decode_fused(5, 32, True), e.decode_fused(9, 33, True)]))
        e.close()
    err = worst(got[0], got[1])
    print("BF16 step behind a context shift, dense_fused 1 vs 0: %.3g" % err)
    assert np.isfinite(got[0]).all() and err <= TOL


# ------------------------------------------------------------------------------------------------ loader, CLI
def test_an_unknown_ggml_type_is_refused_at_load(files, tmp_path):
    blob = bytearray(open(files["BF16"][0], "rb").read())
    key = b"blk.0.attn_k.weight"
    at = blob.index(struct.pack("<Q", len(key)) + key) + 8 + len(key)
    tpos = at + 4 + 8 * struct.unpack_from("<I", blob, at)[0]
    assert struct.unpack_from("<I", blob, tpos)[0] == G.GGML_BF16
    struct.pack_into("<I", blob, tpos, 31)
    bad = str(tmp_path / "type31.gguf")
    open(bad, "wb").write(bytes(blob))
    eng = E.Engine()
    with pytest.raises(_lib.NtkError) as ei:
        eng.load(bad, CTX)
    assert "Unsupported tensor type" in str(ei.value)
    eng.close()


def test_cli_runs_a_synthetic_bf16_model():
    exe = os.path.join(os.path.dirname(E.__file__), "ntransformer")
    assert os.path.exists(exe), "CLI not built"
    r = subprocess.run([exe, "--synthetic", "tiny:BF16", "-p", "hi", "-n", "8", "-t", "0"], capture_output=True, timeout=300)
    txt = (r.stderr + r.stdout).decode("utf-8", "replace")
    assert r.returncode == 0, txt[-2000:]
    assert "BF16" in txt, txt[-2000:]                                     # the load banner names the type
    import re
    m = re.search(r"Decode:\s+(\d+) tokens", txt)
    assert m and int(m.group(1)) >= 1, txt[-2000:]


# ------------------------------------------------------------------------------------------------ tensor parallelism
RANK_SCRIPT = r"""
import sys, json, numpy as np
sys.path.insert(0, sys.argv[1])
from ntransformer_amd import engine as E, tp
rank, world, path, ctx, d = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]), sys.argv[6]
job = json.load(open(d + "/job.json"))
eng = E.Engine()
eng.tp_configure(rank, world)
eng.load(path, ctx)
tp.connect_over_files(eng, rank, world, d, timeout_s=100, run_id=job["run_id"])
lg = [eng.forward(job["prompt"], 0)]
pos = len(job["prompt"])
for t in job["fed"]:
    lg.append(eng.decode_fused(int(t), pos, True))
    pos += 1
np.save(d + "/logits_%d.npy" % rank, np.stack(lg))
json.dump({"tp_error": eng.tp_error()}, open(d + "/done_%d.json" % rank, "w"))
eng.close()
"""


def test_two_processes_of_a_bf16_model_meet_the_oracle(files, tmp_path):
    """tests/test_tp_gpu.py's deployment form (one process per rank, hipIpc handles through files) on the BF16 model: the sharding is expressed in row
    bytes, which BF16 has like F16.  21 prompt tokens, 4 steps from a captured graph."""
    path, twin = files["BF16"]
    prompt, fed = PROMPT[:21], FED[:4]
    m = O.OracleModel(twin, CTX)
    want = np.stack([m.forward(prompt, 0)] + [m.forward([t], 21 + i) for i, t in enumerate(fed)])
    d = str(tmp_path)
    json.dump({"prompt": prompt, "fed": fed, "run_id": "bf16"}, open(os.path.join(d, "job.json"), "w"))
    script = os.path.join(d, "rank.py")
    open(script, "w").write(RANK_SCRIPT)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, script, ROOT, str(k), "2", path, str(CTX), d], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
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
    lgs = [np.load(os.path.join(d, "logits_%d.npy" % k)) for k in range(2)]
    for k in range(2):
        assert json.load(open(os.path.join(d, "done_%d.json" % k)))["tp_error"] == 0
        e = worst(lgs[k], want)
        print("rank %d of 2, BF16: max |d logit| vs the oracle = %.3g" % (k, e))
        assert e <= TOL
    assert np.array_equal(lgs[0], lgs[1])
