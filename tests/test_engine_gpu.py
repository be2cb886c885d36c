"""GPU parity tests for the engine: logits of the HIP engine (1:1 launcher path, fused path, hipGraph replay)
against the golden logits produced by the reference's own host code + CPU kernels (tests/golden/*_logits.npz),
teacher-forced on the golden token stream.  North-star tolerance: |dlogit| <= 1e-3."""
import os

import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from oracle import oracle as O
from test_oracle_golden import CASES, golden_model

pytestmark = pytest.mark.gpu
TOL = 1e-3


def teacher_forced(eng, z, fused, graph):
    prompt, forced = [int(t) for t in z["prompt"]], [int(t) for t in z["forced"]]
    outs = [eng.forward(prompt, 0)]                       # prefill: batched MFMA GEMM unless batched_prefill=0
    pos = len(prompt)
    fed = forced + [int(t) for t in z["fed"][1 + len(forced):]]   # golden greedy continuation, fed verbatim
    for t in fed:
        outs.append(eng.decode_fused(t, pos, graph) if fused else eng.forward([t], pos))
        pos += 1
    return np.stack(outs)


@pytest.mark.parametrize("name,shape,mix", CASES)
@pytest.mark.parametrize("mode", ["reference", "launchers", "fused", "graph"])
def test_logits_match_reference_host_code(name, shape, mix, mode, tmp_path):
    """reference: the reference's exact launch sequence (per-token prompt loop, 15 launches per layer);
    launchers: batched prompt + 1:1 decode launchers; fused / graph: batched prompt + fused decode."""
    path, z = golden_model(name, shape, mix, tmp_path)
    eng = E.Engine()
    eng.load(path, int(z["ctx"]))
    eng.set_option("batched_prefill", mode != "reference")
    got = teacher_forced(eng, z, fused=mode in ("fused", "graph"), graph=mode == "graph")
    want = z["logits"]
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want).max()
    assert err <= TOL, (name, mode, err)
    # greedy choice agrees wherever the golden margin exceeds twice the tolerance
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * TOL
    assert np.array_equal(got.argmax(1)[clear], z["argmax"][clear])
    eng.close()


@pytest.mark.parametrize("mix", ["Q8_0", "Q4_K_M"])
def test_generate_tokens_reproduces_golden_greedy_stream(mix, tmp_path):
    """Engine::generate semantics (engine.cpp:40-145) end to end: greedy decoding from the golden prompt must give
    the golden argmax stream while the margins are clear; checks the device argmax, the position bookkeeping,
    the prefill->decode hand-over and the stats counters."""
    name = "tiny_" + mix.lower()
    path, z = golden_model(name, G.TINY, mix, tmp_path)
    m = O.OracleModel(path, int(z["ctx"]))
    prompt = [int(t) for t in z["prompt"]]
    want, lg = [], m.forward(prompt, 0)
    pos = len(prompt)
    for _ in range(12):
        want.append(m.argmax(lg))
        lg = m.forward([want[-1]], pos)
        pos += 1
    for opts in ({"fused": 1, "graph": 1}, {"fused": 1, "graph": 0}, {"fused": 0, "graph": 0}, {"fused": 1, "graph": 1, "device_sampling": 0}):
        eng = E.Engine()
        eng.load(path, int(z["ctx"]))
        for k, v in opts.items():
            eng.set_option(k, v)
        got = eng.generate_tokens(prompt, 12, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
        assert got == want, (opts, got, want)
        st = eng.stats()
        assert st.prompt_tokens == len(prompt) and st.gen_tokens == 11 and st.decode_ms > 0     # first token not counted
        eng.close()


def test_synthetic_loader_equals_file_loader(tmp_path):
    """nt_engine_load_synthetic builds in HBM exactly the model nt_synth_write_gguf writes to disk."""
    spec = E.synth_spec("tiny", "Q4_K_M")
    path = str(tmp_path / "cpp_tiny.gguf")
    E.synth_write_gguf(path, spec)
    a, b = E.Engine(), E.Engine()
    a.load(path, 128)
    b.load_synthetic(spec, 128)
    toks = [256, 3, 77, 400]
    assert np.array_equal(a.forward(toks, 0), b.forward(toks, 0))
    assert a.bytes_per_token(0) == b.bytes_per_token(0) == G.algorithmic_bytes_per_token(G.TINY, G.tensor_types(G.TINY, "Q4_K_M"), 0)
    # and the oracle agrees on that file
    m = O.OracleModel(path, 128)
    assert np.abs(a.forward(toks, 0) - m.forward(toks, 0)).max() <= TOL
    a.close(), b.close()


def test_c_api_generate_and_tokenizer(tmp_path):
    path = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    eng = E.Engine()
    eng._check(eng.L.nt_engine_load(eng.h, path.encode()), "nt_engine_load")
    assert (eng.vocab_size, eng.n_layers, eng.hidden_size) == (512, 2, 256)
    ids = eng.tokenize("hello world", True)
    assert ids[0] == 256 and len(ids) > 1
    text = eng.generate("hello", 8, temperature=0.0)
    assert isinstance(text, str)
    eng.close()


def test_8b_width_slice_matches_oracle():
    """Two layers at the real Llama-3.1-8B width (H=4096, I=14336, 32/8 heads, hd=128) with the full 128256-row LM
    head, Q8_0: full-width parity against the oracle without the full-depth CPU cost."""
    spec = E.synth_spec("8b", "Q8_0", layers=2)
    path = "/tmp/_8b_l2_q8_0_%d.gguf" % os.getpid()   # (per process: the directory is shared between users and runs)
    E.synth_write_gguf(path, spec)
    eng = E.Engine()
    eng.load(path, 256)
    m = O.OracleModel(path, 256)
    prompt = [128000, 11, 4095, 77777, 128255]
    got, want = eng.forward(prompt, 0), m.forward(prompt, 0)
    assert np.abs(got - want).max() <= TOL
    nxt = 31337
    for pos in range(len(prompt), len(prompt) + 3):
        want = m.forward([nxt], pos)
        got = eng.decode_fused(nxt, pos, graph=True)
        assert np.abs(got - want).max() <= TOL, pos
        nxt = int(np.argmax(want))
    eng.close()
    os.remove(path)


def test_reference_test_gemm_runs_on_the_hip_library():
    """The reference's own unmodified tests/test_gemm.cpp (+ src/core/tensor.cpp), linked through the two binding files
    of integration/ against libntransformer_hip.so (built by oracle/Makefile in the build container): its six kernel
    tests must pass on the MI355X kernels.  This is the drop-in boundary exercised end to end."""
    import subprocess
    exe = os.path.join(os.path.dirname(O.__file__), "_ref", "test_gemm_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/test_gemm_hip not built (needs /root/reference at build time)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SKIP" not in r.stderr and "FAIL" not in r.stderr, r.stderr[-2000:]
    assert r.stderr.count("PASS") == 6, r.stderr[-2000:]


@pytest.mark.parametrize("mix", ["Q8_0", "Q4_K_M", "MIXED"])
def test_batched_prefill_fills_the_same_kv_cache(mix, tmp_path):
    """A 37-token prompt (three 16-token chunks, the last ragged) through the batched MFMA projections and through the
    reference's per-token loops: the logits after the prompt and after eight more teacher-forced tokens (which read the
    whole KV cache the prompt wrote) agree within the north-star tolerance."""
    name = "tiny_" + mix.lower()
    path, z = golden_model(name, G.TINY, mix, tmp_path)
    r = np.random.Generator(np.random.Philox(key=[20260925, 4242]))
    prompt = [int(z["prompt"][0])] + [int(t) for t in r.integers(0, 256, 36)]
    cont = [int(t) for t in r.integers(0, 256, 8)]
    outs = {}
    for batched in (0, 1):
        eng = E.Engine()
        eng.load(path, int(z["ctx"]))
        eng.set_option("batched_prefill", batched)
        lg = [eng.forward(prompt, 0)]
        pos = len(prompt)
        for t in cont:
            lg.append(eng.decode_fused(t, pos, False))
            pos += 1
        outs[batched] = np.stack(lg)
        eng.close()
    assert np.isfinite(outs[1]).all()
    assert np.abs(outs[1] - outs[0]).max() <= TOL, np.abs(outs[1] - outs[0]).max()


@pytest.mark.parametrize("name,shape,mix", [("tiny_q8_0", "TINY", "Q8_0"), ("small_q8_0", "SMALL", "Q8_0"), ("small_q4_k_m", "SMALL", "Q4_K_M")])
def test_prompt_pass_with_folded_launches_gives_the_same_bits(name, shape, mix, tmp_path):
    """The prompt pass with its small launches folded ("prefill_row_max" = 1, the default: RMSNorm / SiLU leave the token maxima for the FP16 GEMM's
    pre-pass, the Wo / down / gate | up launches' K splits are summed by the RMSNorm / SiLU launch that consumes them, RoPE and the cache store are
    one launch) against the separate launches ("prefill_row_max" = 0, the path the golden-logit tests pin to the reference's host code): prompts of 40,
    200 and 700 tokens, the logits after the prompt and after six more decoded tokens (which read every cache row the prompt wrote) equal BIT FOR BIT."""
    path, z = golden_model(name, getattr(G, shape), mix, tmp_path)
    ctx = int(z["ctx"])
    r = np.random.Generator(np.random.Philox(key=[20260929, len(name)]))
    for n in (40, 200, 700, 16):   # (16: the weight-streaming form with its K slices, under the producers' split)
        if n + 8 > ctx: continue
        prompt = [int(z["prompt"][0])] + [int(t) for t in r.integers(0, 256, n - 1)]
        cont = [int(t) for t in r.integers(0, 256, 6)]
        outs = []
        for folded in (0, 1):
            eng = E.Engine()
            eng.load(path, ctx)
            eng.set_option("prefill_row_max", folded)
            lg = [eng.forward(prompt, 0)]
            pos = len(prompt)
            for t in cont:
                lg.append(eng.decode_fused(t, pos, False))
                pos += 1
            eng.close()
            outs.append(np.stack(lg))
        assert np.isfinite(outs[0]).all()
        assert np.array_equal(outs[0], outs[1]), (name, n, float(np.abs(outs[0] - outs[1]).max()))


def test_gate_and_up_of_two_formats_take_one_silu_form(tmp_path):
    """gate and up in different quantised formats go out as separate launches followed by a SiLU x up launch of its own, which
    must take exactly ONE form: split its output into the down projection's operand planes ("prefill_fused_split" = 1, up to 64
    tokens) or leave the token maxima (0).  The producers promise identical output: prompts of 8, 40 and 64 tokens and four
    teacher-forced decode steps, logits equal BIT FOR BIT between the two settings.  (TINY, Q8_0 with ffn_up in Q4_K: ffn_down
    stays in the FP16 GEMM's format set, which the MIXED file's F32 ffn_down is not.)"""
    path = str(tmp_path / "tiny_q8_0_up_q4_k.gguf")
    types = G.make_synthetic_llama(path, G.TINY, "Q8_0", seed=20260925, overrides={"ffn_up": "Q4_K"})
    assert types["blk.0.ffn_gate.weight"] == G.GGML_Q8_0 and types["blk.0.ffn_up.weight"] == G.GGML_Q4_K
    assert types["blk.0.ffn_down.weight"] == G.GGML_Q8_0
    r = np.random.Generator(np.random.Philox(key=[20261016, 1]))
    for n in (8, 40, 64):
        prompt = [G.TINY.bos] + [int(t) for t in r.integers(0, 256, n - 1)]
        cont = [int(t) for t in r.integers(0, 256, 4)]
        outs = []
        for split in (0, 1):
            eng = E.Engine()
            eng.load(path, G.TINY.ctx)
            eng.set_option("prefill_fused_split", split)
            lg = [eng.forward(prompt, 0)]
            pos = len(prompt)
            for t in cont:
                lg.append(eng.decode_fused(t, pos, False))
                pos += 1
            eng.close()
            outs.append(np.stack(lg))
        assert np.isfinite(outs[0]).all()
        assert np.array_equal(outs[0], outs[1]), (n, float(np.abs(outs[0] - outs[1]).max()))


def test_long_context_decode_uses_split_attention_and_matches_the_oracle(tmp_path):
    """Decode at positions 540..550 crosses the engine's attention regimes (single pass -> 8 KV splits at 544,
    Model::attention_regime), 668..678 and 1020..1030 run inside the split regime.  Every mode -- the reference's 1:1 launcher
    sequence, the fused launches, the fused launches replayed from a hipGraph -- is held to the ORACLE (reference
    attention.cu:108-202 over a cache of hundreds of rows, transformer.cpp:604-669), teacher-forced on one token stream, at the
    north-star tolerance; the modes' agreement with each other is a corollary, not the test."""
    path, z = golden_model("small_q8_0", G.SMALL, "Q8_0", tmp_path)   # head_dim 128, GQA 4, context 2048
    r = np.random.Generator(np.random.Philox(key=[20260925, 777]))
    observed = {}
    for start in (540, 668, 1020):
        prompt = [int(z["prompt"][0])] + [int(t) for t in r.integers(0, 256, start - 1)]
        cont = [int(t) for t in r.integers(0, 256, 10)]
        m = O.OracleModel(path, 2048)
        want = [m.forward(prompt, 0)]
        pos = len(prompt)
        for t in cont:
            want.append(m.forward([t], pos))
            pos += 1
        want = np.stack(want)
        outs = {}
        for mode in ("launchers", "fused", "graph"):
            eng = E.Engine()
            eng.load(path, 2048)
            lg = [eng.forward(prompt, 0)]
            pos = len(prompt)
            for t in cont:
                lg.append(eng.forward([t], pos) if mode == "launchers" else eng.decode_fused(t, pos, mode == "graph"))
                pos += 1
            outs[mode] = np.stack(lg)
            eng.close()
            err = np.abs(outs[mode] - want).max(axis=1)
            observed["%d/%s" % (start, mode)] = float(err.max())
            assert err.max() <= TOL, (start, mode, [float(e) for e in err])
        for mode in ("fused", "graph"):
            assert np.abs(outs[mode] - outs["launchers"]).max() <= TOL, (start, mode, np.abs(outs[mode] - outs["launchers"]).max())
    _log_observed({"test": "long_context_decode_vs_oracle", "model": "small Q8_0 (4 layers, hd 128, GQA 4)", "max_abs_err_vs_oracle": observed})


def test_decode_beyond_3072_positions_runs_the_matrix_core_attention_and_matches_the_oracle(tmp_path):
    """From 3072 positions the engine's split attention is the matrix-core form (one workgroup per (KV head, split), 32 splits:
    Model::attention_regime, attention_mfma.hip).  Decode across the border -- positions 3068..3077 -- and at 3900..3909 in the
    fused and the graph-replayed mode against the ORACLE (reference attention.cu:108-202 over a cache of thousands of rows), teacher
    forced, at the north-star tolerance; the cache rows the engine wrote on the way (K within a half ulp: device vs glibc sin / cos;
    V bit-exact) are checked through the oracle's own cache.  Model: the `small` shape (head_dim 128, GQA 4) with 2 layers and a
    4096-token context."""
    import dataclasses
    shape = dataclasses.replace(G.SMALL, name="small4k", layers=2, ctx=4096)
    path = str(tmp_path / "small4k_q8_0.gguf")
    G.make_synthetic_llama(path, shape, "Q8_0", seed=20260926)
    r = np.random.Generator(np.random.Philox(key=[20260926, 4096]))
    observed = {}
    for start in (3068, 3900):
        prompt = [256] + [int(t) for t in r.integers(0, 256, start - 1)]
        cont = [int(t) for t in r.integers(0, 256, 10)]
        m = O.OracleModel(path, 4096)
        want = [m.forward(prompt, 0)]
        pos = len(prompt)
        for t in cont:
            want.append(m.forward([t], pos))
            pos += 1
        want = np.stack(want)
        for mode in ("fused", "graph"):
            eng = E.Engine()
            eng.load(path, 4096)
            lg = [eng.forward(prompt, 0)]
            pos = len(prompt)
            for t in cont:
                lg.append(eng.decode_fused(t, pos, mode == "graph"))
                pos += 1
            eng.close()
            err = np.abs(np.stack(lg) - want).max(axis=1)
            observed["%d/%s" % (start, mode)] = float(err.max())
            assert err.max() <= TOL, (start, mode, [float(e) for e in err])
    _log_observed({"test": "decode_beyond_3072_positions_vs_oracle", "model": "small Q8_0, 2 layers, hd 128, GQA 4, context 4096",
                   "max_abs_err_vs_oracle": observed})


def test_decode_at_8k_and_33k_positions_matches_the_oracle(tmp_path):
    """Contexts beyond 4096 through the ENGINE (reference -c / --ctx-size, main.cpp:74-75): the `small` shape (head_dim 128, GQA 4) with 2 layers and a
    33 000-token context; the SAME seeded random cache rows are written into the engine (nt_engine_debug_kv_write) and into the oracle's cache
    for positions [0, start), then both decode four teacher-forced tokens from `start` = 8190 and 32766 (the matrix-core split attention, 32 splits:
    256 and 1024 rows per split and wave chunk walk) -- fused launches and hipGraph replay against the ORACLE (reference attention.cu:108-202 over tens of
    thousands of cache rows), at the north-star tolerance.  (The oracle's O(n^2) prompt pass at these lengths would take minutes; a prompt pass does
    not reach these positions any differently than 3900, which tests above cover end to end.)"""
    import dataclasses
    ctx = 33000
    shape = dataclasses.replace(G.SMALL, name="small33k", layers=2, ctx=ctx)
    path = str(tmp_path / "small33k_q8_0.gguf")
    G.make_synthetic_llama(path, shape, "Q8_0", seed=20260927)
    per = shape.kv_heads * (shape.hidden // shape.heads)
    observed = {}
    for start in (8190, 32766):
        r = np.random.Generator(np.random.Philox(key=[20260927, start]))
        rows_k = [(0.5 * r.standard_normal((start, per))).astype(np.float16).view(np.uint16) for _ in range(shape.layers)]
        rows_v = [(0.5 * r.standard_normal((start, per))).astype(np.float16).view(np.uint16) for _ in range(shape.layers)]
        cont = [int(t) for t in r.integers(0, 256, 4)]
        m = O.OracleModel(path, ctx)
        for i in range(shape.layers):
            m.k_cache[i][: start * per] = rows_k[i].reshape(-1)
            m.v_cache[i][: start * per] = rows_v[i].reshape(-1)
        want, pos = [], start
        for t in cont:
            want.append(m.forward([t], pos))
            pos += 1
        want = np.stack(want)
        for mode in ("fused", "graph"):
            eng = E.Engine()
            eng.load(path, ctx)
            for i in range(shape.layers):
                eng.kv_write(i, 0, rows_k[i], rows_v[i])
            lg, pos = [], start
            for t in cont:
                lg.append(eng.decode_fused(t, pos, mode == "graph"))
                pos += 1
            eng.close()
            err = np.abs(np.stack(lg) - want).max(axis=1)
            observed["%d/%s" % (start, mode)] = float(err.max())
            assert np.isfinite(np.stack(lg)).all() and err.max() <= TOL, (start, mode, [float(e) for e in err])
    _log_observed({"test": "decode_at_8k_and_33k_positions_vs_oracle", "model": "small Q8_0, 2 layers, hd 128, GQA 4, context 33000",
                   "max_abs_err_vs_oracle": observed})


def test_split_attention_without_the_combine_launch_gives_the_same_bits(tmp_path):
    """The engine's split-KV decode attention as one launch ("attention_merge" = 1: the last workgroup of a head merges the partial states; opt-in,
    it measured slower) against the two-launch form of rounds 3-5 ("attention_merge" = 0, the default) on the same seeded cache rows: both attention regimes (walk with 8
    splits at position 700, matrix cores with 32 splits at 3500), eager and hipGraph replay (the arrival counters return to zero inside every
    replay), 24 teacher-forced tokens each -- the logits must be equal BIT FOR BIT.  The two-launch form is the one pinned to the oracle above."""
    import dataclasses
    ctx = 4096
    shape = dataclasses.replace(G.SMALL, name="small4k", layers=2, ctx=ctx)
    path = str(tmp_path / "small4k_q8_0.gguf")
    G.make_synthetic_llama(path, shape, "Q8_0", seed=20260928)
    per = shape.kv_heads * (shape.hidden // shape.heads)
    for start in (700, 3500):
        r = np.random.Generator(np.random.Philox(key=[20260928, start]))
        rows_k = [(0.5 * r.standard_normal((start, per))).astype(np.float16).view(np.uint16) for _ in range(shape.layers)]
        rows_v = [(0.5 * r.standard_normal((start, per))).astype(np.float16).view(np.uint16) for _ in range(shape.layers)]
        cont = [int(t) for t in r.integers(0, 256, 24)]
        outs = {}
        for merge in (0, 1):
            for graph in (False, True):
                eng = E.Engine()
                eng.load(path, ctx)
                eng.set_option("attention_merge", merge)
                for i in range(shape.layers):
                    eng.kv_write(i, 0, rows_k[i], rows_v[i])
                lg, pos = [], start
                for t in cont:
                    lg.append(eng.decode_fused(t, pos, graph))
                    pos += 1
                toks = eng.decode_greedy_steps(cont[-1], pos, 16)
                eng.close()
                outs[(merge, graph)] = (np.stack(lg), toks)
        base = outs[(0, False)]
        assert np.isfinite(base[0]).all()
        for key, (lg, toks) in outs.items():
            assert np.array_equal(lg, base[0]), (start, key, float(np.abs(lg - base[0]).max()))
            assert toks == base[1], (start, key)


# ---------------------------------------------------------------------------------------------------
# Parity at the BASELINE configs' real width, shallow depth (SURVEY 8(d) "Parity procedure"; reference
# src/model/transformer.cpp:604-669).  Teacher-forced: the oracle runs free greedy decode, the HIP engine is fed the
# same tokens and every step's full logit vector is compared, max |d| <= 1e-3 -- attainable end to end while the model
# is shallow enough that the half roundings of K / V (attention.cu:338) have not yet turned 1e-7 differences between two
# correct F32 implementations into 1e-3 ones.  FULL depth (32 layers, 16 of the 70B shape) is tests/test_parity_depth.py,
# which separates the two with layer-wise teacher forcing and a float64 arbiter.  The observed errors are appended to
# gpurun_out/parity_observed.jsonl on the GPU box (copied to profiles/ by the round script).
# ---------------------------------------------------------------------------------------------------
def _log_observed(rec):
    import json
    root = os.environ.get("GRAFT_REPO_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "parity_observed.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


_THREADS = []


def _oracle_threads():
    if not _THREADS:
        os.environ.setdefault("OMP_WAIT_POLICY", "passive")
        _THREADS.append(O.pick_threads())
    return _THREADS[0]


def _scratch_dir():
    return "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else "/tmp"


def _parity_at_config(tag, preset, mix, layers, n_prompt, n_decode, ctx=256, patch=None, rel_bar=False):
    """patch(path): edits the written GGUF in place before anybody loads it; rel_bar: the 1e-3 scales with the logits' RMS (models whose
    activations were made larger on purpose)."""
    import time
    spec = E.synth_spec(preset, mix, layers=layers)
    path = os.path.join(_scratch_dir(), "_parity_%s_%d.gguf" % (tag, os.getpid()))   # (per process: the directory is shared between users and runs)
    E.synth_write_gguf(path, spec)
    if patch is not None: patch(path)
    try:
        threads = _oracle_threads()
        m = O.OracleModel(path, ctx)
        r = np.random.Generator(np.random.Philox(key=[20260925, 1234]))
        prompt = [spec.bos] + [int(t) for t in r.integers(0, spec.vocab, n_prompt - 1)]
        t0 = time.perf_counter()
        want, fed = [m.forward(prompt, 0)], []
        pos = len(prompt)
        for _ in range(n_decode):
            fed.append(m.argmax(want[-1]))
            want.append(m.forward([fed[-1]], pos))
            pos += 1
        t_oracle = time.perf_counter() - t0
        want = np.stack(want)
        assert np.isfinite(want).all()
        bar = TOL * (max(1.0, float(np.sqrt((want ** 2).mean()))) if rel_bar else 1.0)
        observed = {}
        # reference: the reference's exact launch sequence (per-token prompt loop, 15 launches per layer, --no-fuse);
        # launchers: batched MFMA prompt + 1:1 decode; fused / graph: batched prompt + fused decode (eager / hipGraph replay)
        for mode in ("reference", "launchers", "fused", "graph"):
            eng = E.Engine()
            eng.load(path, ctx)
            eng.set_option("batched_prefill", mode != "reference")
            got = [eng.forward(prompt, 0)]
            pos = len(prompt)
            for t in fed:
                got.append(eng.decode_fused(t, pos, mode == "graph") if mode in ("fused", "graph") else eng.forward([t], pos))
                pos += 1
            eng.close()
            got = np.stack(got)
            assert np.isfinite(got).all(), (tag, mode)
            err = np.abs(got - want).max(axis=1)
            observed[mode] = [float(e) for e in err]
            top2 = np.sort(want, axis=1)[:, -2:]
            clear = (top2[:, 1] - top2[:, 0]) > 2 * TOL
            agree = bool(np.array_equal(got.argmax(1)[clear], want.argmax(1)[clear]))
            assert err.max() <= bar, (tag, mode, observed[mode], bar)
            assert agree, (tag, mode)
        _log_observed({"test": tag, "model": preset, "mix": mix, "layers": layers, "prompt_tokens": n_prompt,
                       "decode_steps": n_decode, "tolerance": TOL, "bar_used": bar, "oracle_threads": threads,
                       "oracle_seconds": round(t_oracle, 2), "logit_rms": float(np.sqrt((want ** 2).mean())),
                       "max_abs_err_per_step": observed,
                       "max_abs_err": {k: max(v) for k, v in observed.items()}})
    finally:
        try:
            os.remove(path)
        except OSError:
            pass


def test_8b_q4_k_m_mix_logits_match_oracle():
    """BASELINE config 3: the llama.cpp Q4_K_M tensor mix at 8B width, 8 layers -- layers 0, 3, 6, 7 carry the Q6_K attn_v /
    ffn_down (`use_more_bits`), the others Q4_K, so both the single-dtype and the split Q|K + V launches occur."""
    _parity_at_config("8b_q4_k_m_8_layers", "8b", "Q4_K_M", 8, 20, 4)


@pytest.mark.parametrize("mix", ["Q4_K_M", "Q6_K"])
def test_70b_width_slice_logits_match_oracle(mix):
    """BASELINE configs 4 / 5 at their real width (H=8192, I=28672, 64 heads, 8 KV heads), 2 layers: the 28672-wide down
    projection (7 column slices, two-pass activation image), Q5_K attn_v (layer 0 of the Q4_K_M mix) and Q6_K (layer 1)."""
    _parity_at_config("70b_width_2_layers_" + mix.lower(), "70b", mix, 2, 18, 3)


def test_cli_binary_generates_and_reports_decode_rate():
    """The `ntransformer` CLI (reference src/main.cpp:52-103 flag set) end to end on the GPU: synthetic tiny model, greedy,
    8 tokens; the reference's statistics block (engine.cpp:595-600) must appear with a decode rate."""
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(E.__file__), "ntransformer")
    assert os.path.exists(exe), "CLI not built"
    r = subprocess.run([exe, "--synthetic", "tiny:Q4_K_M", "-p", "hi", "-n", "8", "-t", "0", "--repeat-penalty", "1.0"],
                       capture_output=True, timeout=300)
    txt = (r.stderr + r.stdout).decode("utf-8", "replace")
    assert r.returncode == 0, txt[-2000:]
    m = re.search(r"Decode:\s+(\d+) tokens.*?([0-9.]+) tok/s", txt)
    assert m, txt[-2000:]
    assert int(m.group(1)) >= 1 and float(m.group(2)) > 0
    # flags whose reference semantics change the output are refused, not silently ignored
    r = subprocess.run([exe, "--synthetic", "tiny:Q4_K_M", "-p", "hi", "-n", "2", "--early-exit", "0.9"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "not supported" in r.stderr


@pytest.mark.parametrize("name,shape,mix", CASES)
def test_reference_transformer_runs_on_the_hip_library(name, shape, mix, tmp_path):
    """The reference's OWN host code -- nt::Transformer / Attention / FFN / RMSNorm / GGUFLoader, compiled unmodified from
    /root/reference/src in the build container (oracle/Makefile: _ref/ref_logits_hip) -- linked through integration/ against
    libntransformer_hip.so and run on the MI355X: its logits must equal the committed goldens, which the SAME host code
    produced over the CPU restatement of the CUDA kernels.  Reference launch sequence: src/model/transformer.cpp:604-669."""
    exe = os.path.join(os.path.dirname(O.__file__), "_ref", "ref_logits_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_logits_hip not built (needs /root/reference at build time)")
    path, z = golden_model(name, shape, mix, tmp_path)
    prompt = [int(t) for t in z["prompt"]]
    fed_all = [int(t) for t in z["fed"][1:]]
    fed, am, got = O.run_ref_logits(path, prompt, fed_all, 0, int(z["ctx"]), out_path=str(tmp_path / "hip_logits.bin"),
                                    exe_name="ref_logits_hip")
    want = z["logits"]
    assert got.shape == want.shape and np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    _log_observed({"test": "reference_transformer_on_hip_library", "model": name, "max_abs_err": err, "tolerance": TOL})
    assert err <= TOL, (name, err)


@pytest.mark.parametrize("name,shape,mix", [c for c in CASES if c[2] in ("Q4_K_M", "Q6_K", "MIXED")])
def test_reference_transformer_on_the_matrix_core_gemv(name, shape, mix, tmp_path):
    """Round 5: the matrix-core K-quant GEMV reached THROUGH THE REFERENCE'S OWN BINDING.  The reference's unmodified nt::Transformer
    (ref_logits_hip) with NT_HIP_AUTO_REPACK=1: integration/nt_cuda_launchers.cpp packs every K-quant matrix at its first launch_gemv
    (ntk_rp_pack, owned by the binding -- what hip_register_resident_weight does from Attention::set_weights / FFN::init, attention.cpp:80-95,
    ffn.cpp:7-29) and serves that pointer from ntk_gemv_rp afterwards; logits against the committed goldens (the same host code over the CPU
    restatement), and the binding's own count of which kernel served the launches."""
    import subprocess
    exe = os.path.join(os.path.dirname(O.__file__), "_ref", "ref_logits_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_logits_hip not built (needs /root/reference at build time)")
    path, z = golden_model(name, shape, mix, tmp_path)
    prompt = [int(t) for t in z["prompt"]]
    fed_all = [int(t) for t in z["fed"][1:]]
    out_path = str(tmp_path / "hip_rp_logits.bin")
    cmd = [exe, path, str(int(z["ctx"])), out_path, str(len(prompt)), "0"] + [str(t) for t in prompt + fed_all]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, NT_HIP_AUTO_REPACK="1", NT_HIP_REPACK_STATS="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    import re
    m = re.search(r"nt_hip_repack: (\d+) tensors repacked, launch_gemv: (\d+) on ntk_gemv_rp \(matrix cores\), (\d+) on ntk_gemv", r.stderr)
    assert m, r.stderr[-2000:]
    n_packed, n_rp, n_raw = (int(g) for g in m.groups())
    assert n_packed > 0 and n_rp > 0
    if mix in ("Q4_K_M", "Q6_K"):
        assert n_rp >= 7 * shape.layers * len(z["logits"]) // 2   # the projections: K-quant in these mixes (in_features % 256 == 0 at this shape)
    raw = np.fromfile(out_path, dtype=np.uint8)
    n_steps, V = np.frombuffer(raw[:8].tobytes(), "<i4")
    got = raw[8:].reshape(n_steps, 8 + 4 * V)[:, 8:].copy().view("<f4").reshape(n_steps, V)
    want = z["logits"]
    assert got.shape == want.shape and np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    _log_observed({"test": "reference_transformer_on_matrix_core_gemv", "model": name, "max_abs_err": err, "tolerance": TOL,
                   "tensors_repacked": n_packed, "launches_rp": n_rp, "launches_raw": n_raw})
    assert err <= TOL, (name, err)


@pytest.mark.parametrize("name,shape,mix", [c for c in CASES if c[2] in ("Q4_K_M", "Q6_K", "MIXED")])
def test_one_resident_copy_gives_the_same_bits_as_two(name, shape, mix, tmp_path):
    """`repack` = 2 (the GGUF bytes of every repacked K-quant matrix freed after the load-time repack; prompt GEMM, the reference's 1:1 launch sequence
    and the fallbacks read the tensor from a scratch that ntk_rp_unpack fills in front of them) against `repack` = 1 (both copies resident): the
    unpack is the byte-exact inverse of the pack, so EVERY logit of a batched prompt, of the per-token reference sequence and of fused / graph decode
    steps is bit-identical, and the weights occupy about half.  Switching 2 -> 1 -> 2 on a loaded model goes through the same bytes."""
    path, z = golden_model(name, shape, mix, tmp_path)
    prompt = [int(t) for t in z["prompt"]]
    fed = [int(t) for t in z["fed"][1:]][:5]
    outs, resident = {}, {}
    for level in (1, 2):
        for batched in (1, 0):
            eng = E.Engine()
            eng.set_option("repack", level)
            eng.load(path, int(z["ctx"]))
            eng.set_option("batched_prefill", batched)
            lg = [eng.forward(prompt, 0)]
            pos = len(prompt)
            for i, t in enumerate(fed):
                lg.append(eng.decode_fused(t, pos, i % 2 == 1) if batched else eng.forward([t], pos))
                pos += 1
            outs[(level, batched)] = np.stack(lg)
            resident[level] = eng.resident_weight_bytes()
            if level == 2 and batched:
                eng.set_option("repack", 1)               # the GGUF bytes come back from the repack ...
                again = eng.forward(prompt, 0)
                eng.set_option("repack", 2)               # ... and go again
                again2 = eng.forward(prompt, 0)
                assert np.array_equal(again, lg[0]) and np.array_equal(again2, lg[0])
            eng.close()
    for batched in (1, 0):
        assert np.isfinite(outs[(2, batched)]).all()
        assert np.array_equal(outs[(1, batched)], outs[(2, batched)]), (name, batched, np.abs(outs[(1, batched)] - outs[(2, batched)]).max())
    if mix != "MIXED":
        assert resident[2] < 0.7 * resident[1], resident


@pytest.mark.parametrize("budget_frac", [0.0, 0.4, 0.999])
def test_a_repack_that_does_not_fit_leaves_the_rest_on_the_raw_path(budget_frac, tmp_path):
    """The load-time repack (engine-owned second copy of the K-quant matrices, reference load path transformer.cpp:286-328 has no counterpart) when the
    device runs out of memory part of the way: nt_hip_malloc fails for the remaining tensors (forced here through ntk_debug_malloc_budget: nothing,
    40 % and all but the last tensor's worth of the repack fit), the load / set_option must NOT fail, the tensors without a repacked form decode on
    the raw-GGUF path, and neither the failed hipMalloc's sticky error nor anything else may surface in the launches that follow: a batched prompt,
    fused and graph decode steps equal the golden logits of the fully repacked engine at the GEMV tolerance, every status NTK_OK.  Then `repack` = 2
    with no room for the unpack scratch: the GGUF bytes stay resident (warning), same logits."""
    from ntransformer_amd import _lib
    name, shape, mix = "small_q4_k_m", G.SMALL, "Q4_K_M"
    path, z = golden_model(name, shape, mix, tmp_path)
    prompt = [int(t) for t in z["prompt"]]
    fed = [int(t) for t in z["fed"][1:]][:4]
    L = _lib.lib()
    L.ntk_debug_malloc_budget.argtypes = [C.c_longlong]
    L.ntk_debug_malloc_budget.restype = None

    def run(eng):
        lg = [eng.forward(prompt, 0)]
        pos = len(prompt)
        for i, t in enumerate(fed):
            lg.append(eng.decode_fused(t, pos, i % 2 == 1))
            pos += 1
        return np.stack(lg)
    ref = E.Engine()
    ref.set_option("repack", 1)
    ref.load(path, int(z["ctx"]))
    want = run(ref)
    rp_total = ref.repacked_bytes()
    ref.close()
    assert rp_total > 0
    eng = E.Engine()
    eng.set_option("repack", 0)
    eng.load(path, int(z["ctx"]))
    try:
        L.ntk_debug_malloc_budget(int(rp_total * budget_frac))
        eng.set_option("repack", 1)                 # runs the repack now: part of it fits
        got = run(eng)
        assert eng.repacked_bytes() <= rp_total * budget_frac + 1 and (budget_frac == 0.0 or eng.repacked_bytes() > 0)
        L.ntk_debug_malloc_budget(0)
        eng.set_option("repack", 2)                 # no room for the unpack scratch: both copies stay
        got2 = run(eng)
    finally:
        L.ntk_debug_malloc_budget(-1)
    eng.close()
    assert np.isfinite(got).all() and np.isfinite(got2).all()
    tol = 1e-3
    assert np.abs(got - want).max() <= tol and np.abs(got2 - want).max() <= tol, (np.abs(got - want).max(), np.abs(got2 - want).max())
    assert np.array_equal(got, got2)


@pytest.mark.parametrize("name,shape,mix", [c for c in CASES if c[0] in ("small_q8_0", "small_q4_k_m")])
def test_two_sequences_share_one_copy_of_the_weights(name, shape, mix, tmp_path):
    """the path shards across REQUESTS -- independent sequences share nothing but the read-only weights.  nt_engine_load_shared gives a second
    engine the first one's tensors (raw GGUF bytes and the decode repack: the same device pointers), its own KV caches, buffers and HIP stream.  Two host
    threads then decode two different prompts at once; each sequence must produce EXACTLY what it produces alone on a private engine -- logits of the prompt
    pass bit for bit, the greedy token stream, and the logits after it -- i.e. the same parity as a single stream (which the golden tests pin to the
    reference's host code).  The second engine adds no weight bytes."""
    import threading
    path, z = golden_model(name, shape, mix, tmp_path)
    ctx = int(z["ctx"])
    prompts = [[int(t) for t in z["prompt"]], [int(t) for t in z["prompt"]][::-1][:-1] + [7, 3]]
    n = 12
    solo = []
    for pr in prompts:
        eng = E.Engine()
        eng.load(path, ctx)
        lg = eng.forward(pr, 0)
        toks = eng.decode_greedy_steps(int(np.argmax(lg)), len(pr), n)
        solo.append((lg, toks, eng.decode_fused(toks[-1], len(pr) + n, True)))
        eng.close()
    a = E.Engine()
    a.load(path, ctx)
    b = E.Engine()
    b.load_shared(a, ctx)
    assert b.repacked_bytes() == 0 and a.weight_bytes() == b.weight_bytes()
    engs, got = (a, b), [None, None]
    for rep in range(3):                       # three rounds: the second and third replay captured graphs on both streams at once
        gate = threading.Barrier(2)

        def worker(i):
            gate.wait()
            lg = engs[i].forward(prompts[i], 0)
            toks = engs[i].decode_greedy_steps(int(np.argmax(lg)), len(prompts[i]), n)
            got[i] = (lg, toks, engs[i].decode_fused(toks[-1], len(prompts[i]) + n, True))
        th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
        for t in th: t.start()
        for t in th: t.join()
        for i in range(2):
            assert got[i] is not None
            assert np.array_equal(got[i][0], solo[i][0]), (rep, i, "prompt logits")
            assert got[i][1] == solo[i][1], (rep, i, got[i][1], solo[i][1])
            assert np.array_equal(got[i][2], solo[i][2]), (rep, i, "logits behind the stream")
    with pytest.raises(Exception):
        b.set_option("repack", 2)              # a sharing sequence cannot re-shape tensors it does not own
    b.close()
    a.close()


def test_decoding_again_after_a_pipelined_run_rebases_the_device_position(tmp_path):
    """The greedy loops keep one step queued ahead of the token the host waits for (Engine::run, decode_greedy_steps: reference engine.cpp:100-136 is
    the loop they replace) and stop the decode clock before a discarded run-ahead step drains -- so after a run the DEVICE position, token and pinned
    ring may be ahead of what the host saw.  Every entry point that decodes afterwards must re-base them (Model::set_device_pos): a second run from an
    EARLIER position, a teacher-forced step, and a generate on the same engine must give what a fresh engine gives."""
    path, z = golden_model("small_q8_0", G.SMALL, "Q8_0", tmp_path)
    prompt = [int(t) for t in z["prompt"]]
    P = len(prompt)

    def fresh():
        e = E.Engine()
        e.load(path, 256)
        e.forward(prompt, 0)
        return e
    a = fresh()
    first = a.decode_greedy_steps(7, P, 9)              # pipelined: the device has run ahead of the host inside this call
    again = a.decode_greedy_steps(7, P, 5)              # back to position P on the SAME engine
    lg_a = a.decode_fused(first[2], P + 3, True)        # a teacher-forced step in the middle of what the cache now holds
    gen_a = a.generate_tokens(prompt, 6, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
    a.close()
    b = fresh()
    assert b.decode_greedy_steps(7, P, 9) == first
    b.close()
    b = fresh()
    assert b.decode_greedy_steps(7, P, 5) == again == first[:5]
    lg_b = b.decode_fused(first[2], P + 3, True)
    b.close()
    assert np.array_equal(lg_a, lg_b)
    b = E.Engine()
    b.load(path, 256)
    assert b.generate_tokens(prompt, 6, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False) == gen_a
    b.close()


def test_reference_cli_runs_on_the_hip_library():
    """The reference's unmodified src/main.cpp + Engine (engine.cpp:40-145) over the HIP library: greedy generation must
    complete and print the reference's own statistics block (engine.cpp:595-600)."""
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(O.__file__), "_ref", "ntransformer_ref_hip")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ntransformer_ref_hip not built (needs /root/reference at build time)")
    r = subprocess.run([exe, "-m", os.path.join(GOLDEN, "tiny_q8_0.gguf"), "-p", "hello", "-n", "8", "-t", "0",
                        "--repeat-penalty", "1.0", "-c", "128"], capture_output=True, timeout=300)
    txt = (r.stderr + r.stdout).decode("utf-8", "replace")   # a random-weight model prints arbitrary bytes
    assert r.returncode == 0, txt[-2000:]
    assert re.search(r"Decode:\s+\d+ tokens", txt), txt[-2000:]


@pytest.mark.parametrize("cfg", [dict(temperature=0.7, top_k=40, top_p=0.9, repeat_penalty=1.1), dict(temperature=0.0, repeat_penalty=1.3),
                                 dict(temperature=1.5, top_k=5, top_p=1.0, repeat_penalty=1.0)])
def test_device_sampling_gives_the_host_samplers_token_stream(cfg, tmp_path):
    """Engine::generate with the reference's DEFAULT CLI settings (-t 0.7, top-k 40, top-p 0.9, repeat-penalty 1.1;
    reference src/main.cpp) samples on the device (one pinned int per token instead of a 513 KB logits download and a
    host partial_sort); the token stream must equal the host sampler's (device_sampling = 0), same seed."""
    path, z = golden_model("small_q8_0", G.SMALL, "Q8_0", tmp_path)
    prompt = [int(t) for t in z["prompt"]]
    outs = []
    for dev in (1, 0):
        eng = E.Engine()
        eng.load(path, 512)
        eng.set_option("device_sampling", dev)
        outs.append(eng.generate_tokens(prompt, 40, seed=7, repeat_window=64, stop_at_eos=False, **cfg))
        eng.close()
    assert outs[0] == outs[1], outs
    assert len(set(outs[0])) > 3


@pytest.mark.parametrize("switch", ["NTK_GEMM_CW=2", "NTK_GEMM_CW=1", "NTK_GEMM_NO_PF=1", "NTK_GEMM_MAP=0", "NTK_GEMM_WGS=4096"])
def test_prompt_gemm_forms_behind_the_tuning_switches_keep_parity(switch):
    """The prompt GEMM (csrc/gemm_f16.hip) picks among forms by launch size: one or two 64-token chunks per workgroup, the plane
    prefetch, the (row tile, chunk) order per XCD, the K split.  The switches that force each form exist in the TUNING build of the
    library only (make tune: libntransformer_hip_tune.so reads them once per process; the shipping library has none); each must give the
    same parity: every FP16-GEMM kernel test and the engine's prompt tests, in a subprocess per switch on that library."""
    import subprocess
    import sys
    tune = os.path.join(os.path.dirname(E.__file__), "libntransformer_hip_tune.so")
    if not os.path.exists(tune):
        pytest.skip("libntransformer_hip_tune.so not built (make -C ntransformer_amd/csrc tune)")
    k, v = switch.split("=")
    env = dict(os.environ, NTK_LIB_PATH=tune, **{k: v})
    here = os.path.dirname(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_hip_kernels.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "gemm_quant_f16"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_engine_gpu.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "batched_prefill_fills or logits_match_reference_host_code"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])


def test_retired_options_are_accepted_and_change_nothing():
    """"persistent" and "fuse_attention" selected structures that lost to the fused launches and were removed (profiles/NEGATIVE_RESULTS.md).
    The options stay accepted; set after the load -- where "persistent" used to switch the repack level -- they leave the decode path, the resident
    bytes, the token stream and every logit bit as they are."""
    def run(options):
        eng = E.Engine()
        eng.load_synthetic(E.synth_spec("tiny", "Q8_0"), 256)
        for k, v in options:
            eng.set_option(k, v)
        prompt = [1, 17, 5, 99, 42]
        logits = [eng.forward(prompt, 0)]
        toks, pos = [], len(prompt)
        for _ in range(8):
            toks.append(int(np.argmax(logits[-1])))
            logits.append(eng.decode_fused(toks[-1], pos, graph=True))
            pos += 1
        out = (toks, np.stack(logits), eng.decode_path(), eng.resident_weight_bytes(), eng.repacked_bytes(), eng.kv_cache_bytes())
        eng.close()
        return out
    a = run([])
    b = run([("persistent", 1), ("persistent", 2), ("fuse_attention", 1)])
    assert a[0] == b[0]
    assert np.isfinite(a[1]).all() and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert a[2] == b[2] and a[2].startswith("fused (5 launches/layer")
    assert a[3:] == b[3:] and a[3] > 0
