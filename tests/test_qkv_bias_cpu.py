"""Qwen2 files on the CPU: the Python writer's qwen2 GGUF through both readers, the loader's refusals (they happen ahead of the device, so they are
tested here without a GPU), the seeded C++ generator's Qwen2 flavour against the engine's own reader -- and THE GUARD of tests/test_engine_qwen2_gpu.py:

test_the_biases_move_the_logits_by_ten_bars_on_every_test_model computes, with the oracle alone, the distance between the bias-aware oracle's logits
(tests/qkv_bias_ref.py) and the plain oracle's on every test model at prompt lengths 3, 4, 37 and 70, and asserts it is at least 10 x the 1e-3 logit bar.
An engine without the feature loads these files without complaint and matches the plain oracle, so it is at least 9 bars away from the reference of every
engine test.  BIAS_SCALE = 0.5 and the seed were chosen here; measured distances (max |dlogit|) over the four lengths: qt64 3.47 .. 4.17, qt128 1.04 .. 3.83, q7 3.83 .. 4.22 -- a thousand bars and more."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from qkv_bias_ref import BIAS_SCALE, GUARD_LENGTHS, MODELS, SEED, TOL, dist, model_file, oracle_ref


def bias_names(layers):
    return ["blk.%d.attn_%s.bias" % (i, m) for i in range(layers) for m in "qkv"]


def test_the_writers_qwen2_file_through_both_readers(tmp_path_factory):
    path = model_file("qt64", tmp_path_factory)
    shape, mix = MODELS["qt64"]
    f = G.read_gguf(path)
    assert f.meta["general.architecture"] in ("qwen2", b"qwen2")
    for key in ("vocab_size", "embedding_length", "feed_forward_length", "block_count", "attention.head_count", "attention.head_count_kv", "context_length",
                "attention.layer_norm_rms_epsilon", "rope.freq_base"):
        assert "qwen2." + key in f.meta and "llama." + key not in f.meta, key
    assert f.meta["qwen2.rope.freq_base"] == 1e6 and abs(f.meta["qwen2.attention.layer_norm_rms_epsilon"] - 1e-6) < 1e-12
    d = E.gguf_describe(path)
    assert d["architecture"] == "qwen2" and d["n_heads"] == 4 and d["n_kv_heads"] == 2 and d["head_dim"] == 64 and d["rope_theta"] == 1e6
    assert d["hidden_size"] == 256 and d["n_layers"] == 2 and d["max_seq_len"] == 1024
    assert d["qkv_bias_tensors"] == 3 * shape.layers
    table = {t["name"]: t for t in d["tensors"]}
    assert len(table) == len(f.tensors) == 3 + 12 * shape.layers
    raw = open(path, "rb").read()
    for name in bias_names(shape.layers):
        want_n = 256 if "attn_q" in name else 128
        ti = f.tensors[name]
        assert tuple(ti.dims) == (want_n,) and ti.ggml_type == G.GGML_F32
        assert table[name]["dims"] == [want_n] and table[name]["type"] == "F32" and table[name]["nbytes"] == 4 * want_n
        a = d["data_offset"] + table[name]["offset"]                    # the C++ reader's offsets lead to the Python reader's bytes
        assert raw[a:a + 4 * want_n] == f.f32(name).tobytes()
        # ... which are the writer's: seeded by name, normal values times the scale
        h = 1469598103934665603
        for c in name.encode():
            h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        want = (BIAS_SCALE * np.random.Generator(np.random.Philox(key=[SEED, h])).standard_normal(want_n)).astype("<f4")
        assert np.array_equal(f.f32(name), want)
    # a dict writes only the named biases; the llama architecture takes them too
    only_k = model_file("qt64", tmp_path_factory, arch="llama", qkv_bias={"k": BIAS_SCALE})
    dk = E.gguf_describe(only_k)
    assert dk["architecture"] == "llama" and dk["qkv_bias_tensors"] == shape.layers
    assert sorted(t["name"] for t in dk["tensors"] if t["name"].endswith(".bias")) == ["blk.0.attn_k.bias", "blk.1.attn_k.bias"]
    # without biases the writer's file is what it was before the writer learnt them
    assert E.gguf_describe(model_file("qt64", tmp_path_factory, arch="llama", qkv_bias=None))["qkv_bias_tensors"] == 0


def test_no_golden_file_carries_a_bias():
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.gguf")))
    assert len(files) >= 4
    for path in files:
        assert E.gguf_describe(path)["qkv_bias_tensors"] == 0, path


def spec(name, dims, ggml_type, values):
    return G.TensorSpec(name, dims, ggml_type, np.asarray(values).astype("<f2" if ggml_type == G.GGML_F16 else "<f4").tobytes())


REFUSALS = {
    # what: (arguments of make_synthetic_llama, the tensor the message must name, status)
    "f16_bias": (dict(qkv_bias={"q": 0.5, "v": 0.5}, extra_tensors=[spec("blk.1.attn_k.bias", (128,), G.GGML_F16, np.ones(128))]), "blk.1.attn_k.bias", -1),
    "short_bias": (dict(qkv_bias={"k": 0.5, "v": 0.5}, extra_tensors=[spec("blk.0.attn_q.bias", (255,), G.GGML_F32, np.ones(255))]), "blk.0.attn_q.bias", -2),
    "short_v_bias": (dict(qkv_bias={"q": 0.5, "k": 0.5}, extra_tensors=[spec("blk.1.attn_v.bias", (127,), G.GGML_F32, np.ones(127))]), "blk.1.attn_v.bias", -2),
    "q_norm": (dict(extra_tensors=[spec("blk.1.attn_q_norm.weight", (64,), G.GGML_F32, np.ones(64))]), "blk.1.attn_q_norm.weight", -9),
    "k_norm": (dict(extra_tensors=[spec("blk.0.attn_k_norm.weight", (64,), G.GGML_F32, np.ones(64))]), "blk.0.attn_k_norm.weight", -9),
    "ffn_down_bias": (dict(extra_tensors=[spec("blk.0.ffn_down.bias", (256,), G.GGML_F32, np.zeros(256))]), "blk.0.ffn_down.bias", -9),
    "beyond_the_layers": (dict(extra_tensors=[spec("blk.5.ffn_up.bias", (512,), G.GGML_F32, np.zeros(512))]), "blk.5.ffn_up.bias", -9),          # (a 2-layer file)
    "output_bias": (dict(qkv_bias=None, arch="llama", extra_tensors=[spec("blk.1.attn_output.bias", (256,), G.GGML_F32, np.zeros(256))]), "blk.1.attn_output.bias", -9),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_the_load_refuses_what_it_would_get_wrong_and_names_the_tensor(what, tmp_path_factory):
    """ahead of the device: the same status and message with and without a GPU"""
    kw, tensor, status = REFUSALS[what]
    e = E.Engine()
    with pytest.raises(_lib.NtkError) as ei:
        e.load(model_file("qt64", tmp_path_factory, **kw), 128)
    assert ei.value.status == status and tensor in str(ei.value), str(ei.value)
    assert e.qkv_bias == -1                                           # nothing is loaded
    e.close()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_biases_move_the_logits_by_ten_bars_on_every_test_model(name, tmp_path_factory):
    """THE GUARD (see the module docstring)"""
    ref = oracle_ref(name, tmp_path_factory)
    for T in GUARD_LENGTHS:
        gap = dist(ref["prompt"][T], ref["plain"][T])
        print(name, "T", T, "bias-aware oracle - plain oracle: max |dlogit| =", gap)
        assert gap >= 10 * TOL, (name, T, gap)
    assert np.isfinite(ref["prompt"][70]).all() and dist(ref["chunked"], ref["prompt"][70]) <= 1e-4          # (the oracle itself: chunked = whole)


def test_the_cpp_generators_qwen2_file_is_what_the_reader_describes(tmp_path):
    """`qwen2:<mix>` in front of the mix: architecture string, keys under qwen2., three F32 bias vectors per layer behind attn_v.weight, each tensor the
    bytes nt_synth_tensor gives under that name; `qwen2-tied:` drops output.weight; without a prefix the file is the Llama file it always was."""
    tiny = dict(hidden=256, inter=512, layers=2, heads=4, kv_heads=2, vocab=512, ctx=256, bos=256, eos=257)

    def make(mix):
        return E.SynthSpec(tiny["hidden"], tiny["inter"], tiny["layers"], tiny["heads"], tiny["kv_heads"], tiny["vocab"], tiny["ctx"], 1e-6, 1e6, 256, 257, mix, 20260925)
    path = str(tmp_path / "q.gguf")
    E.synth_write_gguf(path, make(b"qwen2:Q8_0"), 2)
    d = E.gguf_describe(path)
    assert d["architecture"] == "qwen2" and d["n_heads"] == 4 and d["n_kv_heads"] == 2 and d["rope_theta"] == 1e6 and abs(d["norm_eps"] - 1e-6) < 1e-12
    assert len(d["tensors"]) == 3 + 12 * 2 and d["qkv_bias_tensors"] == 6
    names = [t["name"] for t in d["tensors"]]
    assert names[1:13] == ["blk.0." + n for n in ("attn_norm.weight", "attn_q.weight", "attn_k.weight", "attn_v.weight", "attn_q.bias", "attn_k.bias", "attn_v.bias",
                                                  "attn_output.weight", "ffn_norm.weight", "ffn_gate.weight", "ffn_up.weight", "ffn_down.weight")]
    f = G.read_gguf(path)
    assert "qwen2.block_count" in f.meta and "llama.block_count" not in f.meta
    for t in d["tensors"]:
        if t["name"].endswith(".bias"):
            n = 256 if "attn_q" in t["name"] else 128
            assert t["dims"] == [n] and t["type"] == "F32" and t["nbytes"] == 4 * n
            vals = f.f32(t["name"])
            assert np.isfinite(vals).all() and 0.2 < float(vals.std()) < 1.0             # seeded normal values of scale 0.5
            assert np.array_equal(E.synth_tensor(make(b"qwen2:Q8_0"), t["name"], 2).view("<f4"), vals)
    q_w = f.raw("blk.1.attn_q.weight").tobytes()
    # the tied flavour: the same tensors without output.weight
    tied = str(tmp_path / "t.gguf")
    E.synth_write_gguf(tied, make(b"qwen2-tied:Q8_0"), 2)
    dt = E.gguf_describe(tied)
    assert [t["name"] for t in dt["tensors"]] == [n for n in names if n != "output.weight"] and dt["qkv_bias_tensors"] == 6
    # the Llama file: the nine tensors per layer, and the matrices of the Qwen2 flavour are the Llama flavour's (seeded by name)
    plain = str(tmp_path / "l.gguf")
    E.synth_write_gguf(plain, make(b"Q8_0"), 2)
    dl = E.gguf_describe(plain)
    assert dl["architecture"] == "llama" and len(dl["tensors"]) == 3 + 9 * 2 and dl["qkv_bias_tensors"] == 0
    fl = G.read_gguf(plain)
    assert fl.raw("blk.1.attn_q.weight").tobytes() == q_w
    # the 7B shape of the benchmark: the plan's sizes (no bytes are generated)
    big = E.synth_spec("qwen2.5-7b", "Q8_0")
    L = E._bind()
    assert L.nt_synth_tensor(C.byref(big), b"blk.27.attn_q.bias", None, 0, 1) == 4 * 3584
    assert L.nt_synth_tensor(C.byref(big), b"blk.27.attn_v.bias", None, 0, 1) == 4 * 512
    assert L.nt_synth_tensor(C.byref(big), b"token_embd.weight", None, 0, 1) == 152064 * (3584 // 32) * 34
    assert L.nt_synth_tensor(C.byref(big), b"output.weight", None, 0, 1) == -9          # tied: no such tensor
    assert (G.QWEN25_7B.hidden, G.QWEN25_7B.inter, G.QWEN25_7B.layers, G.QWEN25_7B.heads, G.QWEN25_7B.kv_heads, G.QWEN25_7B.vocab) == (3584, 18944, 28, 28, 4, 152064)
