"""Qwen3 files on the CPU: the Python writer's qwen3 GGUF -- norm vectors, a head size of its own -- through both readers, the loader's refusals (ahead of
the device, so tested here without a GPU), the seeded C++ generator's Qwen3 flavour against the engine's own reader -- and THE GUARD of
tests/test_engine_qwen3_gpu.py:

test_the_norms_and_the_head_size_move_the_logits_by_ten_bars computes, with the oracle alone (tests/qwen3_ref.py), on every test model and at prompt
lengths 3, 4, 37 and 70, the distance between the norm-aware oracle's logits and (a) the same oracle without the norms, (b) the same oracle with the q and k
vectors swapped, (c) on the model whose heads x head_dim exceeds the hidden size, the oracle that keeps hidden / heads -- and asserts each is at least
10 x the 1e-3 logit bar.  An engine that drops the norms, swaps them or computes the head size from the hidden size is therefore at least 9 bars away
from the reference of every engine test.  NORM_AMP = 0.5 and the seed were chosen here."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from qwen3_ref import BIAS_SCALE, CTX, GUARD_LENGTHS, MODELS, NORM_AMP, SEED, TOL, Qwen3Oracle, dist, model_file, oracle_ref, prompt_tokens

GOLDEN_SEED = 20260925          # tools/make_golden.py


def fnv(name):
    h = 1469598103934665603
    for c in name.encode():
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


# ------------------------------------------------------------------------------------------------ the guard
@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_norms_and_the_head_size_move_the_logits_by_ten_bars(name, tmp_path_factory):
    """THE GUARD (see the module docstring)"""
    ref = oracle_ref(name, tmp_path_factory)
    shape, mix, arch, norms = MODELS[name]
    for T in GUARD_LENGTHS:
        assert np.isfinite(ref["prompt"][T]).all()
        for wrong in ("none", "swapped", "coupled"):
            if wrong in ref:
                gap = dist(ref["prompt"][T], ref[wrong][T])
                print(name, "T", T, "norm-aware oracle - the '%s' oracle: max |dlogit| =" % wrong, gap)
                assert gap >= 10 * TOL, (name, T, wrong, gap)
    assert ("none" in ref) == ("swapped" in ref) == norms
    assert ("coupled" in ref) == (name == "q3w128")          # (nemo128's hidden / heads = 256 would read projections the file does not have)
    assert dist(ref["chunked"], ref["prompt"][70]) <= 1e-4   # the oracle itself: chunked = whole


def test_the_order_of_bias_and_norm_moves_the_logits_by_ten_bars(tmp_path_factory):
    """the guard of test_engine_qwen3_gpu.py's bias + norm model: bias first (llama.cpp's order) against norm first, and against no bias at all"""
    path = model_file("q3n64", tmp_path_factory, qkv_bias=BIAS_SCALE)
    toks = prompt_tokens()
    for T in GUARD_LENGTHS:
        want = Qwen3Oracle(path, CTX).forward(toks[:T], 0)
        for wrong, m in (("norm first", Qwen3Oracle(path, CTX, bias_first=False)), ("no norm", Qwen3Oracle(path, CTX, norms="none")),
                         ("no bias", Qwen3Oracle(model_file("q3n64", tmp_path_factory), CTX))):
            gap = dist(want, m.forward(toks[:T], 0))
            print("bias + norm, T", T, "the oracle - the '%s' oracle: max |dlogit| =" % wrong, gap)
            assert np.isfinite(want).all() and gap >= 10 * TOL, (T, wrong, gap)


def test_the_plain_oracle_cannot_stand_in_on_a_decoupled_file(tmp_path_factory):
    """nemo128 carries no norm: what separates it from a Llama file is the head size alone -- the file states 128, hidden / heads is 256"""
    f = G.read_gguf(model_file("nemo128", tmp_path_factory))
    assert G.model_head_dim(f.meta) == 128 and f.meta["llama.embedding_length"] // f.meta["llama.attention.head_count"] == 256
    assert tuple(f.tensors["blk.0.attn_q.weight"].dims) == (512, 256) and tuple(f.tensors["blk.0.attn_output.weight"].dims) == (256, 512)


# ------------------------------------------------------------------------------------------------ readers and writer
def test_the_writers_qwen3_file_through_both_readers(tmp_path_factory):
    for name in sorted(MODELS):
        shape, mix, arch, norms = MODELS[name]
        path = model_file(name, tmp_path_factory)
        f = G.read_gguf(path)
        d = E.gguf_describe(path)
        assert d["architecture"] == arch and f.meta["general.architecture"] in (arch, arch.encode())
        hd = shape.head_dim or shape.hidden // shape.heads
        assert d["head_dim"] == hd == G.model_head_dim(f.meta) == shape.hd, name
        assert (arch + ".attention.key_length" in f.meta) == bool(shape.head_dim) == (arch + ".attention.value_length" in f.meta)
        if shape.head_dim:
            assert f.meta[arch + ".attention.key_length"] == f.meta[arch + ".attention.value_length"] == shape.head_dim
        assert d["hidden_size"] == shape.hidden and d["n_heads"] == shape.heads and d["n_kv_heads"] == shape.kv_heads and d["n_layers"] == 2
        assert d["qk_norm_tensors"] == (2 * shape.layers if norms else 0) and d["qkv_bias_tensors"] == 0
        table = {t["name"]: t for t in d["tensors"]}
        assert len(table) == len(f.tensors) == 3 + (11 if norms else 9) * shape.layers
        assert table["blk.1.attn_q.weight"]["dims"] == [shape.hidden, shape.heads * hd] and table["blk.1.attn_k.weight"]["dims"] == [shape.hidden, shape.kv_heads * hd]
        assert table["blk.1.attn_output.weight"]["dims"] == [shape.heads * hd, shape.hidden]
        raw = open(path, "rb").read()
        for i in range(shape.layers if norms else 0):
            for which in "qk":
                nm = "blk.%d.attn_%s_norm.weight" % (i, which)
                assert tuple(f.tensors[nm].dims) == (hd,) and f.tensors[nm].ggml_type == G.GGML_F32
                assert table[nm]["dims"] == [hd] and table[nm]["type"] == "F32" and table[nm]["nbytes"] == 4 * hd
                a = d["data_offset"] + table[nm]["offset"]                    # the C++ reader's offsets lead to the Python reader's bytes
                assert raw[a:a + 4 * hd] == f.f32(nm).tobytes()
                want = (1.0 + NORM_AMP * np.random.Generator(np.random.Philox(key=[SEED, fnv(nm)])).uniform(-1, 1, hd)).astype("<f4")
                assert np.array_equal(f.f32(nm), want) and 0.5 <= float(want.min()) and float(want.max()) < 1.5
        if norms:          # behind attn_v.weight, as llama.cpp's converter orders them
            names = [t["name"] for t in d["tensors"]]
            at = names.index("blk.0.attn_v.weight")
            assert names[at + 1:at + 4] == ["blk.0.attn_q_norm.weight", "blk.0.attn_k_norm.weight", "blk.0.attn_output.weight"]
    # a dict writes only the named vector
    only_k = model_file("q3n64", tmp_path_factory, qk_norm={"k": NORM_AMP})
    assert E.gguf_describe(only_k)["qk_norm_tensors"] == 2


def test_a_file_without_the_new_arguments_is_the_file_it_always_was(tmp_path):
    """no new key, no new tensor, the same bytes -- against the committed golden file the writer produced before it learnt any of this"""
    golden = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    gf = G.read_gguf(golden)
    path = str(tmp_path / "tiny.gguf")
    G.make_synthetic_llama(path, G.TINY, "Q8_0", seed=GOLDEN_SEED)          # tools/make_golden.py's call
    f = G.read_gguf(path)
    assert not [k for k in f.meta if "key_length" in k or "value_length" in k]
    assert not [n for n in f.tensors if "attn_q_norm" in n or "attn_k_norm" in n]
    d = E.gguf_describe(path)
    assert d["qk_norm_tensors"] == 0 and d["head_dim"] == 64
    assert sorted(gf.tensors) == sorted(f.tensors) and open(path, "rb").read() == open(golden, "rb").read()
    # ... and head_dim=0, qk_norm=None, extra_kvs=() spelled out change nothing
    again = str(tmp_path / "again.gguf")
    G.make_synthetic_llama(again, G.LlamaShape("tiny", 256, 512, 2, 4, 2, 512, ctx=256, bos=256, eos=257, head_dim=0), "Q8_0", seed=GOLDEN_SEED, qk_norm=None, extra_kvs=())
    assert open(again, "rb").read() == open(path, "rb").read()


def test_no_golden_file_carries_a_norm_or_a_head_size():
    files = sorted(glob.glob(os.path.join(GOLDEN, "*.gguf")))
    assert len(files) >= 4
    for path in files:
        d = E.gguf_describe(path)
        assert d["qk_norm_tensors"] == 0 and d["head_dim"] * d["n_heads"] == d["hidden_size"], path


def test_the_cpp_generators_qwen3_file_is_what_the_reader_describes(tmp_path):
    """`qwen3-hd128-tied:<mix>`: architecture and keys qwen3, key_length = value_length = 128, projections of heads x 128, two F32 norm vectors per layer
    behind attn_v.weight with values 1 + 0.5 u, no output.weight; each tensor the bytes nt_synth_tensor gives under that name; `hd128-tied:` is the same
    model under `llama` without the norm vectors; without a prefix the file is the Llama file it always was."""
    tiny = dict(hidden=256, inter=512, layers=2, heads=4, kv_heads=2, vocab=512, ctx=256, bos=256, eos=257)

    def make(mix):
        return E.SynthSpec(tiny["hidden"], tiny["inter"], tiny["layers"], tiny["heads"], tiny["kv_heads"], tiny["vocab"], tiny["ctx"], 1e-6, 1e6, 256, 257, mix, 20260925)
    path = str(tmp_path / "q.gguf")
    E.synth_write_gguf(path, make(b"qwen3-hd128-tied:Q8_0"), 2)
    d = E.gguf_describe(path)
    assert d["architecture"] == "qwen3" and d["n_heads"] == 4 and d["n_kv_heads"] == 2 and d["head_dim"] == 128 and d["hidden_size"] == 256
    assert d["rope_theta"] == 1e6 and abs(d["norm_eps"] - 1e-6) < 1e-12
    assert len(d["tensors"]) == 2 + 11 * 2 and d["qk_norm_tensors"] == 4 and d["qkv_bias_tensors"] == 0
    names = [t["name"] for t in d["tensors"]]
    assert names[0] == "token_embd.weight" and names[-1] == "output_norm.weight" and "output.weight" not in names
    assert names[1:12] == ["blk.0." + n for n in ("attn_norm.weight", "attn_q.weight", "attn_k.weight", "attn_v.weight", "attn_q_norm.weight", "attn_k_norm.weight",
                                                  "attn_output.weight", "ffn_norm.weight", "ffn_gate.weight", "ffn_up.weight", "ffn_down.weight")]
    f = G.read_gguf(path)
    assert "qwen3.block_count" in f.meta and "llama.block_count" not in f.meta
    assert f.meta["qwen3.attention.key_length"] == f.meta["qwen3.attention.value_length"] == 128 and G.model_head_dim(f.meta) == 128
    want_dims = {"attn_q.weight": [256, 512], "attn_k.weight": [256, 256], "attn_v.weight": [256, 256], "attn_output.weight": [512, 256],
                 "attn_q_norm.weight": [128], "attn_k_norm.weight": [128], "attn_norm.weight": [256], "ffn_norm.weight": [256],
                 "ffn_gate.weight": [256, 512], "ffn_up.weight": [256, 512], "ffn_down.weight": [512, 256]}
    for t in d["tensors"]:          # tensor for tensor
        stem = t["name"].split(".", 2)[2] if t["name"].startswith("blk.") else None
        if stem:
            assert t["dims"] == want_dims[stem], t
        got = E.synth_tensor(make(b"qwen3-hd128-tied:Q8_0"), t["name"], 2)
        assert t["nbytes"] == got.nbytes and f.raw(t["name"]).tobytes() == got.tobytes(), t["name"]
        if stem in ("attn_q_norm.weight", "attn_k_norm.weight"):
            vals = f.f32(t["name"])
            assert t["type"] == "F32" and 0.5 <= float(vals.min()) < 0.75 and 1.25 < float(vals.max()) < 1.5          # 1 + 0.5 u over 128 draws
    assert not np.array_equal(f.f32("blk.0.attn_q_norm.weight"), f.f32("blk.0.attn_k_norm.weight"))          # seeded by name
    # the norm-free twin under `llama`: the same matrices, no norm vectors
    twin = str(tmp_path / "t.gguf")
    E.synth_write_gguf(twin, make(b"hd128-tied:Q8_0"), 2)
    dt = E.gguf_describe(twin)
    assert dt["architecture"] == "llama" and dt["head_dim"] == 128 and dt["qk_norm_tensors"] == 0
    assert [t["name"] for t in dt["tensors"]] == [n for n in names if "_norm.weight" not in n or "attn_q_norm" not in n and "attn_k_norm" not in n]
    assert G.read_gguf(twin).raw("blk.1.attn_q.weight").tobytes() == f.raw("blk.1.attn_q.weight").tobytes()
    # coupled: `qwen3:` writes no key_length
    coupled = str(tmp_path / "c.gguf")
    E.synth_write_gguf(coupled, make(b"qwen3:Q8_0"), 2)
    dc = E.gguf_describe(coupled)
    assert dc["head_dim"] == 64 and dc["qk_norm_tensors"] == 4 and "qwen3.attention.key_length" not in G.read_gguf(coupled).meta
    assert "output.weight" in [t["name"] for t in dc["tensors"]]
    # without a prefix: the Llama file, byte for byte the committed one's plan
    plain = str(tmp_path / "l.gguf")
    E.synth_write_gguf(plain, make(b"Q8_0"), 2)
    dl = E.gguf_describe(plain)
    assert dl["architecture"] == "llama" and len(dl["tensors"]) == 3 + 9 * 2 and dl["qk_norm_tensors"] == 0 and dl["head_dim"] == 64
    # a bad head size in the flavour is refused
    for bad in (b"qwen3-hd0:Q8_0", b"qwen3-hd127:Q8_0", b"qwen3-hdx:Q8_0", b"qwen4:Q8_0"):
        with pytest.raises(_lib.NtkError):
            E.synth_write_gguf(str(tmp_path / "bad.gguf"), make(bad), 2)
    # the named shapes of the benchmark: the plan's sizes (no bytes are generated)
    L = E._bind()
    big = E.synth_spec("qwen3-4b", "Q8_0")
    assert L.nt_synth_tensor(C.byref(big), b"blk.35.attn_q_norm.weight", None, 0, 1) == 4 * 128
    assert L.nt_synth_tensor(C.byref(big), b"blk.35.attn_q.weight", None, 0, 1) == 4096 * (2560 // 32) * 34          # 32 heads x 128 rows of 2560
    assert L.nt_synth_tensor(C.byref(big), b"blk.35.attn_output.weight", None, 0, 1) == 2560 * (4096 // 32) * 34
    assert L.nt_synth_tensor(C.byref(big), b"output.weight", None, 0, 1) == -9          # tied
    twin4 = E.synth_spec("qwen3-4b-nonorm", "Q8_0")
    assert L.nt_synth_tensor(C.byref(twin4), b"blk.35.attn_q_norm.weight", None, 0, 1) == -9
    assert L.nt_synth_tensor(C.byref(twin4), b"blk.35.attn_q.weight", None, 0, 1) == 4096 * (2560 // 32) * 34
    big8 = E.synth_spec("qwen3-8b", "Q8_0")
    assert L.nt_synth_tensor(C.byref(big8), b"blk.0.attn_k_norm.weight", None, 0, 1) == 4 * 128
    assert L.nt_synth_tensor(C.byref(big8), b"output.weight", None, 0, 1) == 151936 * (4096 // 32) * 34          # untied
    assert L.nt_synth_tensor(C.byref(E.synth_spec("qwen3-8b-nonorm", "Q8_0")), b"blk.0.attn_k_norm.weight", None, 0, 1) == -9
    assert (G.QWEN3_4B.hidden, G.QWEN3_4B.inter, G.QWEN3_4B.layers, G.QWEN3_4B.heads, G.QWEN3_4B.kv_heads, G.QWEN3_4B.hd, G.QWEN3_4B.vocab) == (2560, 9728, 36, 32, 8, 128, 151936)
    assert (G.QWEN3_8B.hidden, G.QWEN3_8B.inter, G.QWEN3_8B.layers, G.QWEN3_8B.heads, G.QWEN3_8B.kv_heads, G.QWEN3_8B.hd, G.QWEN3_8B.vocab) == (4096, 12288, 36, 32, 8, 128, 151936)


# ------------------------------------------------------------------------------------------------ refusals ahead of the device
def spec(name, dims, ggml_type, values):
    return G.TensorSpec(name, dims, ggml_type, np.asarray(values).astype("<f2" if ggml_type == G.GGML_F16 else "<f4").tobytes())


def pair(layer, n=128):
    return [spec("blk.%d.attn_%s_norm.weight" % (layer, w), (n,), G.GGML_F32, np.ones(n)) for w in "qk"]


W128 = G.QWEN3_W128          # hidden 256, head_dim 128
REFUSALS = {
    # what: (model, arguments of make_synthetic_llama, what the message must name, status)
    "f16_norm": ("q3w128", dict(qk_norm={"q": 0.5}, extra_tensors=[spec("blk.0.attn_k_norm.weight", (128,), G.GGML_F16, np.ones(128)),
                                                                   spec("blk.1.attn_k_norm.weight", (128,), G.GGML_F32, np.ones(128))]), "blk.0.attn_k_norm.weight", -1),
    "norm_of_head_dim_plus_1": ("q3w128", dict(qk_norm={"k": 0.5}, extra_tensors=[spec("blk.0.attn_q_norm.weight", (128,), G.GGML_F32, np.ones(128)),
                                                                                  spec("blk.1.attn_q_norm.weight", (129,), G.GGML_F32, np.ones(129))]), "blk.1.attn_q_norm.weight", -2),
    "norm_of_head_dim_minus_1": ("q3w128", dict(qk_norm={"q": 0.5}, extra_tensors=[spec("blk.0.attn_k_norm.weight", (127,), G.GGML_F32, np.ones(127)),
                                                                                   spec("blk.1.attn_k_norm.weight", (128,), G.GGML_F32, np.ones(128))]), "blk.0.attn_k_norm.weight", -2),
    "norm_of_hidden_values": ("q3w128", dict(qk_norm={"k": 0.5}, extra_tensors=[spec("blk.0.attn_q_norm.weight", (256,), G.GGML_F32, np.ones(256)),
                                                                                spec("blk.1.attn_q_norm.weight", (256,), G.GGML_F32, np.ones(256))]), "blk.0.attn_q_norm.weight", -2),
    "lone_k_norm_beside_full_pairs": ("q3g128", dict(qk_norm=None, extra_tensors=pair(0) + [spec("blk.1.attn_k_norm.weight", (128,), G.GGML_F32, np.ones(128))]),
                                      "blk.1.attn_k_norm.weight", -9),
    "pair_on_layer_5_of_2": ("q3w128", dict(extra_tensors=pair(5)), "blk.5.attn_q_norm.weight", -9),
    "value_length_differs": ("q3w128", dict(extra_kvs=[]), "qwen3.attention.value_length", -9),          # (built below: the writer writes both keys alike)
    "odd_key_length": ("q3w128", None, "qwen3.attention.key_length", -9),
    "zero_key_length": ("q3w128", None, "qwen3.attention.key_length", -9),
}


def refusal_file(what, tmp_path_factory):
    name, kw, _, _ = REFUSALS[what]
    if what in ("value_length_differs", "odd_key_length", "zero_key_length"):
        # the writer states key_length = value_length = shape.head_dim; these files state the pair themselves, on the coupled shape with 128-wide projections
        # left out of the question: the reader refuses on the metadata, ahead of any tensor
        key, val = {"value_length_differs": (128, 64), "odd_key_length": (127, 127), "zero_key_length": (0, 0)}[what]
        return model_file("q3n64", tmp_path_factory, qk_norm=None,
                          extra_kvs=[G.kv_u32("qwen3.attention.key_length", key), G.kv_u32("qwen3.attention.value_length", val)])
    return model_file(name, tmp_path_factory, **kw)


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_the_load_refuses_ahead_of_the_device_and_names_the_tensor_or_key(what, tmp_path_factory):
    """the same status and message with and without a GPU"""
    _, _, named, status = REFUSALS[what]
    path = refusal_file(what, tmp_path_factory)
    e = E.Engine()
    with pytest.raises(_lib.NtkError) as ei:
        e.load(path, 128)
    assert ei.value.status == status and named in str(ei.value), str(ei.value)
    assert e.qk_norm == -1                                           # nothing is loaded
    e.close()
    if "length" in what:          # ... and the Python reader refuses the same metadata, naming the key
        with pytest.raises(ValueError) as vi:
            G.model_head_dim(G.read_gguf(path).meta)
        assert named in str(vi.value)


def test_the_remaining_unsupported_tensors_are_still_refused_by_name(tmp_path_factory):
    path = model_file("q3n64", tmp_path_factory, extra_tensors=[spec("blk.1.attn_output.bias", (256,), G.GGML_F32, np.zeros(256))])
    e = E.Engine()
    with pytest.raises(_lib.NtkError) as ei:
        e.load(path, 128)
    assert ei.value.status == -9 and "blk.1.attn_output.bias" in str(ei.value) and "Qwen3" in str(ei.value)
    e.close()
