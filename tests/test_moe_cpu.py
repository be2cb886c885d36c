"""Mixture-of-experts files on the CPU: the Python writer's expert quartet through both readers, the loader's refusals (ahead of the device, so tested here
without a GPU), the seeded C++ generator's moe flavour against the engine's own reader, the workspace layout, the work-list builder -- and THE GUARD of
tests/test_engine_moe_gpu.py, computed with the oracle alone (tests/moe_ref.py):

  1. on every test model and at prompt lengths 3 / 4 / 37 / 70 every WRONG oracle -- the softmax over all E without renormalising, uniform weights 1 / K, the
     K smallest logits, gate and up swapped, the down expert reversed -- is at least ten engine bars (1e-2) from MoEOracle in the logits;
  2. at every (pass, layer, row) the GPU engine tests run -- the prompts, the chunked pass, the decode steps, the slot tests, the q8_0 test's passes -- the gap
     between the K-th and the (K + 1)-th router logit is at least 16 x tol_for(logits, hidden), tol_for the GEMV bar 4e-6 sqrt(in) max(1, |y|max).  That is a
     CONDITION on the inputs: a selection that flips between two summation orders would turn a rounding difference into a wrong-expert failure, or hide one.
     The seeds and ROUTER_SCALE of moe_ref were searched here until the oracle alone meets it (found: ratios 4.7 / 15.8 / 6.5 / 7.3 at seed 20261101)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from moe_ref import CTX, GUARD_LENGTHS, MODELS, ROUTER_SCALE, SEEDS, TOL, WRONG, MoEOracle, dist, model_file, oracle_ref, select_experts, work_list
from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G

GOLDEN_SEED = 20260925          # tools/make_golden.py


def fnv(name):
    h = 1469598103934665603
    for c in name.encode():
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


# ------------------------------------------------------------------------------------------------ the guard
@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_wrong_oracle_is_ten_bars_away_and_the_routing_gaps_are_wide(name, tmp_path_factory):
    """THE GUARD (see the module docstring)"""
    ref = oracle_ref(name, tmp_path_factory)
    for T in GUARD_LENGTHS:
        assert np.isfinite(ref["prompt"][T]).all()
        for wrong in WRONG:
            gap = dist(ref["prompt"][T], ref[wrong][T])
            print(name, "T", T, "routing oracle - the '%s' oracle: max |dlogit| =" % wrong, gap)
            assert gap >= 10 * TOL, (name, T, wrong, gap)
    print(name, "smallest routing gap over every row the GPU tests run: %.3f x (16 tol_for)" % ref["gap"])
    assert ref["gap"] >= 1.0, (name, ref["gap"])
    assert dist(ref["chunked"], ref["prompt"][70]) <= 1e-4          # the oracle itself: chunked = whole


def test_the_work_list_builder_is_numpys_stable_argsort():
    r = np.random.Generator(np.random.Philox(key=[20261101, 5]))
    for T, n_exp, K in ((1, 4, 2), (17, 8, 2), (70, 128, 8), (5, 256, 16), (3, 4, 4)):
        ids = np.stack([r.permutation(n_exp)[:K] for _ in range(T)]).astype(np.int32)
        offsets, pairs = work_list(ids, n_exp)
        assert np.array_equal(pairs, np.argsort(ids.reshape(-1), kind="stable"))
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(np.bincount(ids.reshape(-1), minlength=n_exp))]))
    lg = np.asarray([1.0, 3.0, 3.0, -1.0, 3.0, 0.5], np.float32)          # equal logits: the lower expert first
    assert list(select_experts(lg, 4)) == [1, 2, 4, 0] and list(select_experts(lg, 2, smallest=True)) == [3, 5]


def test_the_workspace_size_is_what_its_layout_addresses():
    L = _lib.lib()
    for T, n_exp, K, ie, hidden in ((1, 4, 2, 96, 256), (17, 8, 2, 768, 256), (1024, 128, 8, 768, 2048), (1024, 8, 2, 14336, 4096), (3, 256, 16, 32, 64)):
        off = (C.c_size_t * 7)()
        total = L.ntk_moe_workspace_layout(T, n_exp, K, ie, hidden, off)
        assert total == L.ntk_moe_workspace_bytes(T, n_exp, K, ie, hidden) > 0
        need = [T * hidden * 4, T * K * ie * 4, T * K * hidden * 4, T * K * 4, T * K * 4, T * K * 4, (n_exp + 1) * 4]          # xn act part w ids pairs offsets
        spans = sorted((int(off[i]), int(off[i]) + need[i]) for i in range(7))
        assert spans[0][0] == 0 and all(a % 256 == 0 for a, _ in spans)
        assert all(spans[i][1] <= spans[i + 1][0] for i in range(6))          # no two sections overlap
        assert spans[-1][1] <= total < spans[-1][1] + 256                     # ... and the size is the last byte addressed, rounded to 256
    for bad in ((0, 4, 2, 96, 256), (1025, 4, 2, 96, 256), (1, 257, 2, 96, 256), (1, 4, 5, 96, 256), (1, 32, 17, 96, 256), (1, 4, 0, 96, 256), (1, 4, 2, 0, 256)):
        assert L.ntk_moe_workspace_bytes(*bad) == 0


# ------------------------------------------------------------------------------------------------ readers and writer
def test_the_writers_moe_file_through_both_readers(tmp_path_factory):
    for name in sorted(MODELS):
        shape, mix, arch, norms, n_exp, K, ie, layers, over = MODELS[name]
        ie = ie or shape.inter
        path = model_file(name, tmp_path_factory)
        f = G.read_gguf(path)
        d = E.gguf_describe(path)
        routed = list(range(shape.layers)) if layers is None else list(layers)
        assert d["architecture"] == arch and d["expert_count"] == n_exp == f.meta[arch + ".expert_count"]
        assert d["expert_used_count"] == K == f.meta[arch + ".expert_used_count"] and d["expert_feed_forward_length"] == ie and d["moe_layers"] == len(routed)
        assert (arch + ".expert_feed_forward_length" in f.meta) == (MODELS[name][6] is not None)
        table = {t["name"]: t for t in d["tensors"]}
        assert len(table) == len(f.tensors)
        raw = open(path, "rb").read()
        for i in range(shape.layers):
            p = "blk.%d." % i
            assert (p + "ffn_gate.weight" in table) == (p + "ffn_up.weight" in table) == (p + "ffn_down.weight" in table) == (i not in routed)
            assert (p + "ffn_gate_inp.weight" in table) == (i in routed)
            if i not in routed:
                continue
            assert table[p + "ffn_gate_inp.weight"]["dims"] == [shape.hidden, n_exp] and table[p + "ffn_gate_inp.weight"]["type"] == "F32"
            want = (ROUTER_SCALE / np.sqrt(shape.hidden) * np.random.Generator(np.random.Philox(key=[SEEDS[name], fnv(p + "ffn_gate_inp.weight")]))
                    .standard_normal(n_exp * shape.hidden)).astype("<f4")
            assert np.array_equal(f.f32(p + "ffn_gate_inp.weight"), want)
            for m, dims in (("ffn_gate_exps", [shape.hidden, ie, n_exp]), ("ffn_up_exps", [shape.hidden, ie, n_exp]), ("ffn_down_exps", [ie, shape.hidden, n_exp])):
                t = table[p + m + ".weight"]
                assert t["dims"] == dims == list(f.tensors[p + m + ".weight"].dims)
                rb = G.row_bytes(t["ggml_type"], dims[0])
                assert t["nbytes"] == rb * dims[1] * dims[2] == f.tensors[p + m + ".weight"].nbytes
                a = d["data_offset"] + t["offset"]          # the C++ reader's offsets lead to the Python reader's bytes, expert by expert
                for e in (0, n_exp - 1):
                    n = rb * dims[1]
                    assert raw[a + e * n:a + (e + 1) * n] == f.raw(p + m + ".weight")[e * n:(e + 1) * n].tobytes()
            names = [t["name"] for t in d["tensors"]]
            at = names.index(p + "ffn_norm.weight")
            assert names[at + 1:at + 5] == [p + n for n in ("ffn_gate_inp.weight", "ffn_gate_exps.weight", "ffn_up_exps.weight", "ffn_down_exps.weight")]
        if name == "moe4k":          # Q4_K_M with Q6_K down experts: 630-byte rows
            assert table["blk.0.ffn_gate_exps.weight"]["type"] == "Q4_K_M" and table["blk.0.ffn_down_exps.weight"]["type"] == "Q6_K"
            assert G.row_bytes(G.GGML_Q6_K, 768) == 630
        # the oracle's expert slice dequantises to the rows the whole tensor dequantises to
        m = MoEOracle(path, CTX)
        i = routed[-1]
        blk, dt = m.expert("blk.%d.ffn_down_exps.weight" % i, n_exp - 1, shape.hidden, ie)
        gt = f.tensors["blk.%d.ffn_down_exps.weight" % i].ggml_type
        whole = G.dequantize(np.array(f.raw("blk.%d.ffn_down_exps.weight" % i)), gt, ie * shape.hidden * n_exp).reshape(n_exp, shape.hidden, ie)
        assert np.array_equal(G.dequantize(np.array(blk), gt, ie * shape.hidden).reshape(shape.hidden, ie), whole[n_exp - 1]) and dt == G.GGML_TO_DT[gt]


def test_a_file_without_the_new_arguments_is_the_file_it_always_was(tmp_path):
    golden = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    path = str(tmp_path / "tiny.gguf")
    G.make_synthetic_llama(path, G.TINY, "Q8_0", seed=GOLDEN_SEED)          # tools/make_golden.py's call
    assert open(path, "rb").read() == open(golden, "rb").read()
    again = str(tmp_path / "again.gguf")
    G.make_synthetic_llama(again, G.TINY, "Q8_0", seed=GOLDEN_SEED, experts=None, experts_used=None, expert_inter=None, router_scale=3.0, moe_layers=None)
    assert open(again, "rb").read() == open(golden, "rb").read()
    d = E.gguf_describe(path)
    assert (d["expert_count"], d["expert_used_count"], d["expert_feed_forward_length"], d["moe_layers"]) == (0, 0, 0, 0)
    assert not [k for k in G.read_gguf(path).meta if "expert" in k]


def test_the_cpp_generators_moe_file_is_what_the_reader_describes(tmp_path):
    """`qwen3-hd128-moe4x2-i96:<mix>`: architecture qwen3moe, the expert keys, per layer the F32 router and three 3-D expert tensors in place of the dense
    trio, each tensor the bytes nt_synth_tensor gives under that name; Q4_K_M gives ffn_down_exps the type it gives ffn_down; `moe4x2:` under `llama`
    writes no expert_feed_forward_length; without the token the file is the file it always was; counts outside the limits are refused."""
    def make(mix):
        return E.SynthSpec(256, 512, 2, 4, 2, 512, 256, 1e-6, 1e6, 256, 257, mix, 20260925)
    path = str(tmp_path / "m.gguf")
    E.synth_write_gguf(path, make(b"qwen3-hd128-moe4x2-i256:Q4_K_M"), 2)
    d = E.gguf_describe(path)
    assert d["architecture"] == "qwen3moe" and d["head_dim"] == 128 and d["qk_norm_tensors"] == 4
    assert (d["expert_count"], d["expert_used_count"], d["expert_feed_forward_length"], d["moe_layers"]) == (4, 2, 256, 2)
    names = [t["name"] for t in d["tensors"]]
    assert names[1:13] == ["blk.0." + n for n in ("attn_norm.weight", "attn_q.weight", "attn_k.weight", "attn_v.weight", "attn_q_norm.weight", "attn_k_norm.weight",
                                                  "attn_output.weight", "ffn_norm.weight", "ffn_gate_inp.weight", "ffn_gate_exps.weight", "ffn_up_exps.weight",
                                                  "ffn_down_exps.weight")]
    assert not [n for n in names if n.endswith(("ffn_gate.weight", "ffn_up.weight", "ffn_down.weight"))]
    f = G.read_gguf(path)
    assert f.meta["qwen3moe.expert_count"] == 4 and f.meta["qwen3moe.expert_used_count"] == 2 and f.meta["qwen3moe.expert_feed_forward_length"] == 256
    want_dims = {"ffn_gate_inp.weight": [256, 4], "ffn_gate_exps.weight": [256, 256, 4], "ffn_up_exps.weight": [256, 256, 4], "ffn_down_exps.weight": [256, 256, 4]}
    for t in d["tensors"]:          # tensor for tensor
        stem = t["name"].split(".", 2)[2] if t["name"].startswith("blk.") else None
        if stem in want_dims:
            assert t["dims"] == want_dims[stem], t
        got = E.synth_tensor(make(b"qwen3-hd128-moe4x2-i256:Q4_K_M"), t["name"], 2)
        assert t["nbytes"] == got.nbytes and f.raw(t["name"]).tobytes() == got.tobytes(), t["name"]
    table = {t["name"]: t for t in d["tensors"]}
    assert table["blk.0.ffn_gate_inp.weight"]["type"] == "F32" and table["blk.0.ffn_gate_exps.weight"]["type"] == "Q4_K_M"
    assert table["blk.1.ffn_down_exps.weight"]["type"] == "Q6_K" and table["blk.0.ffn_down_exps.weight"]["type"] == "Q4_K_M"          # use_more_bits(1, 2)
    router = f.f32("blk.0.ffn_gate_inp.weight")
    assert 0.5 * 2.0 / 16 < float(router.std()) < 1.5 * 2.0 / 16          # scale 2 / sqrt(hidden)
    # under `llama`, no -i: the experts have the spec's inter and the file no expert_feed_forward_length
    mix = str(tmp_path / "x.gguf")
    E.synth_write_gguf(mix, make(b"moe4x2:Q8_0"), 2)
    dm = E.gguf_describe(mix)
    assert dm["architecture"] == "llama" and dm["expert_feed_forward_length"] == 512 and "llama.expert_feed_forward_length" not in G.read_gguf(mix).meta
    assert {t["name"]: t for t in dm["tensors"]}["blk.1.ffn_up_exps.weight"]["dims"] == [256, 512, 4]
    # without the token: the Llama file
    plain = str(tmp_path / "l.gguf")
    E.synth_write_gguf(plain, make(b"Q8_0"), 2)
    dl = E.gguf_describe(plain)
    assert dl["architecture"] == "llama" and len(dl["tensors"]) == 3 + 9 * 2 and dl["moe_layers"] == 0 and dl["expert_count"] == 0
    for bad in (b"moe0x1:Q8_0", b"moe257x2:Q8_0", b"moe4x5:Q8_0", b"moe32x17:Q8_0", b"moe4x0:Q8_0", b"moe4:Q8_0", b"moe4x2-i0:Q8_0", b"moe4x2y:Q8_0"):
        with pytest.raises(_lib.NtkError):
            E.synth_write_gguf(str(tmp_path / "bad.gguf"), make(bad), 2)
    # the named shapes of the benchmark: the plan's sizes (no bytes are generated)
    L = E._bind()
    big = E.synth_spec("qwen3-30b-a3b", "Q8_0")
    assert L.nt_synth_tensor(C.byref(big), b"blk.47.ffn_gate_inp.weight", None, 0, 1) == 4 * 2048 * 128
    assert L.nt_synth_tensor(C.byref(big), b"blk.47.ffn_gate_exps.weight", None, 0, 1) == 128 * 768 * (2048 // 32) * 34
    assert L.nt_synth_tensor(C.byref(big), b"blk.47.ffn_down_exps.weight", None, 0, 1) == 128 * 2048 * (768 // 32) * 34
    assert L.nt_synth_tensor(C.byref(big), b"blk.47.ffn_gate.weight", None, 0, 1) == -9
    assert L.nt_synth_tensor(C.byref(big), b"blk.0.attn_q.weight", None, 0, 1) == 4096 * (2048 // 32) * 34          # 32 heads of 128 over a hidden size of 2048
    mx = E.synth_spec("mixtral-8x7b", "Q4_K_M")
    assert L.nt_synth_tensor(C.byref(mx), b"blk.0.ffn_up_exps.weight", None, 0, 1) == 8 * 14336 * (4096 // 256) * 144
    assert L.nt_synth_tensor(C.byref(mx), b"blk.0.ffn_down_exps.weight", None, 0, 1) == 8 * 4096 * (14336 // 256) * 210          # use_more_bits(0, 32)
    assert (G.QWEN3_30B_A3B.hidden, G.QWEN3_30B_A3B.layers, G.QWEN3_30B_A3B.heads, G.QWEN3_30B_A3B.kv_heads, G.QWEN3_30B_A3B.hd, G.QWEN3_30B_A3B.vocab) == (2048, 48, 32, 4, 128, 151936)
    assert (G.MIXTRAL_8X7B.hidden, G.MIXTRAL_8X7B.inter, G.MIXTRAL_8X7B.layers, G.MIXTRAL_8X7B.heads, G.MIXTRAL_8X7B.kv_heads) == (4096, 14336, 32, 32, 8)


# ------------------------------------------------------------------------------------------------ refusals ahead of the device
def zeros(name, dims, ggml_type):
    n = int(np.prod(dims))
    return G.TensorSpec(name, tuple(dims), ggml_type, bytes(G.row_bytes(ggml_type, n)))


def rewrite(src, dst, drop=(), add=()):
    """`src` again without the tensors named in `drop` and with the specs of `add` appended; the metadata byte for byte (gguf.write_f32_twin's construction)"""
    f = G.read_gguf(src)
    kvs = [bytes(f._buf[f.kv_span[0]:f.kv_span[1]])] + [b""] * (len(f.meta) - 1)
    specs = [G.TensorSpec(n, ti.dims, ti.ggml_type, bytes(f.raw(n))) for n, ti in f.tensors.items() if n not in drop] + list(add)
    f.close()
    G.write_gguf(dst, kvs, specs)
    return dst


Q8, Q4K, F32, F16 = G.GGML_Q8_0, G.GGML_Q4_K, G.GGML_F32, G.GGML_F16
# what: (how the file is made, what the message must name, status).  The base model is moe8q8: qwen3moe, hidden 256, E 8, K 2, I_e 96, Q8_0.
REFUSALS = {
    "both_forms_on_one_layer": (dict(add=[zeros("blk.0.ffn_gate.weight", (256, 512), Q8)]), "blk.0.ffn_gate.weight", -9),
    "partial_quartet": (dict(drop=["blk.1.ffn_up_exps.weight"]), "blk.1.ffn_up_exps.weight", -9),
    "lone_router": (dict(drop=["blk.0.ffn_gate_exps.weight", "blk.0.ffn_up_exps.weight", "blk.0.ffn_down_exps.weight"]), "blk.0.ffn_gate_exps.weight", -9),
    "quartet_on_layer_5_of_2": (dict(add=[zeros("blk.5.ffn_gate_inp.weight", (256, 8), F32)]), "blk.5.ffn_gate_inp.weight", -9),
    "f16_router": (dict(drop=["blk.0.ffn_gate_inp.weight"], add=[zeros("blk.0.ffn_gate_inp.weight", (256, 8), F16)]), "blk.0.ffn_gate_inp.weight", -1),
    "router_of_7_experts": (dict(drop=["blk.1.ffn_gate_inp.weight"], add=[zeros("blk.1.ffn_gate_inp.weight", (256, 7), F32)]), "blk.1.ffn_gate_inp.weight", -2),
    "router_transposed": (dict(drop=["blk.1.ffn_gate_inp.weight"], add=[zeros("blk.1.ffn_gate_inp.weight", (8, 256), F32)]), "blk.1.ffn_gate_inp.weight", -2),
    "two_dimensional_experts": (dict(drop=["blk.0.ffn_gate_exps.weight"], add=[zeros("blk.0.ffn_gate_exps.weight", (256, 96 * 8), Q8)]), "blk.0.ffn_gate_exps.weight", -2),
    "experts_of_another_width": (dict(drop=["blk.0.ffn_up_exps.weight"], add=[zeros("blk.0.ffn_up_exps.weight", (256, 64, 8), Q8)]), "blk.0.ffn_up_exps.weight", -2),
    "down_experts_not_transposed": (dict(drop=["blk.1.ffn_down_exps.weight"], add=[zeros("blk.1.ffn_down_exps.weight", (256, 96, 8), Q8)]), "blk.1.ffn_down_exps.weight", -2),
    "seven_experts_in_a_tensor": (dict(drop=["blk.1.ffn_down_exps.weight"], add=[zeros("blk.1.ffn_down_exps.weight", (96, 256, 7), Q8)]), "blk.1.ffn_down_exps.weight", -2),
    "f16_experts": (dict(kw=dict(overrides={"ffn_gate_exps": "F16"})), "ffn_gate_exps.weight", -1),
    "bf16_experts": (dict(kw=dict(overrides={"ffn_down_exps": "BF16"})), "ffn_down_exps.weight", -1),
    "q4_0_experts": (dict(kw=dict(overrides={"ffn_up_exps": "Q4_0"})), "ffn_up_exps.weight", -1),
    "q5_k_experts": (dict(drop=["blk.0.ffn_gate_exps.weight"], add=[zeros("blk.0.ffn_gate_exps.weight", (256, 96, 8), G.GGML_Q5_K)]), "blk.0.ffn_gate_exps.weight", -1),
    "q4_k_experts_of_a_width_that_is_no_block": (dict(drop=["blk.0.ffn_down_exps.weight"], add=[zeros("blk.0.ffn_down_exps.weight", (96, 256, 8), Q4K)]),
                                                 "blk.0.ffn_down_exps.weight", -2, "not whole blocks of Q4_K"),
    "rows_beyond_the_staging_lds": (dict(kw=dict(experts=4, expert_inter=16384, moe_layers=(1,))), "blk.1.ffn_down_exps.weight", -2, "bytes of LDS"),
    "no_experts_named": (dict(kw=dict(extra_kvs=[G.kv_u32("qwen3moe.expert_count", 0)])), "qwen3moe.expert_count", -2),
    "257_experts_named": (dict(kw=dict(extra_kvs=[G.kv_u32("qwen3moe.expert_count", 257)])), "qwen3moe.expert_count", -2),
    "no_expert_used": (dict(kw=dict(extra_kvs=[G.kv_u32("qwen3moe.expert_used_count", 0)])), "qwen3moe.expert_used_count", -2),
    "more_used_than_there_are": (dict(kw=dict(extra_kvs=[G.kv_u32("qwen3moe.expert_used_count", 9)])), "qwen3moe.expert_used_count", -2),
    "17_of_32_used": (dict(kw=dict(experts=32, extra_kvs=[G.kv_u32("qwen3moe.expert_used_count", 17)])), "qwen3moe.expert_used_count", -2),
    "expert_keys_without_a_quartet": (dict(kw=dict(experts=None, extra_kvs=[G.kv_u32("qwen3moe.expert_count", 8), G.kv_u32("qwen3moe.expert_used_count", 2)])),
                                      "qwen3moe.expert_count", -9),
    "shared_expert_router": (dict(add=[zeros("blk.0.ffn_gate_inp_shexp.weight", (256,), F32)]), "blk.0.ffn_gate_inp_shexp.weight", -9),
    "shared_expert_gate": (dict(add=[zeros("blk.1.ffn_gate_shexp.weight", (256, 96), Q8)]), "blk.1.ffn_gate_shexp.weight", -9),
    "shared_expert_up": (dict(add=[zeros("blk.1.ffn_up_shexp.weight", (256, 96), Q8)]), "blk.1.ffn_up_shexp.weight", -9),
    "shared_expert_down": (dict(add=[zeros("blk.0.ffn_down_shexp.weight", (96, 256), Q8)]), "blk.0.ffn_down_shexp.weight", -9),
    "biased_routing": (dict(add=[zeros("blk.0.exp_probs_b.bias", (8,), F32)]), "blk.0.exp_probs_b.bias", -9),
    "tensor_parallelism": (dict(tp=(0, 2)), "ffn_gate_inp.weight", -2),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_the_load_refuses_ahead_of_the_device_and_names_the_tensor_or_key(what, tmp_path_factory, tmp_path):
    """the same status and message with and without a GPU"""
    how, named, status = REFUSALS[what][:3]
    path = model_file("moe8q8", tmp_path_factory, **how.get("kw", {}))
    if "drop" in how or "add" in how:
        path = rewrite(path, str(tmp_path / "refused.gguf"), how.get("drop", ()), how.get("add", ()))
    e = E.Engine()
    if "tp" in how:
        e.tp_configure(*how["tp"])
    with pytest.raises(_lib.NtkError) as ei:
        e.load(path, 128)
    print(what, "->", str(ei.value))
    assert ei.value.status == status and named in str(ei.value), str(ei.value)
    assert all(extra in str(ei.value) for extra in REFUSALS[what][3:]), str(ei.value)          # (what the message must say beside the name)
    assert e.moe() == -1                                             # nothing is loaded
    e.close()


def test_a_file_that_mixes_dense_and_routed_layers_is_described_layer_by_layer(tmp_path_factory):
    d = E.gguf_describe(model_file("half", tmp_path_factory))
    names = [t["name"] for t in d["tensors"]]
    assert d["moe_layers"] == 1 and "blk.0.ffn_gate.weight" in names and "blk.1.ffn_gate_inp.weight" in names and "blk.1.ffn_gate.weight" not in names
