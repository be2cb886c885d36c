"""Host-side logic of the product library, on the CPU (no GPU needed): the C ABI loads and exports every symbol
the headers declare, and the GGUF reader / tokenizer / sampler agree with goldens produced by the reference's
own unmodified classes (oracle/_ref/ref_host, tools/make_golden.py -> tests/golden/host_logic.json)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from ntransformer_amd import _lib
from ntransformer_amd import gguf as G


class GenParams(C.Structure):
    _fields_ = [("max_tokens", C.c_int), ("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float),
                ("repeat_penalty", C.c_float), ("repeat_window", C.c_int), ("seed", C.c_uint64), ("stop_at_eos", C.c_int)]


def declared_functions(header, where="include"):
    src = open(os.path.join(ROOT, where, header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b((?:ntk|nt)_[a-z0-9_]+)\s*\(", src)) - {"nt_engine_t", "nt_tokenizer_t"})


@pytest.mark.parametrize("header", ["ntk.h", "ntk_engine.h", "ntransformer.h"])
def test_library_exports_every_declared_symbol(header):
    L = _lib.lib()
    names = declared_functions(header)
    assert len(names) > 15
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_library_exports_nothing_but_the_headers():
    """-fvisibility=hidden: the dynamic symbol table of the shipping library holds the C functions the three headers declare and nothing else of ours
    (hipcc's kernel stubs / __hip_* registration symbols aside)."""
    import shutil
    import subprocess
    if not shutil.which("nm"):
        pytest.skip("binutils' nm is not installed")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    have = {l.split()[-1] for l in out.splitlines() if " T " in l}
    ours = {n for n in have if n.startswith(("ntk_", "nt_"))}
    declared = set(declared_functions("ntk.h")) | set(declared_functions("ntk_engine.h")) | set(declared_functions("ntransformer.h"))
    assert not (ours - declared), sorted(ours - declared)


def test_reference_surface_header_is_the_reference_surface():
    """include/ntk.h after the round-6 split: one ntk_<op> per launcher of reference src/cuda/kernels.h:14-71 (17 names) + the runtime of
    src/core/device.h:36-88 -- none of the engine's fused / repack / prompt / debug entry points."""
    names = set(declared_functions("ntk.h"))
    launchers = {"ntk_rmsnorm", "ntk_rmsnorm_f16", "ntk_rope", "ntk_softmax", "ntk_masked_softmax", "ntk_gemv", "ntk_gemv_add", "ntk_gemm_f32", "ntk_silu_mul",
                 "ntk_add_bias", "ntk_attention_decode", "ntk_attention_prefill", "ntk_copy_to_kv_cache", "ntk_add", "ntk_add_inplace", "ntk_copy",
                 "ntk_cosine_similarity"}
    assert launchers <= names and len(launchers) == 17
    rest = names - launchers
    assert all(n.startswith(("nt_hip_", "nt_cuda_", "ntk_device_", "ntk_stream", "ntk_event_", "ntk_memcpy_")) or n in ("ntk_abi_version", "ntk_status_string", "ntk_row_bytes")
               for n in rest), sorted(rest)
    assert not [n for n in names if "debug" in n or "fused" in n or "_rp" in n or "gemm_quant" in n]


RETIRED_ENTRY_POINTS = ["ntk_persistent_plan_create", "ntk_persistent_launch", "ntk_persistent_error", "ntk_layer_engine_plan_create",
                        "ntk_layer_engine_launch", "ntk_layer_engine_error", "ntk_attention_gemv_fused", "nt_engine_persistent_plan",
                        "nt_engine_persistent_kind"]


def test_retired_experiments_are_not_in_the_library():
    """The persistent token kernel, the layer engine and attention inside the Wo launch all measured slower than the launch path
    (profiles/NEGATIVE_RESULTS.md) and were removed with their engine hooks: the shipping library exports none of their entry points."""
    L = _lib.lib()
    assert not [n for n in RETIRED_ENTRY_POINTS if hasattr(L, n)]


def test_prompt_gemm_workspace_covers_its_layout():
    """ntk_gemm_quant_workspace_bytes (no GPU needed) against the layout csrc/gemm_f16.hip describes: per 64-token chunk (16 of them) the
    FP16 planes of in/32 + 1 steps (8 KB each) and the step sums in WHOLE units of 8 steps up to step in/32 + 7 (2 KB each: the
    pre-pass writes a full unit of zeros behind the last step -- a 128-column remainder used to overrun the area), then the tokens'
    scales (2 x 1024 floats) and the partial sums of K splits (32 chunk x split products for matrices of <= 8192 rows, 16 above)."""
    L = _lib.lib()
    L.ntk_gemm_quant_workspace_bytes.restype = C.c_size_t
    for in_f in (128, 256, 384, 640, 4096, 14336, 28672):
        for out_f in (16, 4096, 8192, 8208, 28672):
            steps = in_f // 32
            chunk = (steps + 1) * 8192 + ((steps + 8 + 7) // 8) * 2048
            need = 16 * chunk + 2 * 1024 * 4 + (32 if out_f <= 8192 else 16) * 64 * out_f * 4
            got = L.ntk_gemm_quant_workspace_bytes(C.c_int(in_f), C.c_int(out_f))
            assert need <= got <= need + 16 * 256 + 4096, (in_f, out_f, need, got)


def test_abi_basics_without_gpu():
    L = _lib.lib()
    assert L.ntk_abi_version() == 1
    # nt::DType numeric contract (reference src/core/types.h:24-35) through ntk_row_bytes (types.h:37-88)
    assert L.ntk_row_bytes(G.DT_Q8_0, 4096) == 4352
    assert L.ntk_row_bytes(G.DT_Q4_0, 1024) == 576          # reference tests/test_tensor.cpp:131-134
    assert L.ntk_row_bytes(G.DT_Q4_K, 4096) == 2304
    assert L.ntk_row_bytes(G.DT_Q5_K, 4096) == 2816
    assert L.ntk_row_bytes(G.DT_Q6_K, 4096) == 3360
    assert L.ntk_row_bytes(G.DT_F16, 10) == 20 and L.ntk_row_bytes(G.DT_F32, 10) == 40
    assert L.ntk_row_bytes(G.DT_Q8_0, 100) == 0
    assert L.ntk_status_string(-1) == b"unsupported dtype"


def test_null_engine_is_tolerated():
    L = _lib.lib()
    L.nt_engine_vocab_size.argtypes = [C.c_void_p]
    L.nt_engine_generate.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_float, C.c_int, C.c_float]
    L.nt_engine_generate.restype = C.c_void_p
    assert L.nt_engine_vocab_size(None) == -1
    assert L.nt_engine_generate(None, b"x", 4, 0.0, 1, 1.0) is None
    L.nt_engine_create.restype = C.c_void_p
    L.nt_engine_destroy.argtypes = [C.c_void_p]
    e = L.nt_engine_create()
    assert e
    assert L.nt_engine_vocab_size(e) == -1          # nothing loaded
    L.nt_engine_load.argtypes = [C.c_void_p, C.c_char_p]
    assert L.nt_engine_load(e, b"/nonexistent.gguf") != 0
    L.nt_engine_destroy(e)


def describe(path):
    L = _lib.lib()
    buf = C.create_string_buffer(4 << 20)
    n = L.nt_gguf_describe(path.encode(), buf, len(buf))
    assert n > 0, n
    return json.loads(buf.value.decode())


@pytest.mark.parametrize("name", ["tiny_q8_0", "tiny_q4_k_m", "tiny_mixed"])
def test_cpp_gguf_reader_matches_python_reader(name):
    path = os.path.join(GOLDEN, name + ".gguf")
    d = describe(path)
    f = G.read_gguf(path)
    assert d["data_offset"] == f.data_offset and d["version"] == 3
    assert (d["hidden_size"], d["intermediate_size"], d["n_layers"], d["n_heads"], d["n_kv_heads"]) == (256, 512, 2, 4, 2)
    assert d["head_dim"] == 64 and d["vocab_size"] == 512 and d["bos"] == 256 and d["eos"] == 257
    assert abs(d["rope_theta"] - 500000.0) < 1e-3 and abs(d["norm_eps"] - 1e-5) < 1e-10
    assert len(d["tensors"]) == len(f.tensors)
    for t in d["tensors"]:
        ti = f.tensors[t["name"]]
        assert tuple(t["dims"]) == ti.dims and t["ggml_type"] == ti.ggml_type
        assert t["offset"] == ti.offset and t["nbytes"] == ti.nbytes and t["dtype"] == G.GGML_TO_DT[ti.ggml_type]


def test_gguf_reader_rejects_garbage(tmp_path):
    L = _lib.lib()
    p = tmp_path / "bad.gguf"
    p.write_bytes(b"NOPE" + b"\0" * 64)
    assert L.nt_gguf_describe(str(p).encode(), None, 0) == -9          # NTK_E_FORMAT
    good = open(os.path.join(GOLDEN, "tiny_q8_0.gguf"), "rb").read()
    p.write_bytes(good[:5000])                                          # truncated inside the metadata
    assert L.nt_gguf_describe(str(p).encode(), None, 0) == -9
    p.write_bytes(good[:200000])                                        # tensors run past the end of the file
    assert L.nt_gguf_describe(str(p).encode(), None, 0) == -9
    assert L.nt_gguf_describe(b"/nonexistent", None, 0) == -8           # NTK_E_IO


HOST = json.load(open(os.path.join(GOLDEN, "host_logic.json")))


@pytest.mark.parametrize("vocab", sorted(HOST["tokenizer"]))
def test_tokenizer_matches_reference(vocab):
    L = _lib.lib()
    L.nt_tokenizer_open.restype = C.c_void_p
    L.nt_tokenizer_open.argtypes = [C.c_char_p]
    L.nt_tokenizer_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    L.nt_tokenizer_decode.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int]
    L.nt_tokenizer_close.argtypes = [C.c_void_p]
    L.nt_tokenizer_is_gpt2.argtypes = [C.c_void_p]
    t = L.nt_tokenizer_open(os.path.join(GOLDEN, vocab).encode())
    assert t
    assert L.nt_tokenizer_is_gpt2(t) == (0 if "spm" in vocab else 1)
    for case in HOST["tokenizer"][vocab]:
        raw = case["text"].encode("utf-8")
        out = (C.c_int * 256)()
        n = L.nt_tokenizer_encode(t, raw, len(raw), 1, out, 256)
        assert list(out[:n]) == case["ids"], case["text"]
        buf = C.create_string_buffer(1024)
        m = L.nt_tokenizer_decode(t, out, n, buf, 1024)
        assert buf.raw[:m].hex() == case["detok_hex"], case["text"]
    L.nt_tokenizer_close(t)


@pytest.mark.parametrize("idx", range(len(HOST["sampler"])))
def test_sampler_matches_reference(idx):
    L = _lib.lib()
    case = HOST["sampler"][idx]
    logits = np.fromfile(os.path.join(GOLDEN, "sampler_logits.f32"), np.float32)
    c = case["cfg"]
    p = GenParams(0, c["temperature"], c["top_k"], c["top_p"], c["repeat_penalty"], c["repeat_window"], c["seed"], 1)
    recent = (C.c_int * len(case["recent"]))(*case["recent"])
    out = (C.c_int * len(case["draws"]))()
    L.nt_sampler_draw.argtypes = [C.c_void_p, C.c_int, C.POINTER(GenParams), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    n = L.nt_sampler_draw(logits.ctypes.data_as(C.c_void_p), logits.size, C.byref(p), recent, len(case["recent"]), len(case["draws"]), out)
    assert n == len(case["draws"])
    assert list(out) == case["draws"]


def test_bench_launch_model_recovers_fixed_cost_and_rate():
    """bench.py's roofline.launch_model (the round-5 review's item 3: t = fixed + bytes / rate, so the GEMV launches' roofline fraction can be re-derived from the
    bench line alone): launch durations made from a known (fixed, rate) over the real per-kind bytes of the 8B Q8_0 layer come back exactly, and the per-kind
    bytes sum to the GEMV bytes of a token."""
    import bench
    from ntransformer_amd import engine as E
    spec = E.synth_spec("8b", "Q8_0")
    by = bench._gemv_bytes_by_kind(spec, "Q8_0")
    assert abs(sum(b * n for b, n in by.values()) - bench._gemv_bytes_per_token(spec, "Q8_0")) < 1.0
    kinds = {k: {"avg_us": 3.0 + b / 6.5e6, "calls": n} for k, (b, n) in by.items()}
    m = bench._launch_model(spec, "Q8_0", kinds)
    assert abs(m["fixed_us"] - 3.0) < 0.02 and abs(m["stream_TBs"] - 6.5) < 0.02
    assert m["per_launch"]["wo"][2] == 32 and m["per_launch"]["lm_head"][2] == 1
    assert bench._launch_model(spec, "Q8_0", None) is None
