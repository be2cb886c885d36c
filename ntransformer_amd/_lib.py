"""ctypes loader for the product library libntransformer_hip.so (built by ntransformer_amd/csrc/Makefile).

Fails loudly: there is NO CPU fallback anywhere in this package.  If the HIP extension is missing the
import raises; if there is no GPU every operator returns NTK_E_NODEVICE and `check()` raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NTK_LIB_PATH") or os.path.join(_HERE, "libntransformer_hip.so")   # (override: A/B of two builds)

NTK_OK = 0
_STATUS = {0: "ok", -1: "unsupported dtype", -2: "bad shape", -3: "HIP launch/runtime error", -4: "misaligned pointer",
           -5: "null pointer", -6: "no usable GPU", -7: "out of memory", -8: "I/O error", -9: "malformed GGUF"}


class NtkError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        super().__init__("ntk status %d (%s)%s" % (status, _STATUS.get(status, "?"), (": " + what) if what else ""))


def check(status: int, what: str = "") -> None:
    if status != NTK_OK:
        raise NtkError(status, what)


class KvBatch(C.Structure):   # ntk_kv_batch: the rows' cache base pointers of one layer
    _fields_ = [("k", C.c_void_p * 16), ("v", C.c_void_p * 16)]


class KvSegments(C.Structure):   # ntk_kv_segments: the segments of a packed prompt pass and their caches of one layer
    _fields_ = [("n_seg", C.c_int), ("row0", C.c_int * 16), ("n_rows", C.c_int * 16), ("start_pos", C.c_int * 16), ("k", C.c_void_p * 16),
                ("v", C.c_void_p * 16)]


class SampleRows(C.Structure):   # ntk_sample_rows: the per-row settings of ntk_sample_rows_top_k
    _fields_ = [("temperature", C.c_float * 16), ("top_p", C.c_float * 16), ("repeat_penalty", C.c_float * 16), ("r", C.c_float * 16),
                ("top_k", C.c_int * 16), ("n_recent", C.c_int * 16)]


class GemvSeg(C.Structure):
    _fields_ = [("W", C.c_void_p), ("y", C.c_void_p), ("rows", C.c_int), ("dtype", C.c_int)]


class GemmPartials(C.Structure):   # ntk_gemm_partials (include/ntk_engine.h)
    _fields_ = [("part", C.c_void_p * 3), ("y", C.c_void_p * 3), ("rows", C.c_int * 3), ("nseg", C.c_int), ("n_tokens", C.c_int), ("nsplit", C.c_int)]


class GemmDesc(C.Structure):   # ntk_gemm_desc (include/ntk_engine.h)
    _fields_ = [("segs", C.POINTER(GemvSeg)), ("nseg", C.c_int), ("X", C.c_void_p), ("n_tokens", C.c_int), ("in_features", C.c_int), ("resid", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("reuse_x", C.c_int), ("row_max", C.c_void_p),
                ("partials", C.POINTER(GemmPartials)), ("weights_repacked", C.c_int), ("full_form", C.c_int)]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    sig = {
        "ntk_abi_version": (i, []),
        "ntk_status_string": (C.c_char_p, [i]),
        "ntk_row_bytes": (sz, [i, C.c_int64]),
        "ntk_device_count": (i, []),
        "ntk_device_init": (i, [i]),
        "ntk_device_name": (i, [C.c_char_p, sz]),
        "ntk_device_mem_info": (i, [C.POINTER(sz), C.POINTER(sz)]),
        "ntk_stream": (vp, [i]),
        "ntk_stream_synchronize": (i, [vp]),
        "ntk_device_synchronize": (i, []),
        "ntk_event_create": (vp, []),
        "ntk_event_destroy": (i, [vp]),
        "ntk_event_record": (i, [vp, vp]),
        "ntk_event_synchronize": (i, [vp]),
        "ntk_event_elapsed_ms": (i, [vp, vp, C.POINTER(f)]),
        "nt_hip_malloc": (vp, [sz]), "nt_hip_free": (None, [vp]),
        "nt_hip_memcpy_h2d": (None, [vp, vp, sz]), "nt_hip_memcpy_d2h": (None, [vp, vp, sz]),
        "nt_hip_memcpy_d2d": (None, [vp, vp, sz]), "nt_hip_memset": (None, [vp, i, sz]),
        "nt_hip_malloc_host": (vp, [sz]), "nt_hip_free_host": (None, [vp]),
        "ntk_memcpy_h2d_async": (i, [vp, vp, sz, vp]), "ntk_memcpy_d2h_async": (i, [vp, vp, sz, vp]),
        "nt_cuda_malloc": (vp, [sz]), "nt_cuda_free": (None, [vp]),
        "nt_cuda_memcpy_h2d": (None, [vp, vp, sz]), "nt_cuda_memcpy_d2h": (None, [vp, vp, sz]),
        "nt_cuda_memcpy_d2d": (None, [vp, vp, sz]), "nt_cuda_memset": (None, [vp, i, sz]),
        "nt_cuda_malloc_host": (vp, [sz]), "nt_cuda_free_host": (None, [vp]),
        "ntk_rmsnorm": (i, [vp, vp, vp, i, i, f, vp]),
        "ntk_rmsnorm_f16": (i, [vp, vp, vp, i, i, f, vp]),
        "ntk_rope": (i, [vp, vp, vp, i, i, i, i, i, f, f, i, vp]),
        "ntk_softmax": (i, [vp, vp, i, i, vp]),
        "ntk_masked_softmax": (i, [vp, vp, vp, i, i, vp]),
        "ntk_gemv": (i, [vp, vp, vp, i, i, i, vp]),
        "ntk_gemv_add": (i, [vp, vp, vp, i, i, i, vp]),
        "ntk_gemm_f32": (i, [vp, vp, vp, i, i, i, vp]),
        "ntk_silu_mul": (i, [vp, vp, vp, i, vp]),
        "ntk_rmsnorm_rowmax": (i, [vp, vp, vp, i, i, f, vp, vp, vp]),
        "ntk_rope_kv_store": (i, [vp, vp, vp, vp, i, i, i, i, f, f, i, vp, vp, i, i, vp]),
        "ntk_silu_mul_rowmax": (i, [vp, vp, vp, i, i, vp, vp]),
        "ntk_add_bias": (i, [vp, vp, i, vp]),
        "ntk_attention_decode": (i, [vp, vp, vp, vp, i, i, i, i, i, f, vp]),
        "ntk_attention_prefill": (i, [vp, vp, vp, vp, i, i, i, i, i, i, f, vp]),
        "ntk_copy_to_kv_cache": (i, [vp, vp, vp, vp, i, i, i, i, i, vp]),
        "ntk_add": (i, [vp, vp, vp, i, vp]),
        "ntk_add_inplace": (i, [vp, vp, i, vp]),
        "ntk_copy": (i, [vp, vp, i, vp]),
        "ntk_cosine_similarity": (i, [vp, vp, vp, i, vp]),
        "ntk_gemv_fused": (i, [C.POINTER(GemvSeg), i, vp, i, vp, f, vp, i, vp]),
        "ntk_debug_gemv_fused_form": (i, [C.POINTER(GemvSeg), i, vp, i, vp, f, vp, i, i, vp]),
        "ntk_q8l_bytes": (sz, [i, i]),
        "ntk_q8l_pack": (i, [vp, vp, i, i, vp]),
        "ntk_q8l_unpack": (i, [vp, vp, i, i, vp]),
        "ntk_rp_bytes": (sz, [i, i, i]),
        "ntk_rp_pack": (i, [vp, vp, i, i, i, vp]),
        "ntk_rp_dequant": (i, [vp, vp, i, i, i, vp]),
        "ntk_rp_unpack": (i, [vp, vp, i, i, i, vp]),
        "ntk_gemv_rp": (i, [vp, vp, vp, i, i, i, vp]),
        "ntk_gemv_rp_fused": (i, [C.POINTER(GemvSeg), i, vp, i, vp, f, vp, i, vp]),
        "ntk_decode_arena_acquire": (i, []), "ntk_decode_arena_release": (None, [i]),
        "ntk_decode_arena_slot": (vp, [i]), "ntk_debug_gemv_static_x": (i, []),
        "ntk_debug_rp_prologue": (i, [vp, vp, vp, f, i, i, i, vp]),
        "ntk_debug_mfma_i8_probe": (i, [vp, vp, vp, vp]),
        "ntk_gemm_quant": (i, [vp, vp, vp, i, i, i, i, vp, vp]),
        "ntk_gemm_dense16_workspace_bytes": (sz, [i, i, i]),
        "ntk_gemm_dense16": (i, [C.POINTER(GemmDesc), vp]),
        "ntk_attention_decode_split": (i, [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, f, f, f, i, vp, vp]),
        "ntk_attention_split_scratch_bytes": (C.c_size_t, [i, i, i]),
        "ntk_attention_split_scratch_init": (i, [vp, i, vp]),
        "ntk_attention_decode_split_merged": (i, [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, f, f, f, i, vp, vp]),
        "ntk_attention_decode_fused": (i, [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, f, f, f, vp]),
        "ntk_attention_decode_batch": (i, [vp, vp, vp, vp, vp, vp, i, vp, i, i, i, i, f, f, f, i, vp, vp]),
        "ntk_kv_segments_validate": (i, [vp, i, i]),
        "ntk_rope_kv_store_segments": (i, [vp, vp, vp, vp, i, i, i, f, f, i, i, vp]),
        "ntk_attention_prefill_segments": (i, [vp, vp, vp, i, i, i, i, f, vp]),
        "ntk_rope_tab": (i, [vp, vp, vp, i, i, i, i, i, f, f, i, vp, vp]),
        "ntk_rope_kv_store_tab": (i, [vp, vp, vp, vp, i, i, i, i, f, f, i, vp, vp, i, i, vp, vp]),
        "ntk_rope_kv_store_segments_tab": (i, [vp, vp, vp, vp, i, i, i, f, f, i, i, vp, vp]),
        "ntk_rope_kv_store_q8_tab": (i, [vp, vp, vp, vp, i, i, i, i, f, f, i, vp, vp, i, i, vp, vp]),
        "ntk_kv_q8_cache_bytes": (C.c_size_t, [i, i, i]),
        "ntk_kv_store_q8": (i, [vp, vp, vp, vp, i, i, i, i, i, vp]),
        "ntk_rope_kv_store_q8": (i, [vp, vp, vp, vp, i, i, i, i, f, f, i, vp, vp, i, i, vp]),
        "ntk_attention_decode_q8": (i, [vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, f, f, f, i, vp, vp]),
        "ntk_kv_dequant_q8_f16": (i, [vp, vp, vp, vp, i, i, i, i, vp]),
        "ntk_attention_decode_q8_batch": (i, [vp, vp, vp, vp, vp, vp, i, vp, i, i, i, i, f, f, f, i, vp, vp]),
        "ntk_kv_shift": (i, [vp, vp, i, i, i, i, i, i, i, vp, f, f, i, vp]),
        "ntk_kv_shift_q8": (i, [vp, vp, i, i, i, i, i, i, i, vp, f, f, i, vp]),
        "ntk_embed_rows": (i, [vp, vp, vp, i, i, i, vp]),
        "ntk_argmax": (i, [vp, i, vp, vp, vp, vp]),
        "ntk_logprob_rows": (i, [vp, i, i, i, vp, vp, vp, vp]),
        "ntk_sample_rows_scratch_bytes": (C.c_size_t, [i, i]),
        "ntk_sample_rows_top_k": (i, [vp, i, i, i, vp, i, C.POINTER(SampleRows), vp, vp, vp, vp]),
        "ntk_advance_pos": (i, [vp, vp]),
        "ntk_qkv_bias": (i, [vp, vp, vp, vp, vp, vp, i, i, i, vp]),
        "ntk_qk_norm": (i, [vp, vp, vp, vp, i, i, i, i, f, vp]),
        "ntk_moe_workspace_layout": (sz, [i, i, i, i, i, C.POINTER(sz)]),
        "ntk_moe_workspace_bytes": (sz, [i, i, i, i, i]),
        "ntk_moe_lds_bytes": (sz, [i, i, i]),
        "ntk_moe_route": (i, [vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp]),
        "ntk_moe_gate_up": (i, [vp, vp, vp, i, vp, i, vp, vp, i, i, i, i, i, vp]),
        "ntk_moe_down": (i, [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, vp]),
        "ntk_moe_gemm_scratch_bytes": (sz, [i, i, i, i, i]),
        "ntk_moe_gemm_gate_up": (i, [vp, vp, vp, i, vp, i, vp, vp, vp, sz, i, i, i, i, i, vp]),
        "ntk_moe_gemm_down": (i, [vp, vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, i, vp]),
        "ntk_debug_sclk": (i, [vp, vp]),
        "ntk_debug_sclk_begin": (i, [vp, vp, vp]),
        "ntk_debug_sclk_end": (i, [vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError here = the .so does not export what include/ntk.h declares
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTS_NTK_H = None  # filled by tests from include/ntk.h
