"""Python mirror of the reference's operator surface (reference src/cuda/kernels.h:14-71) over the C ABI in
include/ntk.h: same function names (`launch_*`), same argument order and meaning, device pointers in and out.
`DeviceBuffer` is a minimal stand-in for the reference's Tensor on Device::CUDA (reference src/core/tensor.h).
Everything here runs on the GPU through libntransformer_hip.so; nothing falls back to the CPU."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import GemvSeg, check


class DeviceBuffer:
    """Owned device allocation with numpy upload/download (blocking copies, like nt_cuda_memcpy_*)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = _lib.lib().nt_hip_malloc(max(self.nbytes, 1))
        if not self.ptr:
            raise _lib.NtkError(-7, "hipMalloc(%d)" % nbytes)

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        if a.nbytes:
            _lib.lib().nt_hip_memcpy_h2d(b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes)
        return b

    @classmethod
    def zeros(cls, nbytes: int) -> "DeviceBuffer":
        b = cls(nbytes)
        _lib.lib().nt_hip_memset(b.ptr, 0, nbytes)
        return b

    def upload(self, a: np.ndarray, offset: int = 0) -> None:
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        _lib.lib().nt_hip_memcpy_h2d(self.ptr + offset, a.ctypes.data_as(C.c_void_p), a.nbytes)

    def numpy(self, dtype=np.float32, count: Optional[int] = None, offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        n = (self.nbytes - offset) // dt.itemsize if count is None else count
        out = np.empty(n, dt)
        # the blocking copy runs on the NULL stream, which does not order against the library's non-blocking
        # compute stream (same as the reference: cudaMemcpy vs cudaStreamNonBlocking) -> drain it first
        check(_lib.lib().ntk_stream_synchronize(None), "stream sync")
        if n:
            _lib.lib().nt_hip_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr + offset, out.nbytes)
        return out

    def at(self, byte_offset: int) -> int:
        return self.ptr + byte_offset

    def free(self) -> None:
        if self.ptr:
            _lib.lib().nt_hip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _p(x) -> Optional[int]:
    if x is None:
        return None
    return x.ptr if isinstance(x, DeviceBuffer) else int(x)


def init(device_id: int = 0) -> None:
    check(_lib.lib().ntk_device_init(device_id), "ntk_device_init")


def synchronize(stream=None) -> None:
    check(_lib.lib().ntk_stream_synchronize(stream), "stream sync")


# ---- the 17 launchers of kernels.h, 1:1 ---------------------------------------------------------------
def launch_rmsnorm(output, input, weight, batch_size, hidden_size, eps, stream=None):
    check(_lib.lib().ntk_rmsnorm(_p(output), _p(input), _p(weight), batch_size, hidden_size, eps, stream), "rmsnorm")


def launch_rmsnorm_f16(output, input, weight, batch_size, hidden_size, eps, stream=None):
    check(_lib.lib().ntk_rmsnorm_f16(_p(output), _p(input), _p(weight), batch_size, hidden_size, eps, stream), "rmsnorm_f16")


def launch_rope(q, k, positions, batch_size, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale,
                interleaved, stream=None):
    check(_lib.lib().ntk_rope(_p(q), _p(k), _p(positions), batch_size, seq_len, n_heads, n_kv_heads, head_dim,
                              theta_base, freq_scale, int(bool(interleaved)), stream), "rope")


def rope_tab(q, k, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, inv_freq=None, stream=None):
    """ntk_rope_tab: ntk_rope with the per-pair frequencies from the device table inv_freq [head_dim / 2] (None: the in-kernel frequency)"""
    check(_lib.lib().ntk_rope_tab(_p(q), _p(k), _p(positions), 1, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale,
                                  int(bool(interleaved)), _p(inv_freq), stream), "rope_tab")


def launch_softmax(output, input, rows, cols, stream=None):
    check(_lib.lib().ntk_softmax(_p(output), _p(input), rows, cols, stream), "softmax")


def launch_masked_softmax(output, input, mask, rows, cols, stream=None):
    check(_lib.lib().ntk_masked_softmax(_p(output), _p(input), _p(mask), rows, cols, stream), "masked_softmax")


def launch_gemv(y, W, x, out_features, in_features, weight_dtype, stream=None):
    check(_lib.lib().ntk_gemv(_p(y), _p(W), _p(x), out_features, in_features, int(weight_dtype), stream), "gemv")


def launch_gemv_add(y, W, x, out_features, in_features, weight_dtype, stream=None):
    check(_lib.lib().ntk_gemv_add(_p(y), _p(W), _p(x), out_features, in_features, int(weight_dtype), stream), "gemv_add")


def launch_gemm_f32(Cm, A, B, M, N, K, stream=None):
    check(_lib.lib().ntk_gemm_f32(_p(Cm), _p(A), _p(B), M, N, K, stream), "gemm_f32")


def launch_silu_mul(output, gate, up, size, stream=None):
    check(_lib.lib().ntk_silu_mul(_p(output), _p(gate), _p(up), size, stream), "silu_mul")


def launch_add_bias(y, bias, size, stream=None):
    check(_lib.lib().ntk_add_bias(_p(y), _p(bias), size, stream), "add_bias")


def launch_attention_decode(output, q, k_cache, v_cache, seq_len, n_heads, n_kv_heads, head_dim, max_seq, scale, stream=None):
    check(_lib.lib().ntk_attention_decode(_p(output), _p(q), _p(k_cache), _p(v_cache), seq_len, n_heads, n_kv_heads,
                                          head_dim, max_seq, scale, stream), "attention_decode")


def launch_attention_prefill(output, Q, k_cache, v_cache, seq_len, start_pos, n_heads, n_kv_heads, head_dim, max_seq,
                             scale, stream=None):
    check(_lib.lib().ntk_attention_prefill(_p(output), _p(Q), _p(k_cache), _p(v_cache), seq_len, start_pos, n_heads,
                                           n_kv_heads, head_dim, max_seq, scale, stream), "attention_prefill")


def launch_copy_to_kv_cache(k_cache, v_cache, k, v, seq_len, n_kv_heads, head_dim, start_pos, max_seq, stream=None):
    check(_lib.lib().ntk_copy_to_kv_cache(_p(k_cache), _p(v_cache), _p(k), _p(v), seq_len, n_kv_heads, head_dim,
                                          start_pos, max_seq, stream), "copy_to_kv_cache")


def launch_add(out, a, b, size, stream=None):
    check(_lib.lib().ntk_add(_p(out), _p(a), _p(b), size, stream), "add")


def launch_add_inplace(a, b, size, stream=None):
    check(_lib.lib().ntk_add_inplace(_p(a), _p(b), size, stream), "add_inplace")


def launch_copy(dst, src, size, stream=None):
    check(_lib.lib().ntk_copy(_p(dst), _p(src), size, stream), "copy")


def launch_cosine_similarity(result, a, b, size, stream=None):
    check(_lib.lib().ntk_cosine_similarity(_p(result), _p(a), _p(b), size, stream), "cosine_similarity")


# ---- engine-level fused operators -----------------------------------------------------------------------
def gemv_fused(segs: Sequence[tuple], x, in_features, norm_w=None, eps=0.0, resid=None, silu_pair=False, stream=None,
               integer_activations=None):
    """segs: [(W, y, rows, dtype), ...] (<= 3, same dtype).  integer_activations (True / False): ntk_debug_gemv_fused_form, the
    activation form of the Q4_K / Q6_K launches chosen by the call instead of by the library's size rule."""
    arr = (GemvSeg * len(segs))()
    for i, (W, y, rows, dt) in enumerate(segs):
        arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = _p(W), _p(y), rows, int(dt)
    if integer_activations is None:
        check(_lib.lib().ntk_gemv_fused(arr, len(segs), _p(x), in_features, _p(norm_w), eps, _p(resid), int(silu_pair),
                                        stream), "gemv_fused")
    else:
        check(_lib.lib().ntk_debug_gemv_fused_form(arr, len(segs), _p(x), in_features, _p(norm_w), eps, _p(resid), int(silu_pair),
                                                   1 if integer_activations else 0, stream), "gemv_fused_form")


def qkv_bias(q, k, v, bq, bk, bv, n_rows, q_dim, kv_dim, stream=None):
    """ntk_qkv_bias: q [n_rows][q_dim] += bq, k / v [n_rows][kv_dim] += bk / bv, in place, one launch; a bias of None leaves its buffer untouched"""
    check(_lib.lib().ntk_qkv_bias(_p(q), _p(k), _p(v), _p(bq), _p(bk), _p(bv), n_rows, q_dim, kv_dim, stream), "qkv_bias")


def qk_norm(q, k, wq, wk, n_rows, n_heads, n_kv_heads, head_dim, eps, stream=None):
    """ntk_qk_norm: RMSNorm of every head of q [n_rows][n_heads * head_dim] (weights wq[head_dim]) and of k [n_rows][n_kv_heads * head_dim] (wk), in place, one launch"""
    check(_lib.lib().ntk_qk_norm(_p(q), _p(k), _p(wq), _p(wk), n_rows, n_heads, n_kv_heads, head_dim, eps, stream), "qk_norm")


MOE_WS_SECTIONS = ("xn", "act", "part", "w", "ids", "pairs", "offsets")   # NTK_MOE_WS_*, in order


def moe_workspace_layout(T, E, K, inter, hidden):
    """ntk_moe_workspace_layout: ({section: byte offset}, total bytes) of one routed-FFN workspace for passes of up to T rows; (None, 0) out of range"""
    off = (C.c_size_t * len(MOE_WS_SECTIONS))()
    total = int(_lib.lib().ntk_moe_workspace_layout(T, E, K, inter, hidden, off))
    return (dict(zip(MOE_WS_SECTIONS, [int(o) for o in off])) if total else None), total


def moe_workspace_bytes(T, E, K, inter, hidden) -> int:
    return int(_lib.lib().ntk_moe_workspace_bytes(T, E, K, inter, hidden))


def moe_route(xn, router, T, hidden, E, K, ids, w, offsets, pairs, logits=None, stream=None):
    """ntk_moe_route: the K largest router logits of each of the T rows (ids int32 [T][K], descending, ties to the lower expert), w = softmax over them,
    and the expert-major work list offsets [E + 1] / pairs [T K]; logits (optional): the raw [T][E] logits"""
    check(_lib.lib().ntk_moe_route(_p(xn), _p(router), T, hidden, E, K, _p(ids), _p(w), _p(offsets), _p(pairs), _p(logits), stream), "moe_route")


def moe_gate_up(act, xn, w_gate, dt_gate, w_up, dt_up, offsets, pairs, T, hidden, inter, E, K, stream=None):
    """ntk_moe_gate_up: act [T K][inter] = SiLU(Wg[e] . xn[t]) x (Wu[e] . xn[t]) for every pair of the work list"""
    check(_lib.lib().ntk_moe_gate_up(_p(act), _p(xn), _p(w_gate), int(dt_gate), _p(w_up), int(dt_up), _p(offsets), _p(pairs), T, hidden, inter, E, K, stream),
          "moe_gate_up")


def moe_down(y, resid, act, w_down, dt_down, ids, w, offsets, pairs, part, T, hidden, inter, E, K, stream=None):
    """ntk_moe_down: y [T][hidden] = resid + sum over k ascending of w[t][k] x (Wd[e_k] . act[t K + k]); y may be resid; part: T K hidden floats of scratch"""
    check(_lib.lib().ntk_moe_down(_p(y), _p(resid), _p(act), _p(w_down), int(dt_down), _p(ids), _p(w), _p(offsets), _p(pairs), _p(part), T, hidden, inter, E, K,
                                  stream), "moe_down")


def moe_gemm_scratch_bytes(T, E, K, inter, hidden) -> int:
    """ntk_moe_gemm_scratch_bytes: the scratch ntk_moe_gemm_gate_up wants for a pass of up to T rows (may be 0; 0 also for counts out of range)"""
    return int(_lib.lib().ntk_moe_gemm_scratch_bytes(T, E, K, inter, hidden))


def moe_gemm_gate_up(act, xn, w_gate, dt_gate, w_up, dt_up, offsets, pairs, T, hidden, inter, E, K, scratch=None, scratch_bytes=0, stream=None):
    """ntk_moe_gemm_gate_up: moe_gate_up's result on the matrix cores (the grouped prompt GEMM); scratch: at least moe_gemm_scratch_bytes bytes, None for 0"""
    check(_lib.lib().ntk_moe_gemm_gate_up(_p(act), _p(xn), _p(w_gate), int(dt_gate), _p(w_up), int(dt_up), _p(offsets), _p(pairs), _p(scratch),
                                          int(scratch_bytes), T, hidden, inter, E, K, stream), "moe_gemm_gate_up")


def moe_gemm_down(y, resid, act, w_down, dt_down, ids, w, offsets, pairs, part, T, hidden, inter, E, K, stream=None):
    """ntk_moe_gemm_down: moe_down's result on the matrix cores, the same combine over part; y may be resid"""
    check(_lib.lib().ntk_moe_gemm_down(_p(y), _p(resid), _p(act), _p(w_down), int(dt_down), _p(ids), _p(w), _p(offsets), _p(pairs), _p(part), T, hidden,
                                       inter, E, K, stream), "moe_gemm_down")


def q8l_bytes(rows, in_features) -> int:
    return int(_lib.lib().ntk_q8l_bytes(rows, in_features))


def q8l_pack(raw, rows, in_features, stream=None) -> "DeviceBuffer":
    """ntk_q8l_pack: the lane-major repack of a raw GGUF Q8_0 matrix (device buffer in, new device buffer out); read by gemv_rp_fused"""
    n = q8l_bytes(rows, in_features)
    if n == 0:
        raise _lib.NtkError(-2, "q8l_pack: shape without a lane-major form")
    dst = DeviceBuffer(n + 256)
    check(_lib.lib().ntk_q8l_pack(_p(dst), _p(raw), rows, in_features, stream), "q8l_pack")
    synchronize(stream)
    return dst


def q8l_unpack(packed, rows, in_features, nbytes, stream=None) -> "DeviceBuffer":
    """ntk_q8l_unpack: the GGUF Q8_0 blocks back from the lane-major form"""
    dst = DeviceBuffer(nbytes + 256)
    check(_lib.lib().ntk_q8l_unpack(_p(dst), _p(packed), rows, in_features, stream), "q8l_unpack")
    synchronize(stream)
    return dst


def rp_bytes(dtype, rows, in_features) -> int:
    return int(_lib.lib().ntk_rp_bytes(int(dtype), rows, in_features))


def rp_pack(raw, rows, in_features, dtype, stream=None) -> "DeviceBuffer":
    """ntk_rp_pack: the engine-owned repack of a raw GGUF K-quant matrix (device buffer in, new device buffer out)."""
    n = rp_bytes(dtype, rows, in_features)
    if n == 0:
        raise _lib.NtkError(-1, "rp_pack: dtype / shape without a repacked form")
    dst = DeviceBuffer(n + 256)
    check(_lib.lib().ntk_rp_pack(_p(dst), _p(raw), rows, in_features, int(dtype), stream), "rp_pack")
    synchronize(stream)   # `raw` may be released by the caller
    return dst


def rp_unpack(rp, rows, in_features, dtype, nbytes, stream=None) -> "DeviceBuffer":
    """ntk_rp_unpack: the raw GGUF blocks back from the engine's repacked form (nbytes = rows * row_bytes of the GGUF encoding)."""
    dst = DeviceBuffer(nbytes + 256)
    check(_lib.lib().ntk_rp_unpack(_p(dst), _p(rp), rows, in_features, int(dtype), stream), "rp_unpack")
    synchronize(stream)
    return dst


def gemv_rp_fused(segs: Sequence[tuple], x, in_features, norm_w=None, eps=0.0, resid=None, silu_pair=False, stream=None):
    """ntk_gemv_rp_fused: gemv_fused over REPACKED tensors: segs = [(rp, y, rows, dtype), ...] (<= 3; one or two K-quant formats)."""
    arr = (GemvSeg * len(segs))()
    for i, (W, y, rows, dt) in enumerate(segs):
        arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = _p(W), _p(y), rows, int(dt)
    check(_lib.lib().ntk_gemv_rp_fused(arr, len(segs), _p(x), in_features, _p(norm_w), eps, _p(resid), int(silu_pair),
                                       stream), "gemv_rp_fused")


ARENA_HIDDEN, ARENA_ATTN_OUT, ARENA_GATE = 1, 2, 3   # NTK_ARENA_* (include/ntk_engine.h)


def decode_arena_slot(slot: int) -> int:
    """device address of a static decode-activation slot (ntk_decode_arena_slot); write it with upload_to / read it with download_from"""
    p = _lib.lib().ntk_decode_arena_slot(int(slot))
    if not p:
        raise _lib.NtkError(-1, "ntk_decode_arena_slot(%d)" % slot)
    return int(p)


def upload_to(ptr: int, a: np.ndarray) -> None:
    a = np.ascontiguousarray(a)
    _lib.lib().nt_hip_memcpy_h2d(ptr, a.ctypes.data_as(C.c_void_p), a.nbytes)


def gemv_static_x() -> int:
    """the slot whose early-x form this thread's last lane-major Q8_0 launch took (0: the ordinary kernel)"""
    return int(_lib.lib().ntk_debug_gemv_static_x())


def _gemm_quant_f16(segs, X, n_tokens, in_features, resid=None, row_max=None, partials=None, stream=None, keep=None, repacked=False, workspace=None,
                    reuse_x=0, full_form=False):
    """ntk_gemm_quant_f16 behind its descriptor (include/ntk_engine.h: ntk_gemm_desc); segs = [(W, Y, rows, dtype), ...] of one format sharing X.  The
    workspace is allocated here (and kept alive in `keep` when the caller's next launch reads the deferred partial sums)."""
    L = _lib.lib()
    L.ntk_gemm_quant_workspace_bytes.restype = C.c_size_t
    n = int(L.ntk_gemm_quant_workspace_bytes(C.c_int(in_features), C.c_int(sum(r for _, _, r, _ in segs))))
    ws = workspace if workspace is not None else DeviceBuffer(n)   # (workspace: gemm_workspace(); with reuse_x = 1 its planes come from a *_prepare_x launch)
    arr = (GemvSeg * len(segs))()
    for i, (W, y, rows, dt) in enumerate(segs):
        arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = _p(W), _p(y), rows, int(dt)
    d = _lib.GemmDesc()
    d.segs, d.nseg, d.X, d.n_tokens, d.in_features, d.resid = arr, len(segs), _p(X), n_tokens, in_features, _p(resid)
    d.workspace, d.workspace_bytes, d.reuse_x, d.row_max = ws.ptr, n, int(reuse_x), _p(row_max)
    d.partials = C.pointer(partials) if partials is not None else None
    d.weights_repacked = 1 if repacked else 0
    d.full_form = 1 if full_form else 0   # the form of a full 1024-token pass whatever n_tokens is: chunking-independent bits
    L.ntk_gemm_quant_f16.argtypes = [C.POINTER(_lib.GemmDesc), C.c_void_p]
    st = L.ntk_gemm_quant_f16(C.byref(d), stream)
    if keep is not None:
        keep.append(ws)
    else:
        synchronize()   # `ws` is released when this returns
    return st


def gemm_quant_f16_prepared(segs, X, n_tokens, in_features, resid=None, row_max=None, stream=None):
    """-> a zero-argument callable that issues the same ntk_gemm_quant_f16 launch each time (descriptor and workspace built once: timing loops of tools/)"""
    L = _lib.lib()
    L.ntk_gemm_quant_workspace_bytes.restype = C.c_size_t
    n = int(L.ntk_gemm_quant_workspace_bytes(C.c_int(in_features), C.c_int(sum(r for _, _, r, _ in segs))))
    ws = DeviceBuffer(n)
    arr = (GemvSeg * len(segs))()
    for i, (W, y, rows, dt) in enumerate(segs):
        arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = _p(W), _p(y), rows, int(dt)
    d = _lib.GemmDesc()
    d.segs, d.nseg, d.X, d.n_tokens, d.in_features, d.resid = arr, len(segs), _p(X), n_tokens, in_features, _p(resid)
    d.workspace, d.workspace_bytes, d.reuse_x, d.row_max = ws.ptr, n, 0, _p(row_max)
    L.ntk_gemm_quant_f16.argtypes = [C.POINTER(_lib.GemmDesc), C.c_void_p]

    def call(_keep=(ws, arr, d)):
        return L.ntk_gemm_quant_f16(C.byref(d), stream)
    return call


def gemm_dense16_workspace(in_features, rows, dtype) -> "DeviceBuffer":
    """a workspace of ntk_gemm_dense16_workspace_bytes for F16 / BF16 matrices [rows][in_features]"""
    n = int(_lib.lib().ntk_gemm_dense16_workspace_bytes(in_features, rows, int(dtype)))
    if n == 0:
        raise _lib.NtkError(-1, "ntk_gemm_dense16_workspace_bytes: not a 16-bit dtype")
    return DeviceBuffer(n)


def gemm_dense16(segs, X, n_tokens, in_features, resid=None, workspace=None, reuse_x=0, repacked=False, stream=None) -> int:
    """ntk_gemm_dense16 (include/ntk_engine.h): segs = [(W, Y, rows, dtype), ...] F16 or BF16 matrices sharing X, on the 16-bit matrix cores.  Returns the
    status (a refusal launches nothing); synchronises when the workspace is allocated here."""
    ws = workspace if workspace is not None else DeviceBuffer(max(int(_lib.lib().ntk_gemm_dense16_workspace_bytes(in_features, sum(r for _, _, r, _ in segs), int(segs[0][3]))), 256))
    arr = (GemvSeg * len(segs))()
    for i, (W, y, rows, dt) in enumerate(segs):
        arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = _p(W), _p(y), rows, int(dt)
    d = _lib.GemmDesc()
    d.segs, d.nseg, d.X, d.n_tokens, d.in_features, d.resid = arr, len(segs), _p(X), n_tokens, in_features, _p(resid)
    d.workspace, d.workspace_bytes, d.reuse_x = _p(ws), ws.nbytes if isinstance(ws, DeviceBuffer) else (1 << 40), int(reuse_x)
    d.weights_repacked = 1 if repacked else 0
    st = _lib.lib().ntk_gemm_dense16(C.byref(d), stream)
    synchronize()
    return st


def gemm_quant_ws_multi(segs, X, n_tokens, in_features, stream=None, repacked=False):
    """several matrices of one format sharing X as one launch of the FP16 GEMM: segs = [(W, Y, rows, dtype), ...]"""
    return _gemm_quant_f16(segs, X, n_tokens, in_features, stream=stream, repacked=repacked)


def gemm_quant_ws(Y, W, X, n_tokens, out_features, in_features, dtype, resid=None, stream=None, repacked=False):
    """FP16-MFMA prompt projection, 64-token chunks, up to 1024 tokens per pass (repacked: W = the decode repack of the matrix, ops.rp_pack)"""
    st = _gemm_quant_f16([(W, Y, out_features, dtype)], X, n_tokens, in_features, resid=resid, stream=stream, repacked=repacked)
    synchronize()
    return st


def gemm_quant_ws_rm(Y, W, X, n_tokens, out_features, in_features, dtype, row_max, resid=None, stream=None):
    """the same with the tokens' largest |x| supplied (row_max: device floats [n_tokens]; None = computed by a pass over X)"""
    st = _gemm_quant_f16([(W, Y, out_features, dtype)], X, n_tokens, in_features, resid=resid, row_max=row_max, stream=stream)
    synchronize()
    return st


def gemm_deferred_then_consumer(kind, W, X, n_tokens, rows, in_features, dtype, row_max=None, **kw):
    """The prompt projections with their split-K sums folded into the consuming launch (include/ntk_engine.h: ntk_gemm_desc.partials).
    kind "norm": one matrix [rows][in] + ntk_reduce_rmsnorm_rowmax(kw: hidden, weight, eps, x_out, row_max_out, zero);
    kind "silu": W = (gate, up) + ntk_reduce_silu_mul_rowmax(kw: output, row_max_out).  Returns the launch's nsplit."""
    L = _lib.lib()
    pt = _lib.GemmPartials()
    keep = []
    if kind == "norm":
        y = DeviceBuffer(n_tokens * rows * 4)
        in_place = kw.get("in_place", True)   # Y = resid = hidden (the engine's form) or Y elsewhere and no residual input (the consumer adds Y)
        check(_gemm_quant_f16([(W, kw["hidden"] if in_place else y, rows, dtype)], X, n_tokens, in_features, resid=kw["hidden"] if in_place else None,
                              row_max=row_max, partials=pt, keep=keep), "gemm deferred")
        L.ntk_reduce_rmsnorm_rowmax.argtypes = [C.c_void_p, C.POINTER(_lib.GemmPartials), C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        check(L.ntk_reduce_rmsnorm_rowmax(_p(kw["hidden"]), C.byref(pt), _p(kw["weight"]), kw["eps"], _p(kw["x_out"]), _p(kw["row_max_out"]), _p(kw.get("zero")), None),
              "reduce_rmsnorm_rowmax")
    else:
        yg, yu = DeviceBuffer(n_tokens * rows * 4), DeviceBuffer(n_tokens * rows * 4)
        check(_gemm_quant_f16([(W[0], yg, rows, dtype), (W[1], yu, rows, dtype)], X, n_tokens, in_features, row_max=row_max, partials=pt, keep=keep),
              "gemm multi deferred")
        L.ntk_reduce_silu_mul_rowmax.argtypes = [C.c_void_p, C.POINTER(_lib.GemmPartials), C.c_void_p, C.c_void_p]
        check(L.ntk_reduce_silu_mul_rowmax(_p(kw["output"]), C.byref(pt), _p(kw["row_max_out"]), None), "reduce_silu_mul_rowmax")
    synchronize()
    return int(pt.nsplit)


def rope_kv_store(q, k, v, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, k_cache, v_cache, start_pos, max_seq):
    check(_lib.lib().ntk_rope_kv_store(_p(q), _p(k), _p(v), _p(positions), seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale,
                                       int(bool(interleaved)), _p(k_cache), _p(v_cache), start_pos, max_seq, None), "rope_kv_store")


def rope_kv_store_tab(q, k, v, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, k_cache, v_cache, start_pos, max_seq,
                      inv_freq=None):
    """ntk_rope_kv_store_tab: rope_kv_store with the frequency table (None: the in-kernel frequency)"""
    check(_lib.lib().ntk_rope_kv_store_tab(_p(q), _p(k), _p(v), _p(positions), seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale,
                                           int(bool(interleaved)), _p(k_cache), _p(v_cache), start_pos, max_seq, _p(inv_freq), None), "rope_kv_store_tab")


def gemm_workspace(in_features, rows):
    L = _lib.lib()
    L.ntk_gemm_quant_workspace_bytes.restype = C.c_size_t
    return DeviceBuffer(int(L.ntk_gemm_quant_workspace_bytes(C.c_int(in_features), C.c_int(rows))))


def prepare_x(kind, workspace, n_tokens, width, **kw):
    """The FP16 GEMM's operand pre-pass inside the launch that produces X (include/ntk_engine.h: ntk_*_prepare_x): planes, step sums and 1 / s of
    X[n_tokens][width] into `workspace`.  kind "x": X; "rmsnorm": output, input, weight, eps; "silu": output, gate, up;
    "reduce_rmsnorm": hidden, partials, weight, eps, x_out; "reduce_silu": output, partials."""
    L = _lib.lib()
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    if kind == "x":
        L.ntk_gemm_prepare_x.argtypes = [vp, i, i, vp, vp]
        st = L.ntk_gemm_prepare_x(_p(kw["X"]), n_tokens, width, workspace.ptr, None)
    elif kind == "rmsnorm":
        L.ntk_rmsnorm_prepare_x.argtypes = [vp, vp, vp, i, i, f, vp, vp]
        st = L.ntk_rmsnorm_prepare_x(_p(kw["output"]), _p(kw["input"]), _p(kw["weight"]), n_tokens, width, kw["eps"], workspace.ptr, None)
    elif kind == "silu":
        L.ntk_silu_mul_prepare_x.argtypes = [vp, vp, vp, i, i, vp, vp]
        st = L.ntk_silu_mul_prepare_x(_p(kw["output"]), _p(kw["gate"]), _p(kw["up"]), n_tokens, width, workspace.ptr, None)
    elif kind == "reduce_rmsnorm":
        L.ntk_reduce_rmsnorm_prepare_x.argtypes = [vp, C.POINTER(_lib.GemmPartials), vp, f, vp, vp, vp]
        st = L.ntk_reduce_rmsnorm_prepare_x(_p(kw["hidden"]), C.byref(kw["partials"]), _p(kw["weight"]), kw["eps"], _p(kw["x_out"]), workspace.ptr, None)
    else:
        L.ntk_reduce_silu_mul_prepare_x.argtypes = [vp, C.POINTER(_lib.GemmPartials), vp, vp]
        st = L.ntk_reduce_silu_mul_prepare_x(_p(kw["output"]), C.byref(kw["partials"]), workspace.ptr, None)
    synchronize()
    return st


def launch_rmsnorm_rowmax(output, input, weight, n_tokens, hidden_size, eps, row_max, zero_tokens=None, stream=None):
    check(_lib.lib().ntk_rmsnorm_rowmax(_p(output), _p(input), _p(weight), n_tokens, hidden_size, eps, _p(row_max), _p(zero_tokens), stream), "rmsnorm_rowmax")


def launch_silu_mul_rowmax(output, gate, up, n_tokens, width, row_max, stream=None):
    check(_lib.lib().ntk_silu_mul_rowmax(_p(output), _p(gate), _p(up), n_tokens, width, _p(row_max), stream), "silu_mul_rowmax")


def sample_top_k(logits, n, recent, n_recent, repeat_penalty, temperature, top_k, top_p, r, d_out, stream=None):
    """ntk_sample_top_k: the reference sampler on the device; logits are penalised in place; token id to d_out (device int)."""
    L = _lib.lib()
    L.ntk_sample_scratch_bytes.restype = C.c_size_t
    scratch = DeviceBuffer(int(L.ntk_sample_scratch_bytes(C.c_int(n))))
    L.ntk_sample_top_k.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    st = L.ntk_sample_top_k(_p(logits), n, _p(recent), n_recent, repeat_penalty, temperature, top_k, top_p, r, _p(d_out), None,
                            _p(scratch), stream)
    synchronize()
    return st


def sample_rows_top_k(logits, n_rows, vocab, ld, recent, recent_ld, rows, d_out, stream=None, null=()):
    """ntk_sample_rows_top_k: the sampler over the rows of a batched step, each with its own settings.  logits: device F32 [n_rows][ld], penalised in
    place; recent: device int32 [n_rows][recent_ld]; rows: a list of (temperature, top_k, top_p, repeat_penalty, r, n_recent) per row, or a ready
    _lib.SampleRows; token ids to d_out (device int32 [n_rows]).  Returns the status.  null: names of pointer arguments to pass as NULL (the refusals)."""
    L = _lib.lib()
    if not isinstance(rows, _lib.SampleRows):
        sr = _lib.SampleRows()
        for b, (temperature, top_k, top_p, repeat_penalty, r, n_recent) in enumerate(rows):
            sr.temperature[b], sr.top_k[b], sr.top_p[b], sr.repeat_penalty[b], sr.r[b], sr.n_recent[b] = temperature, top_k, top_p, repeat_penalty, r, n_recent
        rows = sr
    scratch = DeviceBuffer(int(L.ntk_sample_rows_scratch_bytes(min(max(n_rows, 1), 16), min(max(vocab, 1), 1 << 20))))
    arg = lambda name, v: None if name in null else v
    st = L.ntk_sample_rows_top_k(arg("logits", _p(logits)), n_rows, vocab, ld, _p(recent), recent_ld, arg("rows", C.pointer(rows)), arg("d_out", _p(d_out)), None,
                                 arg("scratch", _p(scratch)), stream)
    synchronize()   # `scratch` is released when this returns
    return st


def gemm_quant(Y, W, X, n_tokens, out_features, in_features, dtype, resid=None, stream=None):
    """Y[t,:] = W . X[t,:] (+ resid[t,:]) for a chunk of prompt tokens: one pass over W per 16 tokens (ntk_gemm_quant)."""
    check(_lib.lib().ntk_gemm_quant(_p(Y), _p(W), _p(X), n_tokens, out_features, in_features, int(dtype), _p(resid),
                                    stream), "gemm_quant")


def attention_decode_fused(output, q, k, v, k_cache, v_cache, d_pos, n_heads, n_kv_heads, head_dim, max_seq, scale,
                           theta_base, freq_scale=1.0, inv_freq=None, stream=None):
    check(_lib.lib().ntk_attention_decode_fused(_p(output), _p(q), _p(k), _p(v), _p(k_cache), _p(v_cache), _p(d_pos),
                                                _p(inv_freq), n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base,
                                                freq_scale, stream), "attention_decode_fused")


def attention_decode_split(output, q, k, v, k_cache, v_cache, d_pos, n_heads, n_kv_heads, head_dim, max_seq, scale,
                           theta_base, nsplit, freq_scale=1.0, inv_freq=None, stream=None):
    """Long-context decode attention: nsplit workgroups per head + a merge launch (ntk_attention_decode_split)."""
    scratch = DeviceBuffer(int(_lib.lib().ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit)))
    check(_lib.lib().ntk_attention_decode_split(_p(output), _p(q), _p(k), _p(v), _p(k_cache), _p(v_cache), _p(d_pos),
                                                _p(inv_freq), n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base,
                                                freq_scale, nsplit, _p(scratch), stream), "attention_decode_split")
    synchronize()   # `scratch` is released when this returns
    return None


def attention_decode_split_merged(output, q, k, v, k_cache, v_cache, d_pos, n_heads, n_kv_heads, head_dim, max_seq, scale,
                                  theta_base, nsplit, freq_scale=1.0, inv_freq=None, stream=None, launches=1):
    """The same as ONE launch (ntk_attention_decode_split_merged): the last workgroup of a head merges; `launches` > 1 repeats the launch on
    the same scratch (the arrival counters must come back to zero each time)."""
    scratch = DeviceBuffer(int(_lib.lib().ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit)))
    check(_lib.lib().ntk_attention_split_scratch_init(_p(scratch), n_heads, stream), "attention_split_scratch_init")
    for _ in range(launches):
        check(_lib.lib().ntk_attention_decode_split_merged(_p(output), _p(q), _p(k), _p(v), _p(k_cache), _p(v_cache), _p(d_pos),
                                                           _p(inv_freq), n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base,
                                                           freq_scale, nsplit, _p(scratch), stream), "attention_decode_split_merged")
    synchronize()
    return None


def attention_decode_batch(output, q, k, v, k_caches, v_caches, positions, n_rows, n_heads, n_kv_heads, head_dim, max_seq, scale,
                           theta_base, nsplit=1, freq_scale=1.0, inv_freq=None, stream=None, table=True):
    """Decode attention of n_rows sequences, each with its own caches (k_caches / v_caches: lists of DeviceBuffers) and its own position
    (positions: device int [n_rows]): ntk_attention_decode_batch.  table=False passes a NULL cache table (the refusal)."""
    L = _lib.lib()
    kv = _lib.KvBatch()
    for b, (kc, vc) in enumerate(zip(k_caches, v_caches)):
        kv.k[b], kv.v[b] = _p(kc), _p(vc)
    scratch = DeviceBuffer(max(n_rows, 1) * int(L.ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit)))
    check(L.ntk_attention_decode_batch(_p(output), _p(q), _p(k), _p(v), C.addressof(kv) if table else None, _p(positions), n_rows, _p(inv_freq),
                                       n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, freq_scale, nsplit, _p(scratch), stream),
          "attention_decode_batch")
    synchronize()   # `scratch` is released when this returns
    return None


def kv_segments(segments, k_caches=None, v_caches=None, n_seg=None, row0=None):
    """An ntk_kv_segments descriptor from segments = [(n_rows, start_pos), ...] laid back to back from row 0 (row0: other first rows, for the refusal
    tests) and the segments' caches (DeviceBuffers, raw addresses or None = NULL); n_seg overrides the count."""
    d = _lib.KvSegments()
    d.n_seg = len(segments) if n_seg is None else n_seg
    row = 0
    for s, (n, start) in enumerate(segments[:16]):
        d.row0[s], d.n_rows[s], d.start_pos[s] = (row if row0 is None else row0[s]), n, start
        row += n
        for side, caches in ((d.k, k_caches), (d.v, v_caches)):
            c = caches[s] if caches is not None else None
            side[s] = c if c is None or isinstance(c, int) else _p(c)
    return d


def kv_segments_validate(desc, total_rows, max_seq) -> int:
    """ntk_kv_segments_validate (host only): NTK_OK, NTK_E_SHAPE or NTK_E_NULL; desc: a _lib.KvSegments or None"""
    return int(_lib.lib().ntk_kv_segments_validate(C.addressof(desc) if desc is not None else None, int(total_rows), int(max_seq)))


def rope_kv_store_segments(q, k, v, desc, n_heads, n_kv_heads, head_dim, theta_base, max_seq, freq_scale=1.0, interleaved=False, stream=None) -> int:
    """ntk_rope_kv_store_segments: RoPE of q (in place) and the F16 store of the rotated k and of v for every segment of a packed pass, one launch; returns
    the status (the caller checks it: the refusal tests read it)"""
    return int(_lib.lib().ntk_rope_kv_store_segments(_p(q), _p(k), _p(v), C.addressof(desc) if desc is not None else None, n_heads, n_kv_heads, head_dim,
                                                     theta_base, freq_scale, int(interleaved), max_seq, stream))


def rope_kv_store_segments_tab(q, k, v, desc, n_heads, n_kv_heads, head_dim, theta_base, max_seq, freq_scale=1.0, interleaved=False, inv_freq=None,
                               stream=None) -> int:
    """ntk_rope_kv_store_segments_tab: rope_kv_store_segments with the frequency table (None: the in-kernel frequency); returns the status"""
    return int(_lib.lib().ntk_rope_kv_store_segments_tab(_p(q), _p(k), _p(v), C.addressof(desc) if desc is not None else None, n_heads, n_kv_heads,
                                                         head_dim, theta_base, freq_scale, int(interleaved), max_seq, _p(inv_freq), stream))


def attention_prefill_segments(output, Q, desc, n_heads, n_kv_heads, head_dim, max_seq, scale, stream=None) -> int:
    """ntk_attention_prefill_segments: causal prompt attention of every segment of a packed pass over its own caches; returns the status"""
    return int(_lib.lib().ntk_attention_prefill_segments(_p(output), _p(Q), C.addressof(desc) if desc is not None else None, n_heads, n_kv_heads, head_dim,
                                                         max_seq, scale, stream))


def embed_rows(out, table, tokens, n_tokens, hidden, dtype, stream=None, allow_unsupported=False):
    st = _lib.lib().ntk_embed_rows(_p(out), _p(table), _p(tokens), n_tokens, hidden, int(dtype), stream)
    if not (allow_unsupported and st == -1):
        check(st, "embed_rows")
    return st


def argmax(logits, n, d_out_token, scratch, h_mirror=None, stream=None):
    check(_lib.lib().ntk_argmax(_p(logits), n, _p(d_out_token), _p(h_mirror), _p(scratch), stream), "argmax")


def logprob_rows(logits, n_rows, vocab, ld, targets, logprob, top1=None, stream=None):
    """ntk_logprob_rows: logprob[r] = log softmax(logits[r, :vocab])[targets[r]] (0 where targets[r] < 0), top1[r] (optional) = the row's first maximum;
    logits: device F32 [n_rows][ld], targets / top1: device int32 [n_rows]"""
    check(_lib.lib().ntk_logprob_rows(_p(logits), n_rows, vocab, ld, _p(targets), _p(logprob), _p(top1), stream), "logprob_rows")


def advance_pos(d_pos, stream=None):
    check(_lib.lib().ntk_advance_pos(_p(d_pos), stream), "advance_pos")


def sclk_mhz(stream=None) -> float:
    """ntk_debug_sclk: the shader clock right now, MHz (one wave spinning for ~50 us; blocking)"""
    import numpy as np
    b = DeviceBuffer.zeros(24)
    check(_lib.lib().ntk_debug_sclk(_p(b), stream), "sclk probe")
    synchronize(stream)
    v = b.numpy(np.uint64)
    return 100.0 * float(v[0]) / max(float(v[1]), 1.0)


class SclkSpan:
    """with SclkSpan() as c: <work on the compute stream, synchronised before the block ends> ; c.mhz = the average shader clock of the
    span (ntk_debug_sclk_begin / _end: a one-wave kernel beside the work, on the library's second stream)"""

    def __enter__(self):
        L = _lib.lib()
        self.flag, self.out = DeviceBuffer.zeros(8), DeviceBuffer.zeros(24)
        self.mhz = None
        check(L.ntk_debug_sclk_begin(_p(self.flag), _p(self.out), L.ntk_stream(1)), "sclk begin")
        return self

    def __exit__(self, *exc):
        import numpy as np
        L = _lib.lib()
        check(L.ntk_debug_sclk_end(_p(self.flag), L.ntk_stream(2)), "sclk end")
        check(L.ntk_stream_synchronize(L.ntk_stream(2)), "sync")
        check(L.ntk_stream_synchronize(L.ntk_stream(1)), "sync")
        v = self.out.numpy(np.uint64)
        if v[1] > 0:
            self.mhz = 100.0 * float(v[0]) / float(v[1])
        return False
