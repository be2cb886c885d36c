"""The 8-bit (Q8_0) KV cache seen from Python: the numpy quantiser, the block <-> device-plane conversion, a float64 GQA attention
over arbitrary real K / V (the checkers of tests/test_kv_q8_*.py), and ctypes wrappers of the ntk_kv_*_q8 entry points.

Canonical form: GGUF block_q8_0 = {half d; int8 q[32]} (34 bytes), a row of n_kv_heads * head_dim elements = that many / 32 blocks.
Device form (csrc/attention_q8.hip): per layer and side ONE buffer -- int8 quants [max_seq][row], then half scales [max_seq][row / 32]."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .ops import DeviceBuffer, _p, check, synchronize


# ---------------------------------------------------------------------------------------------- numpy side
def quantize_q8_0(x: np.ndarray):
    """ggml quantize_row_q8_0_ref in float32: x [..., 32 m] -> (d float16 [..., m], q int8 [..., m, 32]).
    amax over the block, d = amax / 127, id = d ? 1 / d : 0, q = roundf(x * id) (ties away from zero), d stored RNE.
    Where ggml is undefined (a subnormal amax makes 1 / d infinite): x * id = NaN counts as 0, the product is clamped to +-127."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    xb = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    with np.errstate(all="ignore"):
        amax = np.abs(xb).max(axis=-1)
        d = (amax / np.float32(127.0)).astype(np.float32)
        inv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
        t = (xb * inv[..., None]).astype(np.float32)
        t = np.where(np.isnan(t), np.float32(0.0), t)
        t = np.clip(t, np.float32(-127.0), np.float32(127.0)).astype(np.float64)   # (float64: |t| + 0.5 is exact, so this IS roundf)
        q = (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int8)
        dh = d.astype(np.float16)
    return dh, q


def to_blocks(d: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(d [..., m] float16, q [..., m, 32] int8) -> canonical bytes uint8 [..., m, 34]"""
    out = np.empty(q.shape[:-1] + (34,), np.uint8)
    out[..., :2] = np.ascontiguousarray(d, dtype=np.float16)[..., None].view(np.uint8)
    out[..., 2:] = np.ascontiguousarray(q, dtype=np.int8).view(np.uint8)
    return out


def from_blocks(blocks: np.ndarray):
    """canonical bytes uint8 [..., m, 34] -> (d float16 [..., m], q int8 [..., m, 32])"""
    b = np.ascontiguousarray(blocks, dtype=np.uint8)
    d = np.ascontiguousarray(b[..., :2]).view(np.float16)[..., 0]
    q = np.ascontiguousarray(b[..., 2:]).view(np.int8)
    return d, q


def dequantize_exact(blocks: np.ndarray) -> np.ndarray:
    """half(d) * q, exact (float64) -- what the decode kernel uses: [..., m, 34] -> [..., 32 m]"""
    d, q = from_blocks(blocks)
    v = d.astype(np.float64)[..., None] * q.astype(np.float64)
    return v.reshape(v.shape[:-2] + (v.shape[-2] * 32,))


def dequantize_f16(blocks: np.ndarray) -> np.ndarray:
    """half_rne(float32(half(d)) * q) as uint16 bits -- what ntk_kv_dequant_q8_f16 writes"""
    d, q = from_blocks(blocks)
    with np.errstate(all="ignore"):
        v = (d.astype(np.float32)[..., None] * q.astype(np.float32)).astype(np.float16)
    return v.reshape(v.shape[:-2] + (v.shape[-2] * 32,)).view(np.uint16)


def attention_f64(q: np.ndarray, K: np.ndarray, V: np.ndarray, n_heads: int, n_kv_heads: int, head_dim: int, scale: float) -> np.ndarray:
    """GQA decode attention in float64 over real-valued K, V [n_keys, n_kv_heads * head_dim]; q [n_heads * head_dim] -> [n_heads * head_dim]"""
    n = K.shape[0]
    qh = np.asarray(q, np.float64).reshape(n_heads, head_dim)
    Kh = np.asarray(K, np.float64).reshape(n, n_kv_heads, head_dim)
    Vh = np.asarray(V, np.float64).reshape(n, n_kv_heads, head_dim)
    group = n_heads // n_kv_heads
    out = np.empty((n_heads, head_dim), np.float64)
    for h in range(n_heads):
        g = h // group
        s = (Kh[:, g, :] @ qh[h]) * float(scale)
        p = np.exp(s - s.max())
        out[h] = (p[:, None] * Vh[:, g, :]).sum(axis=0) / p.sum()
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------- device side
def cache_bytes(max_seq: int, n_kv_heads: int, head_dim: int) -> int:
    return int(_lib.lib().ntk_kv_q8_cache_bytes(max_seq, n_kv_heads, head_dim))


class Q8Cache:
    """One layer's K or V cache in the device layout"""

    def __init__(self, max_seq: int, n_kv_heads: int, head_dim: int, fill: int = 0):
        self.max_seq, self.row = max_seq, n_kv_heads * head_dim
        self.nbytes = cache_bytes(max_seq, n_kv_heads, head_dim)
        self.buf = DeviceBuffer(self.nbytes)
        _lib.lib().nt_hip_memset(self.buf.ptr, fill, self.nbytes)

    @property
    def ptr(self):
        return self.buf.ptr

    def __int__(self):   # (ops._p: passes as a device pointer)
        return int(self.buf.ptr)

    def write_blocks(self, pos0: int, blocks: np.ndarray) -> None:
        """canonical blocks uint8 [n, row / 32, 34] -> rows [pos0, pos0 + n)"""
        d, q = from_blocks(blocks)
        self.buf.upload(np.ascontiguousarray(q).reshape(-1), pos0 * self.row)
        self.buf.upload(np.ascontiguousarray(d).reshape(-1), self.max_seq * self.row + pos0 * (self.row // 32) * 2)

    def read_blocks(self, pos0: int, n: int) -> np.ndarray:
        q = self.buf.numpy(np.int8, n * self.row, pos0 * self.row).reshape(n, self.row // 32, 32)
        d = self.buf.numpy(np.float16, n * (self.row // 32), self.max_seq * self.row + pos0 * (self.row // 32) * 2).reshape(n, self.row // 32)
        return to_blocks(d, q)

    def raw(self) -> np.ndarray:
        return self.buf.numpy(np.uint8)


def kv_store_q8(kc: Q8Cache, vc: Q8Cache, k, v, seq_len, n_kv_heads, head_dim, start_pos, stream=None):
    check(_lib.lib().ntk_kv_store_q8(_p(kc), _p(vc), _p(k), _p(v), seq_len, n_kv_heads, head_dim, start_pos, kc.max_seq, stream), "kv_store_q8")


def rope_kv_store_q8(q, k, v, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, kc: Q8Cache, vc: Q8Cache, start_pos, freq_scale=1.0,
                     interleaved=0, stream=None):
    check(_lib.lib().ntk_rope_kv_store_q8(_p(q), _p(k), _p(v), _p(positions), seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale,
                                          interleaved, _p(kc), _p(vc), start_pos, kc.max_seq, stream), "rope_kv_store_q8")


def rope_kv_store_q8_tab(q, k, v, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, kc: Q8Cache, vc: Q8Cache, start_pos, freq_scale=1.0,
                         interleaved=0, inv_freq=None, stream=None):
    """ntk_rope_kv_store_q8_tab: rope_kv_store_q8 with the frequency table (None: the in-kernel frequency)"""
    check(_lib.lib().ntk_rope_kv_store_q8_tab(_p(q), _p(k), _p(v), _p(positions), seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale,
                                              interleaved, _p(kc), _p(vc), start_pos, kc.max_seq, _p(inv_freq), stream), "rope_kv_store_q8_tab")


def kv_dequant_q8_f16(k16, v16, kc: Q8Cache, vc: Q8Cache, n_rows, n_kv_heads, head_dim, stream=None):
    check(_lib.lib().ntk_kv_dequant_q8_f16(_p(k16), _p(v16), _p(kc), _p(vc), n_rows, n_kv_heads, head_dim, kc.max_seq, stream), "kv_dequant_q8_f16")


def attention_decode_q8_status(output, q, k, v, k_cache, v_cache, d_pos, n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, nsplit,
                               freq_scale=1.0, inv_freq=None, stream=None, launches=1) -> int:
    scratch = DeviceBuffer(int(_lib.lib().ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit)))
    st = 0
    for _ in range(launches):
        st = _lib.lib().ntk_attention_decode_q8(_p(output), _p(q), _p(k), _p(v), _p(k_cache), _p(v_cache), _p(d_pos), _p(inv_freq), n_heads,
                                                n_kv_heads, head_dim, max_seq, scale, theta_base, freq_scale, nsplit, _p(scratch), stream)
        if st != 0:
            break
    synchronize()   # `scratch` is released when this returns
    return int(st)


def attention_decode_q8(*args, **kw) -> None:
    check(attention_decode_q8_status(*args, **kw), "attention_decode_q8")


def attention_decode_q8_batch_status(output, q, k, v, caches, positions, n_rows, n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, nsplit,
                                     freq_scale=1.0, inv_freq=None, stream=None, table=True, scratch=True) -> int:
    """ntk_attention_decode_q8_batch: the decode attention of n_rows sequences over their own 8-bit caches.  caches: a list of (K, V) Q8Cache pairs, one
    per row (None for a NULL entry); positions: device int [n_rows].  table=False passes a NULL table, scratch=False a NULL scratch (the refusals).
    Returns the status."""
    L = _lib.lib()
    kv = _lib.KvBatch()
    for b, pair in enumerate(caches):
        kv.k[b], kv.v[b] = (_p(pair[0]), _p(pair[1])) if pair is not None else (None, None)
    buf = DeviceBuffer(max(n_rows, 1) * int(L.ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit))) if scratch else None
    st = L.ntk_attention_decode_q8_batch(_p(output), _p(q), _p(k), _p(v), C.addressof(kv) if table else None, _p(positions), n_rows, _p(inv_freq),
                                         n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, freq_scale, nsplit, _p(buf), stream)
    synchronize()   # `buf` is released when this returns
    return int(st)


def attention_decode_q8_batch(*args, **kw) -> None:
    check(attention_decode_q8_batch_status(*args, **kw), "attention_decode_q8_batch")
