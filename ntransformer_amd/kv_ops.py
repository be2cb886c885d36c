"""KV cache sequence operations seen from Python: ctypes wrappers of ntk_kv_shift / ntk_kv_shift_q8 (csrc/kv_ops.hip) and the numpy checkers of the
context shift (tests/test_kv_ops_cpu.py, tests/test_kv_shift_gpu.py, tests/test_kv_ops_engine_gpu.py).

The rotation contract (include/ntk_engine.h): pair i turns by angle = float32(delta) * freq_i * freq_scale, evaluated in float32 left to right, delta =
dst0 - src0; freq_i = inv_freq[i] or, without a table, 1 / float32(pow(float64(theta), float64(float32(2 i) / head_dim))); a' = a c - b s, b' = a s + b c;
the pair is (i, i + head_dim / 2), or (2 i, 2 i + 1) when interleaved.  The checkers rotate the STORED values in float64 with cos / sin of that float32
angle, then round to half (F16) or requantise with kv_q8.quantize_q8_0 (Q8)."""
from __future__ import annotations

import numpy as np

from . import _lib
from . import kv_q8
from .ops import _p, check


# ---------------------------------------------------------------------------------------------- numpy side
def pair_freqs(head_dim: int, theta: float = 10000.0, inv_freq=None) -> np.ndarray:
    """float32 [head_dim / 2]: the table as given, or the forward kernels' expression"""
    if inv_freq is not None:
        f = np.ascontiguousarray(inv_freq, dtype=np.float32)
        assert f.shape == (head_dim // 2,)
        return f
    i = np.arange(head_dim // 2, dtype=np.float32)
    e = (np.float32(2.0) * i) / np.float32(head_dim)
    return (np.float32(1.0) / np.power(np.float64(np.float32(theta)), e.astype(np.float64)).astype(np.float32)).astype(np.float32)


def shift_angles(delta: int, head_dim: int, theta: float = 10000.0, inv_freq=None, freq_scale: float = 1.0) -> np.ndarray:
    """float32 [head_dim / 2]: float32(delta) * freq * freq_scale, left to right"""
    return ((np.float32(delta) * pair_freqs(head_dim, theta, inv_freq)).astype(np.float32) * np.float32(freq_scale)).astype(np.float32)


def rotate_f64(x: np.ndarray, delta: int, head_dim: int, theta: float = 10000.0, inv_freq=None, freq_scale: float = 1.0,
               interleaved: bool = False) -> np.ndarray:
    """x [..., n_heads * head_dim] (any real dtype) rotated by `delta` positions, in float64 with the float32 angle of the contract"""
    x = np.asarray(x, np.float64)
    h = x.reshape(x.shape[:-1] + (x.shape[-1] // head_dim, head_dim))
    ang = shift_angles(delta, head_dim, theta, inv_freq, freq_scale).astype(np.float64)
    c, s = np.cos(ang), np.sin(ang)
    out = np.empty_like(h)
    if interleaved:
        a, b = h[..., 0::2], h[..., 1::2]
        out[..., 0::2] = a * c - b * s
        out[..., 1::2] = a * s + b * c
    else:
        a, b = h[..., :head_dim // 2], h[..., head_dim // 2:]
        out[..., :head_dim // 2] = a * c - b * s
        out[..., head_dim // 2:] = a * s + b * c
    return out.reshape(x.shape)


def pair_max(x: np.ndarray, head_dim: int, interleaved: bool = False) -> np.ndarray:
    """max(|a|, |b|) of every element's pair, in x's shape [..., n_heads * head_dim] (the magnitude the rounding bars scale with)"""
    m = np.abs(np.asarray(x, np.float64))
    h = m.reshape(m.shape[:-1] + (m.shape[-1] // head_dim, head_dim))
    out = np.empty_like(h)
    if interleaved:
        p = np.maximum(h[..., 0::2], h[..., 1::2])
        out[..., 0::2] = p
        out[..., 1::2] = p
    else:
        p = np.maximum(h[..., :head_dim // 2], h[..., head_dim // 2:])
        out[..., :head_dim // 2] = p
        out[..., head_dim // 2:] = p
    return out.reshape(m.shape)


def shift_f16_ref(k_halves: np.ndarray, v_halves: np.ndarray, src0: int, dst0: int, n_rows: int, head_dim: int, theta: float = 10000.0,
                  inv_freq=None, freq_scale: float = 1.0, interleaved: bool = False):
    """The context shift of F16 caches: k_halves, v_halves uint16 [..., max_seq, n_kv_heads * head_dim] -> new (k, v) of the same shape.  Rows
    [src0, src0 + n_rows) go to [dst0, ...): V as it is, K rotated by dst0 - src0 positions in float64 and rounded to half (nearest even); every other
    row is returned unchanged."""
    k = np.array(k_halves, dtype=np.uint16, copy=True)
    v = np.array(v_halves, dtype=np.uint16, copy=True)
    assert 0 <= dst0 < src0 and n_rows >= 1 and src0 + n_rows <= k.shape[-2]
    src_k = np.ascontiguousarray(k_halves[..., src0:src0 + n_rows, :], dtype=np.uint16)
    rot = rotate_f64(src_k.view(np.float16).astype(np.float64), dst0 - src0, head_dim, theta, inv_freq, freq_scale, interleaved)
    k[..., dst0:dst0 + n_rows, :] = rot.astype(np.float16).view(np.uint16)
    v[..., dst0:dst0 + n_rows, :] = np.ascontiguousarray(v_halves[..., src0:src0 + n_rows, :], dtype=np.uint16)
    return k, v


def shift_q8_ref(k_blocks: np.ndarray, v_blocks: np.ndarray, src0: int, dst0: int, n_rows: int, head_dim: int = 128, theta: float = 10000.0,
                 inv_freq=None, freq_scale: float = 1.0, interleaved: bool = False):
    """The context shift of 8-bit caches in canonical blocks: uint8 [..., max_seq, n_kv_heads * head_dim / 32, 34] -> new (k, v).  V blocks move as they
    are; K rows are dequantised exactly (half(d) * q), rotated in float64, and requantised with kv_q8.quantize_q8_0."""
    k = np.array(k_blocks, dtype=np.uint8, copy=True)
    v = np.array(v_blocks, dtype=np.uint8, copy=True)
    assert 0 <= dst0 < src0 and n_rows >= 1 and src0 + n_rows <= k.shape[-3]
    src_k = np.ascontiguousarray(k_blocks[..., src0:src0 + n_rows, :, :], dtype=np.uint8)
    rot = rotate_f64(kv_q8.dequantize_exact(src_k), dst0 - src0, head_dim, theta, inv_freq, freq_scale, interleaved)
    d, q = kv_q8.quantize_q8_0(rot.astype(np.float32))
    k[..., dst0:dst0 + n_rows, :, :] = kv_q8.to_blocks(d, q)
    v[..., dst0:dst0 + n_rows, :, :] = np.ascontiguousarray(v_blocks[..., src0:src0 + n_rows, :, :], dtype=np.uint8)
    return k, v


# ---------------------------------------------------------------------------------------------- device side
def kv_shift_status(k_cache, v_cache, n_layers, max_seq, n_kv_heads, head_dim, src0, dst0, n_rows, inv_freq=None, theta_base=10000.0, freq_scale=1.0,
                    interleaved=0, stream=None) -> int:
    """ntk_kv_shift over F16 caches [n_layers][max_seq][n_kv_heads][head_dim] (device); inv_freq: device float32 [head_dim / 2] or None.  The status."""
    return int(_lib.lib().ntk_kv_shift(_p(k_cache), _p(v_cache), n_layers, max_seq, n_kv_heads, head_dim, src0, dst0, n_rows, _p(inv_freq), theta_base,
                                       freq_scale, int(interleaved), stream))


def kv_shift(*args, **kw) -> None:
    check(kv_shift_status(*args, **kw), "kv_shift")


def kv_shift_q8_status(k_cache, v_cache, n_layers, max_seq, n_kv_heads, head_dim, src0, dst0, n_rows, inv_freq=None, theta_base=10000.0, freq_scale=1.0,
                       interleaved=0, stream=None) -> int:
    """ntk_kv_shift_q8 over n_layers consecutive 8-bit layer buffers of kv_q8.cache_bytes(max_seq, n_kv_heads, head_dim) bytes each.  The status."""
    return int(_lib.lib().ntk_kv_shift_q8(_p(k_cache), _p(v_cache), n_layers, max_seq, n_kv_heads, head_dim, src0, dst0, n_rows, _p(inv_freq), theta_base,
                                          freq_scale, int(interleaved), stream))


def kv_shift_q8(*args, **kw) -> None:
    check(kv_shift_q8_status(*args, **kw), "kv_shift_q8")


def q8_planes_to_blocks(raw: np.ndarray, n_layers: int, max_seq: int, row: int) -> np.ndarray:
    """the bytes of n_layers consecutive 8-bit layer buffers -> canonical blocks uint8 [n_layers, max_seq, row / 32, 34]"""
    lb = raw.size // n_layers
    out = np.empty((n_layers, max_seq, row // 32, 34), np.uint8)
    for l in range(n_layers):
        buf = np.ascontiguousarray(raw[l * lb:(l + 1) * lb])
        q = buf[:max_seq * row].view(np.int8).reshape(max_seq, row // 32, 32)
        d = buf[max_seq * row:max_seq * row + max_seq * (row // 32) * 2].view(np.float16).reshape(max_seq, row // 32)
        out[l] = kv_q8.to_blocks(d, q)
    return out


def q8_blocks_to_planes(blocks: np.ndarray, layer_bytes: int) -> np.ndarray:
    """canonical blocks uint8 [n_layers, max_seq, row / 32, 34] -> the bytes of n_layers consecutive layer buffers (the padding behind a layer: zero)"""
    n_layers, max_seq, nb = blocks.shape[:3]
    row = nb * 32
    out = np.zeros(n_layers * layer_bytes, np.uint8)
    for l in range(n_layers):
        d, q = kv_q8.from_blocks(blocks[l])
        o = l * layer_bytes
        out[o:o + max_seq * row] = np.ascontiguousarray(q).reshape(-1).view(np.uint8)
        out[o + max_seq * row:o + max_seq * row + max_seq * nb * 2] = np.ascontiguousarray(d).reshape(-1).view(np.uint8)
    return out
