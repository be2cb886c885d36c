"""The FP8 (OCP E4M3) KV cache seen from Python: the numpy encoder, the exact decoder, the layout, and ctypes wrappers of the ntk_*_fp8 entry
points (the counterpart of kv_q8.py; the float64 attention the tests check against is kv_q8.attention_f64).

A code is S.EEEE.MMM, bias 7: (-1)^S * 2^(E - 7) * (1 + M / 8) for E > 0, (-1)^S * 2^-6 * M / 8 for E = 0; no infinities, S.1111.111 = NaN; the
largest value is 448 (0x7E).  Device form (csrc/attention_fp8.hip): per layer and side ONE buffer, uint8 [max_seq][row]."""
from __future__ import annotations

import numpy as np

from . import _lib
from .ops import DeviceBuffer, _p, check, synchronize

MAX = 448.0


def decode_e4m3(codes: np.ndarray) -> np.ndarray:
    """uint8 codes -> float32, exactly (0x7F / 0xFF -> NaN)"""
    c = np.ascontiguousarray(codes, dtype=np.uint8).astype(np.int32)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    mag = np.where((e == 15) & (m == 7), np.nan, mag)
    return np.where(c & 0x80, -mag, mag).astype(np.float32)


def encode_e4m3(x: np.ndarray) -> np.ndarray:
    """float32 -> uint8 codes: round to nearest, ties to even, saturating at +-448 (infinities included); NaN -> S.1111.111.
    In float64 (every step exact): the spacing at |x| is 2^(max(floor(log2 |x|), -6) - 3), and np.rint rounds ties to even."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = np.minimum(np.abs(x.astype(np.float64)), MAX)
    with np.errstate(all="ignore"):
        ex = np.maximum(np.floor(np.log2(np.where(a > 0, a, 1.0))), -6.0)
        step = 2.0 ** (ex - 3.0)
        r = np.rint(np.where(np.isnan(a), 0.0, a) / step) * step          # an exact multiple of the step; may reach the next binade
        ex2 = np.maximum(np.floor(np.log2(np.where(r > 0, r, 1.0))), -6.0)
        sub = r < 2.0 ** -6
        code = np.where(sub, r * 2.0 ** 9, ((ex2 + 7.0) * 8.0) + (r / 2.0 ** ex2 - 1.0) * 8.0).astype(np.int32)
    code = np.where(np.isnan(x), 0x7F, code)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def decode_f16(codes: np.ndarray) -> np.ndarray:
    """what ntk_kv_dequant_fp8_f16 writes: the exact values as half bits (uint16)"""
    return decode_e4m3(codes).astype(np.float16).view(np.uint16)


def cache_bytes(max_seq: int, n_kv_heads: int, head_dim: int) -> int:
    return int(_lib.lib().ntk_kv_fp8_cache_bytes(max_seq, n_kv_heads, head_dim))


class Fp8Cache:
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

    def write_rows(self, pos0: int, codes: np.ndarray) -> None:
        self.buf.upload(np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1), pos0 * self.row)

    def read_rows(self, pos0: int, n: int) -> np.ndarray:
        return self.buf.numpy(np.uint8, n * self.row, pos0 * self.row).reshape(n, self.row)


def kv_store_fp8(kc: Fp8Cache, vc: Fp8Cache, k, v, seq_len, n_kv_heads, head_dim, start_pos, stream=None):
    check(_lib.lib().ntk_kv_store_fp8(_p(kc), _p(vc), _p(k), _p(v), seq_len, n_kv_heads, head_dim, start_pos, kc.max_seq, stream), "kv_store_fp8")


def rope_kv_store_fp8(q, k, v, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, kc: Fp8Cache, vc: Fp8Cache, start_pos, freq_scale=1.0,
                      interleaved=0, inv_freq=None, tab=False, stream=None):
    """ntk_rope_kv_store_fp8, or with tab=True its _tab form (inv_freq None: the in-kernel frequency)"""
    L = _lib.lib()
    head = (_p(q), _p(k), _p(v), _p(positions), seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, _p(kc), _p(vc), start_pos,
            kc.max_seq)
    st = L.ntk_rope_kv_store_fp8_tab(*head, _p(inv_freq), stream) if tab else L.ntk_rope_kv_store_fp8(*head, stream)
    check(st, "rope_kv_store_fp8")


def kv_dequant_fp8_f16(k16, v16, kc: Fp8Cache, vc: Fp8Cache, n_rows, n_kv_heads, head_dim, stream=None):
    check(_lib.lib().ntk_kv_dequant_fp8_f16(_p(k16), _p(v16), _p(kc), _p(vc), n_rows, n_kv_heads, head_dim, kc.max_seq, stream), "kv_dequant_fp8_f16")


def attention_decode_fp8_status(output, q, k, v, k_cache, v_cache, d_pos, n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, nsplit,
                                freq_scale=1.0, inv_freq=None, stream=None) -> int:
    scratch = DeviceBuffer(int(_lib.lib().ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit)))
    st = _lib.lib().ntk_attention_decode_fp8(_p(output), _p(q), _p(k), _p(v), _p(k_cache), _p(v_cache), _p(d_pos), _p(inv_freq), n_heads, n_kv_heads,
                                             head_dim, max_seq, scale, theta_base, freq_scale, nsplit, _p(scratch), stream)
    synchronize()   # `scratch` is released when this returns
    return int(st)


def attention_decode_fp8(*args, **kw) -> None:
    check(attention_decode_fp8_status(*args, **kw), "attention_decode_fp8")
