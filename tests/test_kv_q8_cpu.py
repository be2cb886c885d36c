"""The 8-bit (Q8_0) KV cache, host side: the numpy quantiser and float64 attention the GPU tests check against (ntransformer_amd/kv_q8.py)
are themselves tied to GGUF's Q8_0 dequantisation and to the oracle; the option and the symbols exist without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ntransformer_amd import _lib, gguf, kv_q8
from ntransformer_amd import engine as E
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNEL_SYMBOLS = ["ntk_kv_q8_cache_bytes", "ntk_kv_store_q8", "ntk_rope_kv_store_q8", "ntk_attention_decode_q8", "ntk_kv_dequant_q8_f16"]
NEW_ENGINE_SYMBOLS = ["nt_engine_kv_cache_bytes", "nt_engine_debug_kv_read_q8", "nt_engine_debug_kv_write_q8"]


def rng(seed):
    return np.random.default_rng(20261017 + seed)


def test_quantiser_reconstructs_within_half_a_step_through_gguf_dequantize():
    r = rng(1)
    x = (r.standard_normal((64, 1024)) * r.choice([0.05, 1.0, 40.0], (64, 1))).astype(np.float32)   # (d stays a normal half: relative rounding 2^-11)
    d, q = kv_q8.quantize_q8_0(x)
    blocks = kv_q8.to_blocks(d, q)
    assert blocks.shape == (64, 32, 34)
    back = gguf.dequantize(blocks.tobytes(), gguf.GGML_Q8_0, x.size).reshape(x.shape)
    # d / 2 per element holds for the quantiser's own (unrounded F32) d = amax / 127 -- up to the two F32 roundings of 1 / d and x * id, each
    # <= 2^-24 of |x * id| <= 127 -- ...
    d32 = (np.abs(x.reshape(64, 32, 32)).max(axis=-1) / np.float32(127.0)).astype(np.float64)
    exact32 = (d32[..., None] * q.astype(np.float64)).reshape(x.shape)
    assert (np.abs(exact32 - x) <= np.repeat(d32, 32, axis=-1) * (0.5 + 127 * 2.0 ** -23)).all()
    # ... and through gguf.dequantize, which multiplies by the STORED half d (RNE: within 2^-11 of d, so each value moves by <= 127 * 2^-11 d more)
    assert (np.abs(d.astype(np.float64) - d32) <= d32 * 2.0 ** -11).all()
    step = np.repeat(d32, 32, axis=-1)
    assert (np.abs(back.astype(np.float64) - x) <= step * (0.5 + 127 * 2.0 ** -11 + 127 * 2.0 ** -23)).all()
    assert np.array_equal(back, kv_q8.dequantize_exact(blocks).astype(np.float32))   # the exact product IS the GGUF dequantisation


def test_quantiser_zero_blocks_extremes_and_ties():
    x = np.zeros((1, 128), np.float32)
    x[0, 32:64] = np.linspace(-3.0, 3.0, 32, dtype=np.float32)           # holds -amax and +amax
    x[0, 64] = 127.0; x[0, 65] = 0.5; x[0, 66] = -2.5; x[0, 67] = 1.5   # d = 1: exact ties, away from zero
    x[0, 96] = 1e-40                                                     # subnormal amax
    d, q = kv_q8.quantize_q8_0(x)
    assert d[0, 0] == 0 and not q[0, 0].any()
    assert q[0, 1, 0] == -127 and q[0, 1, 31] == 127
    assert d[0, 2] == 1.0 and list(q[0, 2, :4]) == [127, 1, -3, 2]
    assert d[0, 3] == 0 and q[0, 3, 0] == 127 and not q[0, 3, 1:].any()  # the pinned undefined case: 1 / d = inf


def test_float64_attention_is_tied_to_the_oracle_on_an_f16_cache():
    r = rng(2)
    for seq, nh, nkv, hd in [(1, 8, 2, 128), (300, 32, 8, 128), (1025, 16, 2, 128), (77, 5, 1, 128)]:
        kc = r.standard_normal(seq * nkv * hd).astype(np.float16).view(np.uint16)
        vc = r.standard_normal(seq * nkv * hd).astype(np.float16).view(np.uint16)
        q = r.standard_normal(nh * hd).astype(np.float32)
        scale = float(1 / np.sqrt(hd))
        ref = O.attention_decode(q, kc, vc, seq, nh, nkv, hd, seq, scale)
        got = kv_q8.attention_f64(q, kc.view(np.float16).reshape(seq, nkv * hd), vc.view(np.float16).reshape(seq, nkv * hd), nh, nkv, hd, scale)
        err = float(np.abs(got - ref).max())
        print("seq %d nh %d nkv %d: |f64 - oracle| = %.3g" % (seq, nh, nkv, err))
        assert err <= 3e-5


def test_kv_cache_option_is_validated_without_a_gpu():
    eng = E.Engine()
    try:
        with pytest.raises(_lib.NtkError) as ei:
            eng.set_option("kv_cache", "bogus")
        assert "bogus" in str(ei.value)
        eng.set_option("kv_cache", "q8_0")
        eng.set_option("kv_cache", "f16")
    finally:
        eng.close()


def test_header_declares_and_library_exports_the_new_symbols():
    L = _lib.lib()
    eng_h = open(os.path.join(ROOT, "include", "ntk_engine.h")).read()
    pub_h = open(os.path.join(ROOT, "include", "ntransformer.h")).read()
    for name in NEW_KERNEL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, eng_h), name
        assert getattr(L, name)
    for name in NEW_ENGINE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, pub_h), name
        assert getattr(L, name)
    assert "kv_cache" in pub_h
    L.ntk_kv_q8_cache_bytes.restype = C.c_size_t
    assert L.ntk_kv_q8_cache_bytes(4096, 8, 128) == 4096 * 1024 * 17 // 16   # 1.0625 bytes per element
    assert L.ntk_kv_q8_cache_bytes(4096, 8, 100) == 0
